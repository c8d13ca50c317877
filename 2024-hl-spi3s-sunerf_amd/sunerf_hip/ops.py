"""Tensor-level wrappers over the C ABI: argument validation, output allocation, current-stream plumbing.

PyTorch is used for device memory and streams only; every numerical op of the render path runs in the HIP
kernels of ``csrc/``.
"""
import ctypes
import functools
import os
import threading
from typing import Optional, Sequence, Tuple

import torch

from . import lib as _l
from ._ffi import _dev, _ptr, _ptr_array, _stream, _workspace

SAMPLER_STRATIFIED = 0
SAMPLER_SPHERICAL = 1
SUPPORTED_D_FILTER = (64, 128, 256, 512)
TRAINABLE_D_FILTER = (64, 128, 256, 512)
PRECISION_FAST, PRECISION_EXACT, PRECISION_HALF = 0, 1, 2     # include/sunerf_hip.h: SUNERF_PRECISION_*
PRECISION_AUTO = -1           # host-side policy (not a kernel mode): FAST while a probe shows it inside the gate, else EXACT
PRECISION_NAMES = {PRECISION_FAST: 'fast', PRECISION_EXACT: 'exact', PRECISION_HALF: 'half', PRECISION_AUTO: 'auto'}

# AUTO policy.  FAST (fp16 head + two fp8 correction products) behaves like arithmetic with ~58x the rounding noise of the
# fp32 reference, EXACT (three fp16 products) like ~7x (tests/tools/precision_scan.py): both are far inside
# the north-star gate (1e-4 relative) for freshly initialised and for trained networks, but the noise of ANY arithmetic
# -- the reference's included -- is amplified by the network's conditioning, and with all hidden weights x 4 FAST leaves
# the gate while EXACT stays inside.  So the mode is chosen by MEASUREMENT: every PROBE_EVERY-th parameter version (and the
# first) PROBE_RAYS rays spread evenly over the render call at hand are rendered in both modes and compared in gate units,
#     max_ray |fast - exact| / (1e-4 |exact| + 1e-6 max|exact|)      over image, height_map, absorption_map,
# FAST is kept while that stays below PROBE_LIMIT.  Calibration (tests/tools/probe_calibration.py, hidden weights x 1 ... x 4, two seeds):
# with 144 rays the probe tracks FAST's true worst gate units against the fp32 reference within 10 % (x 2: probe 0.37 / 0.38, true
# 0.32 / 0.41; x 3: 0.40 / 0.49, true 0.43 / 0.47; x 4: 1.19 / 0.92, true 1.26 / 0.95), so 0.5 keeps FAST below ~0.55 of the gate.
PROBE_EVERY = 64
PROBE_RAYS = 144
PROBE_LIMIT = 0.5
# The FIRST probe of an image is read at once (one 4-byte device -> host copy: nothing is known about the network yet); later
# re-probes are ASYNCHRONOUS: the measured units go to a pinned host word behind an event and the decision is taken by the first
# render call that finds the event complete -- the training step never waits for a probe.  Under a process group the units are
# MAX-all-reduced first, so every rank takes the same arithmetic at the same parameter version (equal step times, no rank-dependent
# forward).
PROBE_ASYNC = True
# Under a process group the decision of an asynchronous probe is taken at a DETERMINISTIC point -- the first render call at
# least PROBE_APPLY_AFTER parameter versions after the probe (its event has long completed by then; the call synchronises on it
# to be sure) -- not whenever event.query() first returns true, which differs from rank to rank.  Every rank takes part in the
# MAX all-reduce of the units whatever its own batch looks like (an empty batch contributes 0).
PROBE_APPLY_AFTER = 2
probe_group = None            # process group of the probe's all-reduce (None = the default group); ClipAdam(group=...) sets it


def _probe_world() -> int:
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_world_size(probe_group)
    return 1


def default_precision(d_filter: int) -> int:
    """Forward arithmetic of newly packed models: ``SUNERF_FORWARD_PRECISION`` = ``auto`` (default: ``fast`` guarded by the
    probe above), ``fast`` (fp16 head product + two block-scaled fp8 correction products), ``exact`` (three fp16
    products per term) or ``half`` (opt-in: single fp16 operands -- the bf16-class arithmetic of BASELINE config 3; NOT
    within 1e-4 of the fp32 reference)."""
    mode = os.environ.get('SUNERF_FORWARD_PRECISION', 'auto').lower()
    names = {v: k for k, v in PRECISION_NAMES.items()}
    if mode not in names:
        raise ValueError(f"SUNERF_FORWARD_PRECISION must be one of {sorted(names)}, not {mode!r}")
    return names[mode]


BACKWARD_PRECISIONS = ('default', 'exact')


def backward_precision() -> str:
    """Arithmetic of the MLP backward: ``SUNERF_BACKWARD_PRECISION`` = ``default`` (unset: the fp16 kernels, the fp32 one for
    batches of at most ``exact_backward_limit()`` samples) or ``exact`` (every batch with query points in fp32, whatever its size:
    ``sunerf_mlp_backward_exact_chunked``; the training forwards then write no activation stash).  With
    ``SUNERF_FORWARD_PRECISION=exact`` this is fp32-class training end to end."""
    mode = os.environ.get('SUNERF_BACKWARD_PRECISION', 'default').strip().lower() or 'default'
    if mode not in BACKWARD_PRECISIONS:
        raise ValueError(f"SUNERF_BACKWARD_PRECISION must be one of {list(BACKWARD_PRECISIONS)}, not {mode!r}")
    return mode


def _stash_wanted(training: bool) -> bool:
    """A training forward writes the activation stash unless the backward will recompute the activations in fp32."""
    return training and backward_precision() != 'exact'


_workspaces = {}                        # (device, stream) -> scratch of the d_filter = 512 render kernel
STASH_FP16, STASH_PHASE = 0, 1          # include/sunerf_hip.h: SUNERF_STASH_*


def stash_format_of(stash, n_rays: int, n_samples: int, packed) -> int:
    """The format a stash tensor was written in, told by its size (the two formats differ by almost 2 x): the size of this batch
    exactly, or -- a stash of more rays used for its first ``n_rays`` (both formats are ray-major) -- a whole number of chunks of
    one format only."""
    lib = _l.load()
    need = {fmt: lib.sunerf_act_stash_bytes(n_rays, n_samples, packed.d_filter, packed.n_linear, fmt) for fmt in (STASH_PHASE, STASH_FP16)}
    for fmt, nbytes in need.items():
        if nbytes and stash.numel() == nbytes:
            return fmt
    chunk = {fmt: lib.sunerf_act_stash_bytes(1, 1, packed.d_filter, packed.n_linear, fmt) // 2 for fmt in need}     # (1 chunk + 1 spare)
    fits = [fmt for fmt, nbytes in need.items() if nbytes and stash.numel() > nbytes and stash.numel() % chunk[fmt] == 0]
    if len(fits) == 1:
        return fits[0]
    raise ValueError('the activation stash does not have the size of either format for this batch')


class _DeferredWord:
    """A device scalar on its way to the host: copied into a pinned word behind an event on the current stream of ``device``.
    What is done with it, and when, is the policy of its owner (the two probes below differ in that)."""

    def __init__(self, scalar: torch.Tensor, device):
        self.host = torch.empty(1, dtype=torch.float32, pin_memory=True)
        self.host.copy_(scalar, non_blocking=True)
        self.event = torch.cuda.Event()
        self.event.record(torch.cuda.current_stream(device))

    def ready(self, wait: bool = False) -> bool:
        """Has the word arrived (``wait``: blocks until it has)?  Once it has, ``float(self.host[0])`` is the scalar."""
        if wait:
            self.event.synchronize()
        return wait or self.event.query()


class PackedMLP:
    """fp16 hi/lo A-fragment image of one NeRF MLP (see csrc/sunerf_common.h).  Re-pack after every
    parameter update (``repack``)."""

    def __init__(self, weights: Sequence[torch.Tensor], biases: Sequence[torch.Tensor], precision: Optional[int] = None):
        self.n_linear = len(weights)
        # Any width up to 512 and both input forms of NeRF (model.py:28-33) run on the compiled kernels by ZERO PADDING, which is
        # exact: a padded hidden unit has zero weights and bias, sin(0) = 0, and zero outgoing weights; a first layer without
        # positional encoding, Linear(4, d), is the 84-input layer with its weights in the four raw-coordinate columns (reference
        # columns 0..3 of the encoder output, model.py:127-132) and zeros under the 80 sin / cos features.
        self.d_model = int(weights[0].shape[0])
        self.d_in = int(weights[0].shape[1])
        if self.d_model < 1 or self.d_model > SUPPORTED_D_FILTER[-1]:
            raise ValueError(f'd_filter={self.d_model} is outside 1..{SUPPORTED_D_FILTER[-1]}')
        if self.d_in not in (4, 84):
            raise ValueError('the first layer takes the 84 positional-encoding features or the 4 raw coordinates')
        self.d_filter = next(d for d in SUPPORTED_D_FILTER if d >= self.d_model)
        self.padded = self.d_filter != self.d_model or self.d_in != 84
        precision = default_precision(self.d_filter) if precision is None else int(precision)
        self.auto = precision == PRECISION_AUTO
        self.precision = PRECISION_FAST if self.auto else precision          # the kernel mode of `buffer`
        self.probe_due = self.auto
        self.last_probe = None            # gate units measured by the last probe (AUTO only)
        self._versions_since_probe = 0
        self._pending_probe = None        # (_DeferredWord, sensitivity, version, collective) of a probe whose result has not been read yet
        self._version = 0                 # parameter version: counts the (re)packs
        self._alt_buffer = None           # image of the OTHER arithmetic (AUTO): what the probe compares against, what a mode change swaps in
        self._alt_version = None          # the parameter version `_alt_buffer` holds, None: re-pack it on use
        # the W^T probe of the pipelined backward (_pipe_w_probe below): its two sets of scratch gradients, its word in flight, the
        # parameter version it ran at, the last measured difference, and the decision taken from it (single fp16 W^T)
        self._pipe_probe_bufs = self._pipe_w_pending = self._pipe_probe_version = self.pipe_w_probe = None
        self.pipe_hi_only = False
        # evaluation/loader.py:226-229 calls the renderer from a ThreadPoolExecutor: (re)packing, probing and the buffer swap of
        # a mode change are serialised; a render call works on the (buffer, precision) pair it read under the lock
        self._lock = threading.RLock()
        self.d_out = int(weights[-1].shape[0])
        lib = _l.load()
        nbytes = lib.sunerf_packed_mlp_bytes(self.d_filter, self.n_linear)
        if nbytes == 0:
            raise ValueError(f'unsupported MLP shape: d_filter={self.d_filter}, n_linear={self.n_linear}')
        self.device = weights[0].device
        self.buffer = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self.buffer_t = None        # transposed image for the backward pass, packed on demand
        self._t_valid = False
        self._keepalive = None      # (weights, biases): the fp32 parameters of the last (re)pack in the kernel shapes, see kernel_params
        self._pad_w = self._pad_b = None        # zero-padded models: the kernel-shaped copies of the parameters ...
        self._pad_gw = self._pad_gb = None      # ... and the kernel-shaped gradients the backward kernels write (stage_grads)
        self.repack(weights, biases)

    def _shapes(self, d_in: int, d: int):
        return [((self.d_out if i == self.n_linear - 1 else d, d_in if i == 0 else d), (self.d_out if i == self.n_linear - 1 else d,))
                for i in range(self.n_linear)]            # [(weight shape, bias shape)] with the given input and hidden widths

    def kernel_shapes(self):
        """[(weight shape, bias shape)] of the (padded) network the kernels see."""
        return self._shapes(84, self.d_filter)

    def model_shapes(self):
        """[(weight shape, bias shape)] of the model's own nn.Linear layers."""
        return self._shapes(self.d_in, self.d_model)

    def kernel_shaped(self, make=torch.empty):
        """(weights, biases): new fp32 device tensors of ``kernel_shapes``."""
        f32 = dict(dtype=torch.float32, device=self.device)
        return [make(ws, **f32) for ws, _ in self.kernel_shapes()], [make(bs, **f32) for _, bs in self.kernel_shapes()]

    def _padded(self, weights, biases):
        """Copies the model's parameters into zero-initialised tensors of the kernel's shapes (device copies only)."""
        if self._pad_w is None:
            self._pad_w, self._pad_b = self.kernel_shaped(torch.zeros)
        for W, b, pw, pb in zip(weights, biases, self._pad_w, self._pad_b):
            pw[:W.shape[0], :W.shape[1]].copy_(W.detach())
            pb[:b.shape[0]].copy_(b.detach())
        return self._pad_w, self._pad_b

    def repack(self, weights: Sequence[torch.Tensor], biases: Sequence[torch.Tensor]):
        assert len(weights) == self.n_linear and len(biases) == self.n_linear
        if self.padded:
            for i, (w, b, (w_shape, b_shape)) in enumerate(zip(weights, biases, self.model_shapes())):
                _dev(w.detach(), f'weight[{i}]', w_shape); _dev(b.detach(), f'bias[{i}]', b_shape)
            weights, biases = self._padded(weights, biases)
        ws, bs = [], []
        for i, (w, b, (w_shape, b_shape)) in enumerate(zip(weights, biases, self.kernel_shapes())):
            ws.append(_dev(w.detach(), f'weight[{i}]', w_shape))
            bs.append(_dev(b.detach(), f'bias[{i}]', b_shape))
        self._keepalive = (ws, bs)
        self._pack_into(self.buffer, self.precision)
        self._t_valid = False
        self._version += 1
        if self.auto:
            self._versions_since_probe += 1
            if self._versions_since_probe >= PROBE_EVERY:
                self.probe_due = True

    def kernel_params(self):
        """(weights, biases): the fp32 parameters of the last (re)pack in ``kernel_shapes`` -- the model's own tensors, the zero-padded
        copies for a padded model -- for the packers and the fp32 backward kernels (kept alive here until those have run)."""
        return self._keepalive

    def _pack_into(self, buffer: torch.Tensor, precision: int):
        ws, bs = self.kernel_params()
        _l.call(self.device, 'sunerf_pack_mlp', _ptr_array(ws), _ptr_array(bs), self.n_linear, self.d_filter, self.d_out, precision,
                _ptr(buffer), _stream(self.device))

    def stage_grads(self, grad_weights: Sequence[torch.Tensor], grad_biases: Sequence[torch.Tensor], accumulate: bool):
        """Checks the caller's gradient buffers (per layer one contiguous fp32 tensor of the model's shape) -> ``(kernel weights, kernel
        biases, kernel accumulate, fold)``: what a backward kernel writes, and the step to run after it.  These are the caller's own
        buffers and a no-op, unless the model is zero-padded (``__init__``): then the kernel fills staging buffers of the padded shapes
        and ``fold`` copies (``accumulate``: adds) their leading blocks, the model's gradients, into the caller's (the padding's own
        gradients are discarded: those weights are not parameters)."""
        if len(grad_weights) != self.n_linear or len(grad_biases) != self.n_linear:
            raise ValueError('one weight and one bias gradient buffer per layer')
        for i, (gw, gb, (w_shape, b_shape)) in enumerate(zip(grad_weights, grad_biases, self.model_shapes())):
            if gw.shape != w_shape or gb.shape != b_shape or gw.dtype != torch.float32 or gb.dtype != torch.float32 \
                    or not gw.is_contiguous() or not gb.is_contiguous():
                raise ValueError(f'grad buffer {i} has the wrong shape / layout')
        if not self.padded:
            return grad_weights, grad_biases, accumulate, lambda: None
        if self._pad_gw is None:
            self._pad_gw, self._pad_gb = self.kernel_shaped()
        pad_w, pad_b = self._pad_gw, self._pad_gb
        into = torch.Tensor.add_ if accumulate else torch.Tensor.copy_

        def fold():
            for gw, gb, pw, pb in zip(grad_weights, grad_biases, pad_w, pad_b):
                into(gw, pw[:gw.shape[0], :gw.shape[1]])
                into(gb, pb[:gb.shape[0]])
        return pad_w, pad_b, False, fold

    def image_for_call(self, probe=None):
        """``(image buffer, kernel precision)`` of one forward call, read under the lock: this call's image, whatever other threads
        decide next.  Before that a finished probe's decision is taken and, when one is due (AUTO), ``probe()`` runs it on the caller's rays."""
        with self._lock:
            self._apply_probe()
            if self.auto and self.probe_due and probe is not None:
                probe()
            return self.buffer, self.precision

    def probe(self, rays_o, rays_d, times, z_vals, reg_radius: float, sensitivity: float = 1.0) -> float:
        """AUTO: renders PROBE_RAYS rays of the call in both arithmetics, keeps FAST if it is inside the gate with margin,
        switches this image to EXACT otherwise (and back when a later probe allows it).  One 4-byte device -> host read
        per PROBE_EVERY parameter versions.  Returns the measured gate units.  ``sensitivity``: how much more strongly than
        the emission image the caller's own integral reacts to an error of the raw output (the density-temperature image goes
        with exp(2 raw_0): 2) -- the measured units are multiplied by it."""
        total = rays_o.shape[0]
        n = min(PROBE_RAYS, total)
        self.probe_due = False
        self._versions_since_probe = 0
        world = _probe_world()
        if n == 0 and world <= 1:
            return 0.0
        units = torch.zeros(1, dtype=torch.float32, device=self.device)
        if n > 0:
            # PROBE_RAYS rays spread evenly over the call (the first rays of a frame are an off-disk corner of the image)
            sel = slice(0, (total // n) * n, total // n)
            rays_o, rays_d, z_vals = rays_o[sel].contiguous(), rays_d[sel].contiguous(), z_vals[sel].contiguous()
            times = times.reshape(-1)[sel].contiguous()
            if self._alt_buffer is None:
                self._alt_buffer = torch.empty_like(self.buffer)
            other = PRECISION_EXACT if self.precision == PRECISION_FAST else PRECISION_FAST
            self._pack_into(self._alt_buffer, other)
            self._alt_version = self._version
            views = {self.precision: self.buffer, other: self._alt_buffer}
            outs = {mode: _emission_render(self, image, mode, rays_o, rays_d, times, z_vals, reg_radius, want_epilogues=True)
                    for mode, image in views.items()}
            for k in ('image', 'height_map', 'absorption_map'):
                f, e = outs[PRECISION_FAST][k].reshape(-1), outs[PRECISION_EXACT][k].reshape(-1)
                # absorption_map = sum(1 - a): the reference forms 1 - a in fp32, i.e. with 2^-24 absolute noise per sample.
                # The 1e-6 max|exact| term is NOT part of the parity gate (tests/conftest.py:gate_units is purely relative): it
                # keeps rays whose exact value is (next to) zero -- off-disk rays of a frame -- from deciding the arithmetic of
                # the whole image by 0 / 0; it can only make the probe more lenient on rays 1e-2 below the brightest one.
                floor = z_vals.shape[1] * 6e-8 if k == 'absorption_map' else 0.0
                units = torch.maximum(units, ((f - e).abs() / (1e-4 * e.abs() + 1e-6 * e.abs().max() + floor)).max())
            units = torch.nan_to_num(units, nan=float('inf'))      # NaN: non-finite outputs in either mode -> EXACT; the finite check reports them
        if world > 1:
            import torch.distributed as dist
            # every rank probes at the same parameter version and takes part whatever its own batch holds: one decision
            dist.all_reduce(units, op=dist.ReduceOp.MAX, group=probe_group)
        first = self.last_probe is None
        self._pending_probe = (_DeferredWord(units, self.device), float(sensitivity), self._version, world > 1)
        self._apply_probe(block=first or not PROBE_ASYNC)
        return self.last_probe

    def _apply_probe(self, block: bool = False) -> None:
        """Takes the decision of a finished probe (``block``: waits for it)."""
        pending = self._pending_probe
        if pending is None:
            return
        word, sensitivity, version, collective = pending
        if collective and not block:
            # ranks must switch at the same parameter version: a fixed distance behind the probe, not "when the event is seen"
            if self._version < version + PROBE_APPLY_AFTER:
                return
        if not word.ready(wait=block or collective):
            return
        self._pending_probe = None
        units = float(word.host[0]) * sensitivity
        self.last_probe = units
        want = PRECISION_FAST if units <= PROBE_LIMIT else PRECISION_EXACT
        if want != self.precision:
            # A render call of another thread may still hold (self.buffer, old precision) as the pair it read under the lock:
            # the live buffer is never re-packed in another arithmetic.  The image of the wanted mode goes into the alternate
            # buffer (the probe left it there if the parameters have not changed since) and the two are swapped.
            if self._alt_version != self._version:
                self._alt_buffer = torch.empty_like(self.buffer)      # a fresh one: the old alternate may be some call's snapshot too
                self._pack_into(self._alt_buffer, want)
            self.buffer, self._alt_buffer = self._alt_buffer, self.buffer
            self.precision = want
            self._alt_version = None       # what is now the alternate holds the OTHER mode of this version at best: re-pack on use

    def wait_probe(self) -> Optional[float]:
        """Blocks until a probe in flight has been read and its decision taken; returns the last measured gate units."""
        with self._lock:
            self._apply_probe(block=True)
            return self.last_probe

    def transposed(self) -> torch.Tensor:
        """fp16 W^T image consumed by sunerf_mlp_dgrad (packed lazily, once per parameter version)."""
        if self.buffer_t is None:
            self.buffer_t = torch.empty(_l.load().sunerf_packed_mlp_t_bytes(self.d_filter, self.n_linear), dtype=torch.uint8,
                                        device=self.device)
        if not self._t_valid:
            _l.call(self.device, 'sunerf_pack_mlp_t', _ptr_array(self.kernel_params()[0]), self.n_linear, self.d_filter, self.d_out,
                    _ptr(self.buffer_t), _stream(self.device))
            self._t_valid = True
        return self.buffer_t


def sample_z(kind: int, rays_o, rays_d, t_vals, distance: float, solar_R: float,
             t_rand: Optional[torch.Tensor] = None) -> torch.Tensor:
    n = rays_o.shape[0]
    rays_o = _dev(rays_o, 'rays_o', (n, 3))
    rays_d = _dev(rays_d, 'rays_d', (n, 3))
    t_vals = _dev(t_vals.reshape(-1), 't_vals')
    s = t_vals.numel()
    if t_rand is not None:
        t_rand = _dev(t_rand, 't_rand', (n, s))
    z = torch.empty(n, s, dtype=torch.float32, device=rays_o.device)
    _l.call(rays_o.device, 'sunerf_sample_z', kind, _ptr(rays_o), _ptr(rays_d), _ptr(t_vals), _ptr(t_rand), n, s,
            float(distance), float(solar_R), _ptr(z), _stream(rays_o.device))
    return z


def _forward_scratch(packed: PackedMLP, dev, n_rays: int, n_samples: int, training: bool):
    """What a forward launch of ``n_rays`` x ``n_samples`` needs beside its outputs -> ``(workspace or None, its bytes, stash or None,
    stash format)``: the scratch of the d_filter = 512 render kernel, and for a training forward the activation stash in the format
    of the backward that is going to read it (none under ``SUNERF_BACKWARD_PRECISION=exact``)."""
    lib = _l.load()
    ws_bytes = lib.sunerf_render_workspace_bytes(packed.d_filter)
    ws = _workspace(_workspaces, dev, ws_bytes) if ws_bytes else None
    stash, fmt = None, STASH_FP16
    if _stash_wanted(training):
        fmt = training_stash_format(packed, n_rays, n_samples)
        stash = torch.empty(lib.sunerf_act_stash_bytes(n_rays, n_samples, packed.d_filter, packed.n_linear, fmt), dtype=torch.uint8,
                            device=dev)
    return ws, ws_bytes, stash, fmt


def emission_render_fwd(packed: PackedMLP, rays_o, rays_d, times, z_vals, reg_radius: float,
                        want_raw: bool = False, want_epilogues: bool = False, training: bool = False,
                        probe_sensitivity: float = 1.0):
    """One fused render pass.  Returns dict(image (N,1), weights (N,S), absorption (N,S)[, raw (N,S,2)]
    [, height_map (N,), absorption_map (N,), regularization (N,S)][, stash]).  ``training=True`` also writes the
    activation stash needed by :func:`emission_render_bwd` (and implies ``want_raw``); under
    ``SUNERF_BACKWARD_PRECISION=exact`` the backward does not read one and ``stash`` is None."""
    n, s = z_vals.shape
    rays_o = _dev(rays_o, 'rays_o', (n, 3))
    rays_d = _dev(rays_d, 'rays_d', (n, 3))
    times = _dev(times.reshape(-1), 'times', (n,))
    z_vals = _dev(z_vals, 'z_vals', (n, s))
    if packed.device != z_vals.device:
        raise _l.SunerfHipError('packed weights and rays are on different devices')
    image, precision = packed.image_for_call(lambda: packed.probe(rays_o, rays_d, times, z_vals, reg_radius, probe_sensitivity))
    return _emission_render(packed, image, precision, rays_o, rays_d, times, z_vals, reg_radius, want_raw, want_epilogues, training)


def _emission_render(packed: PackedMLP, image, precision: int, rays_o, rays_d, times, z_vals, reg_radius: float,
                     want_raw: bool = False, want_epilogues: bool = False, training: bool = False):
    """:func:`emission_render_fwd` on validated inputs with a GIVEN packed image and its arithmetic (the call's own, or one of the
    two the probe compares)."""
    n, s = z_vals.shape
    dev = z_vals.device
    f32 = dict(dtype=torch.float32, device=dev)
    out = {'image': torch.empty(n, 1, **f32), 'weights': torch.empty(n, s, **f32),
           'absorption': torch.empty(n, s, **f32)}
    want_raw = want_raw or training
    if training and packed.d_filter not in TRAINABLE_D_FILTER:
        raise NotImplementedError(f'training with d_filter={packed.d_filter} is not implemented (inference only); '
                                  f'trainable widths: {TRAINABLE_D_FILTER}')
    ws, ws_bytes, stash, fmt = _forward_scratch(packed, dev, n, s, training)
    raw = torch.empty(n, s, 2, **f32) if want_raw else None
    hm = am = reg = None
    if want_epilogues:
        hm, am, reg = torch.empty(n, **f32), torch.empty(n, **f32), torch.empty(n, s, **f32)
    _l.call(dev, 'sunerf_emission_render_fwd', _ptr(image), packed.d_filter, packed.n_linear,
            precision, _ptr(rays_o), _ptr(rays_d), _ptr(times), _ptr(z_vals), n, s, _ptr(out['image']),
            _ptr(out['weights']), _ptr(out['absorption']), _ptr(raw), _ptr(hm), _ptr(am), _ptr(reg),
            float(reg_radius), _ptr(stash), fmt, _ptr(ws), ws_bytes, _stream(dev))
    if want_raw:
        out['raw'] = raw
    if training:
        out['stash'] = stash
    if want_epilogues:
        out.update(height_map=hm, absorption_map=am, regularization=reg)
    return out


def mlp_points_fwd(packed: PackedMLP, points: torch.Tensor, training: bool = False):
    """NeRF.forward on free-standing points (M, 4) -> dict(raw (M, 2)[, stash, n_padded]).  The points are padded to whole
    32-point chunks; ``training=True`` also writes the activation stash :func:`mlp_backward` needs (with ``g_raw`` of shape
    (n_padded / 32, 32, 2)); ``stash`` is None under ``SUNERF_BACKWARD_PRECISION=exact``."""
    m = points.shape[0]
    dev = points.device
    points = _dev(points, 'points', (m, 4))
    if packed.device != dev:
        raise _l.SunerfHipError('packed weights and points are on different devices')

    def probe():
        # the measured choice of the arithmetic (AUTO) needs rays: PROBE_RAYS of the points as two-sample rays o = 0, d = xyz, z = 1
        # (a rank without points still takes part in the probe's all-reduce, with zero units)
        if m > 0 or _probe_world() > 1:
            k = min(PROBE_RAYS, m)
            idx = torch.linspace(0, max(m - 1, 0), k, device=dev).long()
            sel = points[idx]
            packed.probe(torch.zeros(k, 3, device=dev), sel[:, :3].contiguous(), sel[:, 3].contiguous(), torch.ones(k, 2, device=dev), 0.0)
    image, precision = packed.image_for_call(probe)
    m_pad = (m + 31) // 32 * 32
    if m_pad != m:
        points = torch.cat([points, points.new_zeros(m_pad - m, 4)])
    if training and packed.d_filter not in TRAINABLE_D_FILTER:
        raise NotImplementedError(f'training with d_filter={packed.d_filter} is not implemented (inference only)')
    ws, ws_bytes, stash, fmt = _forward_scratch(packed, dev, m_pad // 32, 32, training)
    raw = torch.empty(m_pad, 2, dtype=torch.float32, device=dev)
    _l.call(dev, 'sunerf_mlp_points_fwd', _ptr(image), packed.d_filter, packed.n_linear, precision, _ptr(points),
            m_pad, _ptr(raw), _ptr(stash), fmt, _ptr(ws), ws_bytes, _stream(dev))
    out = {'raw': raw[:m], 'n_padded': m_pad}
    if training:
        out['stash'] = stash
    return out


def hier_resample(z_vals, weights, u: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``u``: (S_f,) shared sample positions (perturb=False) or (N, S_f) per-ray (perturb=True)."""
    n, sc = z_vals.shape
    z_vals = _dev(z_vals, 'z_vals', (n, sc))
    weights = _dev(weights.detach(), 'weights', (n, sc))
    per_ray = int(u.dim() == 2)
    sf = u.shape[-1]
    order = None
    if per_ray:
        # perturb=True: random positions.  The inverse CDF is monotone, so SORTED positions give sorted new samples and the
        # kernel merges two ascending runs by rank; handed unsorted ones it falls back to one lane's insertion sort per ray
        # (2.6 ms instead of 10 us for 3072 rays x 64 + 128 samples).  The new samples are returned in the caller's order.
        u, order = torch.sort(u, dim=-1)
    u = _dev(u, 'u', (n, sf) if per_ray else (sf,))
    new_z = torch.empty(n, sf, dtype=torch.float32, device=z_vals.device)
    z_comb = torch.empty(n, sc + sf, dtype=torch.float32, device=z_vals.device)
    _l.call(z_vals.device, 'sunerf_hier_resample', _ptr(z_vals), _ptr(weights), _ptr(u), per_ray, n, sc, sf,
            _ptr(new_z), _ptr(z_comb), _stream(z_vals.device))
    if order is not None:
        new_z = torch.empty_like(new_z).scatter_(-1, order, new_z)
    return new_z, z_comb


def sample_pdf(bins, weights, u: torch.Tensor) -> torch.Tensor:
    """HierarchicalSampler.sample_pdf (sampling.py:128-169) on given bins (N, B) and weights (N, B-1) -> samples (N, S_f);
    ``u`` as in :func:`hier_resample`."""
    n, nb = bins.shape
    bins = _dev(bins, 'bins', (n, nb))
    weights = _dev(weights.detach(), 'weights', (n, nb - 1))
    per_ray = int(u.dim() == 2)
    sf = u.shape[-1]
    u = _dev(u, 'u', (n, sf) if per_ray else (sf,))
    samples = torch.empty(n, sf, dtype=torch.float32, device=bins.device)
    _l.call(bins.device, 'sunerf_sample_pdf', _ptr(bins), _ptr(weights), _ptr(u), per_ray, n, nb, sf, _ptr(samples),
            _stream(bins.device))
    return samples


def emission_render_bwd(packed: PackedMLP, rays_o, rays_d, z_vals, raw, stash, g_image, g_reg, g_reg_const: float,
                        reg_radius: float, grad_weights: Sequence[torch.Tensor], grad_biases: Sequence[torch.Tensor],
                        accumulate: bool = False, times=None):
    """Backward of one render pass: fills (or accumulates into) ``grad_weights[i]`` / ``grad_biases[i]`` (nn.Linear
    layouts) from the gradient w.r.t. the 'image' output (N,) or (N,1) and the 'regularization' output
    (``g_reg`` (N,S) tensor or None + the constant ``g_reg_const``).  ``times`` (N,): the forward's time coordinate -- with it
    the small-batch fp32 backward can recompute the activations (``mlp_backward(query=...)``); without it the fp16 kernels run.
    Under ``SUNERF_BACKWARD_PRECISION=exact`` ``times`` is required."""
    if times is None and backward_precision() == 'exact':
        raise _l.SunerfHipError(_NO_QUERY)
    g_raw, absmax = emission_integral_bwd(raw, z_vals, rays_d, g_image, rays_o=rays_o, g_reg=g_reg, g_reg_const=g_reg_const,
                                          reg_radius=reg_radius, return_absmax=True)
    mlp_backward(packed, g_raw, absmax, stash, grad_weights, grad_biases, accumulate,
                 query=None if times is None else ('rays', rays_o, rays_d, times, z_vals))
    return g_raw


def emission_integral_fwd(raw, z_vals, rays_d):
    """EmissionRadiativeTransfer.raw2outputs (emission.py:14-54) on a given raw tensor -> (image (N,1), weights, absorption)."""
    n, s = z_vals.shape
    dev = z_vals.device
    raw = _dev(raw, 'raw', (n, s, 2)); z_vals = _dev(z_vals, 'z_vals', (n, s)); rays_d = _dev(rays_d, 'rays_d', (n, 3))
    f32 = dict(dtype=torch.float32, device=dev)
    image, weights, absorption = torch.empty(n, 1, **f32), torch.empty(n, s, **f32), torch.empty(n, s, **f32)
    _l.call(dev, 'sunerf_emission_integral_fwd', _ptr(raw), _ptr(z_vals), _ptr(rays_d), n, s, _ptr(image), _ptr(weights),
            _ptr(absorption), _stream(dev))
    return image, weights, absorption


def emission_integral_bwd(raw, z_vals, rays_d, g_image=None, g_weights=None, g_absorption=None, *, rays_o=None, g_reg=None,
                          g_reg_const: float = 0.0, reg_radius: float = 0.0, return_absmax: bool = False):
    """d / d raw of :func:`emission_integral_fwd` for gradients w.r.t. any of its three outputs -> g_raw (N,S,2).

    The keyword-only arguments reach the rest of ``sunerf_emission_integral_bwd``: the gradient w.r.t. the 'regularization'
    epilogue relu(|o + d z| - reg_radius) (1 - absorption), as the (N,S) tensor ``g_reg`` or, when that is None, the constant
    ``g_reg_const`` (both need ``rays_o``).  ``return_absmax=True`` returns (g_raw, absmax): the 4-byte word with the bit pattern
    of max |g_raw| (int32, view it as float32) that selects the fp16 gradient scale of the backward kernels after it."""
    n, s = z_vals.shape
    dev = z_vals.device
    raw = _dev(raw, 'raw', (n, s, 2)); z_vals = _dev(z_vals, 'z_vals', (n, s)); rays_d = _dev(rays_d, 'rays_d', (n, 3))
    g_image = torch.zeros(n, dtype=torch.float32, device=dev) if g_image is None else _dev(g_image.reshape(-1), 'g_image', (n,))
    g_weights = None if g_weights is None else _dev(g_weights, 'g_weights', (n, s))
    g_absorption = None if g_absorption is None else _dev(g_absorption, 'g_absorption', (n, s))
    g_reg = None if g_reg is None else _dev(g_reg, 'g_reg', (n, s))
    if rays_o is None:
        if g_reg is not None or g_reg_const != 0.0:
            raise ValueError('a gradient w.r.t. the regularization output needs rays_o')
        rays_o = rays_d           # (rays_o only enters through the regularization term: not read when g_reg = 0)
    else:
        rays_o = _dev(rays_o, 'rays_o', (n, 3))
    g_raw = torch.empty(n, s, 2, dtype=torch.float32, device=dev)
    absmax = torch.empty(1, dtype=torch.int32, device=dev)
    _l.call(dev, 'sunerf_emission_integral_bwd', _ptr(raw), _ptr(z_vals), _ptr(rays_o), _ptr(rays_d), _ptr(g_image), _ptr(g_reg),
            _ptr(g_weights), _ptr(g_absorption), float(g_reg_const), float(reg_radius), n, s, _ptr(g_raw), _ptr(absmax),
            _stream(dev))
    return (g_raw, absmax) if return_absmax else g_raw


# ---- which backward runs (DESIGN.md sections 5.4 and 5.5): the whole policy ------------------------------------------------------
# 'pipe' (default): the layer-pipelined kernel of csrc/bwd_pipe.hip where it applies (d_filter 256, n_linear >= 3, a 256-CU
# device), the two-kernel dgrad + wgrad elsewhere; 'classic' (SUNERF_BACKWARD, or SUNERF_STASH=fp16): always the two kernels.  The
# pipelined launch needs all of its 256 workgroups resident at once: ranks that SHARE one GPU (the CPU-rehearsal tests) must use
# 'classic' (_shared_device), and a launch that gives up switches the process to it (pipe_status).
# Small batches take the reference's arithmetic (csrc/bwd_exact.hip).  The fp16 backward kernels carry ~2^-12 of relative rounding
# error per term of a gradient sum (dZ, cos, H are single fp16 operands).  A training batch averages that away (every tensor within
# 1e-3 of the fp32 oracle from ~1e4 samples on); a batch of a few hundred samples whose bias sums cancel to a few per cent of their
# terms does not (tests/tools/bias_conditioning.py).  Up to EXACT_BACKWARD_SAMPLES samples per call -- where the fp16 kernels are
# launch-latency-bound anyway -- the backward therefore recomputes the activations and runs the chain in fp32.
# SUNERF_EXACT_BACKWARD_SAMPLES overrides the limit (0: never); a backward kernel asked for BY NAME (SUNERF_BACKWARD, tests forcing a
# mode, and the two automatic switches above: they set the same _backward_forced) is always honoured.
# SUNERF_BACKWARD_PRECISION=exact sends EVERY batch that has a query to the any-size fp32 kernel, a forced SUNERF_BACKWARD included.
# The forward decides first (training_stash_format): it leaves the stash for the backward it expects -- phases are read by the
# pipelined kernel only, fp16 sin + cos fragments by the two kernels only, the fp32 kernels read none (_stash_wanted).  The backward
# (_backward_path) goes by the stash it is handed, and refuses a phase stash where the pipelined kernel can no longer run.
_backward_forced = None
EXACT_BACKWARD_SAMPLES = 4096
_NO_QUERY = ('SUNERF_BACKWARD_PRECISION=exact: the fp32 backward recomputes the activations from the query points, and this '
             'backward was given none (pass times= / query=); the fp16 kernels are not run in its place')


def backward_mode() -> str:
    if _backward_forced is not None:
        return _backward_forced
    mode = os.environ.get('SUNERF_BACKWARD', 'pipe').lower()
    if mode not in ('pipe', 'classic'):
        raise ValueError(f"SUNERF_BACKWARD must be 'pipe' or 'classic', not {mode!r}")
    return mode


def exact_backward_limit() -> int:
    v = os.environ.get('SUNERF_EXACT_BACKWARD_SAMPLES', '').strip()
    return EXACT_BACKWARD_SAMPLES if v == '' else max(0, int(v))


def _shared_device(dev) -> bool:
    """Ranks of one process group that drive the SAME GPU cannot all keep a 256-workgroup persistent launch resident: the
    process then uses the two-kernel backward (decided once, collectively, when the optimiser / gradient bucket is built:
    sunerf_hip.dist.ranks_share_a_device; here only the cached answer is read -- no collective inside a backward)."""
    global _backward_forced
    from . import dist as _dist
    if _dist.shared_device_known(dev):
        import warnings
        warnings.warn('several ranks of the process group share one GPU: the layer-pipelined backward needs the whole device, '
                      'this process uses the two-kernel backward (SUNERF_BACKWARD=classic)', RuntimeWarning)
        _backward_forced = 'classic'
        return True
    return False


def training_stash_format(packed, n_rays: int, n_samples: int) -> int:
    """What the training forward leaves for the backward: 16-bit phases (half the bytes; what the layer-pipelined backward reads)
    whenever that backward is going to run -- d_filter 256 on a 256-CU device, SUNERF_BACKWARD not 'classic', no rank sharing the
    card --, fp16 sin + cos fragments for the two-kernel backward otherwise.  ``SUNERF_STASH=fp16`` forces the latter (and with
    it the two-kernel backward)."""
    if os.environ.get('SUNERF_STASH', '').strip().lower() == 'fp16' or n_rays <= 0:
        return STASH_FP16
    if backward_mode() != 'pipe':
        return STASH_FP16
    with torch.cuda.device(packed.device):
        ok = _l.load().sunerf_bwd_pipe_workspace_bytes(n_rays, n_samples, packed.d_filter, packed.n_linear) > 0
    if not ok or _shared_device(packed.device):
        return STASH_FP16
    return STASH_PHASE


def _backward_path(n_rays: int, n_samples: int, has_query: bool, stash_format, pipe_available) -> str:
    """The backward of one :func:`mlp_backward` call on ``n_rays`` x ``n_samples`` samples: 'fp32_chunked', 'fp32', 'pipe' or 'classic';
    'empty' when there is nothing to launch.  Touches no device and reads nothing but ``_backward_forced`` and the SUNERF_*
    environment.  ``stash_format`` and ``pipe_available`` are zero-argument callables -- the format of the stash handed to the
    backward, and whether the workspace query of the pipelined backward is positive for this shape and device -- asked only when
    the rows before them have not decided (an fp32 backward may have been given no stash at all)."""
    total = n_rays * n_samples
    if backward_precision() == 'exact':
        if not has_query:
            raise _l.SunerfHipError(_NO_QUERY)
        return 'fp32_chunked' if total else 'empty'
    by_name = _backward_forced is not None or bool(os.environ.get('SUNERF_BACKWARD', '').strip())
    if has_query and total > 0 and not by_name and total <= exact_backward_limit():
        return 'fp32'
    if n_rays > 0 and stash_format() == STASH_PHASE:
        if backward_mode() != 'pipe':
            raise _l.SunerfHipError('this activation stash holds 16-bit phases (written for the layer-pipelined backward) but the '
                                    'two-kernel backward was selected after the forward ran: choose SUNERF_BACKWARD before the forward, '
                                    'or SUNERF_STASH=fp16')
        if not pipe_available():
            raise _l.SunerfHipError('phase stash but no pipelined backward for this shape / device')
        return 'pipe'
    return 'classic'


def mlp_backward(packed: PackedMLP, g_raw, absmax, stash, grad_weights: Sequence[torch.Tensor],
                 grad_biases: Sequence[torch.Tensor], accumulate: bool = False, query=None):
    """dgrad + wgrad of the sine MLP from the gradient w.r.t. its raw output (N,S,2): fills / accumulates the nn.Linear
    gradients.  ``absmax``: 4-byte device scalar with the bit pattern of max |g_raw| (written by the integral backward).
    ``query``: what the forward was evaluated on -- ``('rays', rays_o, rays_d, times, z_vals)`` or ``('points', points (N*S, 4))``;
    given it, batches of at most ``exact_backward_limit()`` samples take the fp32 backward (csrc/bwd_exact.hip), and under
    ``SUNERF_BACKWARD_PRECISION=exact`` every batch does (the any-size kernel; no stash is read, ``stash`` may be None)."""
    n, s = g_raw.shape[0], g_raw.shape[1]
    dev = g_raw.device
    kernel_w, kernel_b, kernel_accumulate, fold = packed.stage_grads(grad_weights, grad_biases, accumulate)

    @functools.cache
    def pipe_bytes():       # one workspace query per call: the decision asks whether it is positive, the pipelined launcher for the size
        with torch.cuda.device(dev):
            return _l.load().sunerf_bwd_pipe_workspace_bytes(n, s, packed.d_filter, packed.n_linear)
    path = _backward_path(n, s, query is not None, lambda: stash_format_of(stash, n, s, packed), lambda: pipe_bytes() > 0)
    if path == 'empty':
        if not kernel_accumulate:
            for t in (*kernel_w, *kernel_b):
                t.zero_()
    elif path in ('fp32', 'fp32_chunked'):
        _mlp_backward_exact(packed, g_raw, query, kernel_w, kernel_b, kernel_accumulate, chunked=path == 'fp32_chunked')
    elif path == 'pipe':
        _mlp_backward_pipe(packed, g_raw, absmax, stash, pipe_bytes(), kernel_w, kernel_b, kernel_accumulate)
    else:
        _mlp_backward_classic(packed, g_raw, absmax, stash, kernel_w, kernel_b, kernel_accumulate)
    fold()


# ---- the two-kernel backward (csrc/render_bwd.hip, csrc/wgrad.hip) ---------------------------------------------------------------
def wgrad_split(n_linear: int, n_cus: int = 256, d_filter: int = 256) -> int:
    """Partial sums per layer in sunerf_mlp_wgrad: n_linear * split (* 4 workgroup blocks at d_filter = 512) workgroups
    must fit the chip in ONE wave (one workgroup per CU, all about equally long): 9 layers -> 28 (252 workgroups);
    288 would take two rounds."""
    blocks = 4 if d_filter > 256 else 1
    return max(1, n_cus // (n_linear * blocks))


def _mlp_backward_classic(packed: PackedMLP, g_raw, absmax, stash, grad_weights, grad_biases, accumulate: bool):
    lib = _l.load()
    n, s = g_raw.shape[0], g_raw.shape[1]
    dev = g_raw.device
    D, nl = packed.d_filter, packed.n_linear
    stream = _stream(dev)
    dz = torch.empty(lib.sunerf_dz_stash_bytes(n, s, D, nl), dtype=torch.uint8, device=dev)
    _l.call(dev, 'sunerf_mlp_dgrad', _ptr(packed.transposed()), D, nl, _ptr(g_raw), _ptr(absmax), _ptr(stash),
            _ptr(dz), n, s, stream)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    cap = int(os.environ.get('SUNERF_GRID_CAP_WGRAD', 0))        # experiment knob, see csrc/sunerf_common.h
    split = wgrad_split(nl, cap if 0 < cap < cus else cus, D)
    ws = torch.empty(lib.sunerf_wgrad_workspace_bytes(D, nl, split), dtype=torch.uint8, device=dev)
    _l.call(dev, 'sunerf_mlp_wgrad', D, nl, packed.d_out, _ptr(packed.transposed()), _ptr(stash), _ptr(dz), _ptr(g_raw), _ptr(absmax), n, s,
            _ptr(ws), split, _ptr_array(grad_weights), _ptr_array(grad_biases), int(accumulate), stream)


# ---- the pipelined backward (csrc/bwd_pipe.hip) --------------------------------------------------------------------------------
pipe_timing = False                       # True: every pipelined launch is bracketed by library-owned HIP events (flags bit 7)
_pipe_ws = {}                             # (device, stream) -> workspace
_pipe_checked = {}                        # workspaces whose sticky status word has not been looked at yet
PIPE_WS_STICKY, PIPE_WS_DEBUG = 0, 256    # include/sunerf_hip.h: fixed offsets of the sticky status block / the debug counters


def _env_on(name: str) -> bool:
    return os.environ.get(name, '0').lower() not in ('', '0', 'false', 'no', 'off')


def pipe_w_mode() -> str:
    """Precision of W^T in the pipelined backward's data gradient: 'auto' (default: a single fp16 W^T while a measured probe
    allows it, fp16 head + remainder otherwise -- see _pipe_w_probe), 'hi' (SUNERF_PIPE_HI_ONLY=1), 'hilo' (=0)."""
    v = os.environ.get('SUNERF_PIPE_HI_ONLY', 'auto').strip().lower()
    if v in ('', 'auto'):
        return 'auto'
    return 'hilo' if v in ('0', 'false', 'no', 'off') else 'hi'


def _pipe_flags() -> int:
    return (1 if pipe_w_mode() == 'hi' else 0) | (2 if _env_on('SUNERF_PIPE_DEBUG') else 0) | (0x80 if pipe_timing else 0)


def pipe_kernel_time():
    """(sum of the kernel durations in ms, number of launches) of the pipelined-backward launches issued while
    ``ops.pipe_timing`` was set, measured by HIP events inside the C ABI on the launch stream; waits for them and forgets them."""
    ms, n = ctypes.c_double(0.0), ctypes.c_int(0)
    _l.check(_l.load().sunerf_bwd_pipe_kernel_time(ctypes.byref(ms), ctypes.byref(n)), 'sunerf_bwd_pipe_kernel_time')
    return ms.value, n.value


def pipe_debug(dev=None):
    """SUNERF_PIPE_DEBUG=1: per-workgroup counters of the last pipelined launch, (8, 256, 8) int32: [0] loop ticks (100 MHz),
    fallback spins and their ticks on the input link, the same on the output link, chunks, layer, pipeline; [1] shader clocks / 16 of
    data wave 1 per phase of its loop (wait, barrier, k-steps, epilogue + decoder; of the latter: products + conversion, .. + stores); [2], [3] the same of weight waves 4 and 5 (top, operand
    reads + gate, matrix phase, counted wait, barrier); [4], [5] viewed as int64 (32, 8, 8): the stamps of iteration n / 2 of every
    wave of the workgroups of pipeline 0 (tools/pipe_check.py prints them as a timeline)."""
    for (d, _), ws in _pipe_ws.items():
        if dev is None or d == dev:
            return ws[PIPE_WS_DEBUG:PIPE_WS_DEBUG + 256 * 64 * 4].view(torch.int32).reshape(8, 256, 8).cpu()
    return None


def _pipe_workspace(dev, nbytes: int) -> torch.Tensor:
    key = (dev, torch.cuda.current_stream(dev).cuda_stream)
    ws = _pipe_ws.get(key)
    if ws is None or ws.numel() < nbytes:
        if ws is not None and key in _pipe_checked:
            pipe_status()          # the outgoing workspace's sticky word is looked at before it is dropped
        ws = _pipe_ws[key] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        ws[PIPE_WS_STICKY:PIPE_WS_DEBUG].zero_()      # the sticky status block is the caller's: zeroed once, read + cleared by pipe_status
    _pipe_checked[key] = ws
    return ws


def pipe_status(raise_on_failure: Optional[bool] = None) -> int:
    """Worst status of ALL pipelined backward launches since the last call (one 4-byte read per workspace; call it where the
    step synchronises anyway).  The word is sticky: every launch's reduce kernel raises it to its own status, nothing but this
    function clears it -- a give-up of the fine model's launch is still there after the coarse model's launch on the same
    workspace.  Non-zero: a launch gave up (csrc/bwd_pipe.hip) -- its gradients were NaN, so the optimiser skipped that step.
    The process then switches to the two-kernel backward and says so: with a warning by default, with an exception when
    ``SUNERF_BACKWARD=pipe`` was asked for explicitly (or ``raise_on_failure=True``)."""
    global _backward_forced
    worst = 0
    for key, ws in list(_pipe_checked.items()):
        word = ws[PIPE_WS_STICKY:PIPE_WS_STICKY + 4].view(torch.int32)
        status = int(word.item())
        if status:
            word.zero_()
        worst = max(worst, status)
        del _pipe_checked[key]
    if worst:
        _backward_forced = 'classic'
        msg = (f'the pipelined backward gave up (status {worst}: 1 = workgroups not co-resident, 2 = a workgroup class was not '
               'placed on one XCD, 3 = a hand-off timed out); the step was skipped (NaN gradients) and this process now uses the '
               'two-kernel backward (SUNERF_BACKWARD=classic selects it from the start)')
        if raise_on_failure is None:
            raise_on_failure = os.environ.get('SUNERF_BACKWARD', '').lower() == 'pipe'
        if raise_on_failure:
            raise _l.SunerfHipError(msg)
        import warnings
        warnings.warn(msg, RuntimeWarning)
    return worst


# ---- single or split W^T in the pipelined backward: chosen by measurement, like the forward arithmetic -----------------------
# The data-gradient waves multiply dZ by W^T as fp16 head + fp16 remainder (32 matrix instructions per chunk) or by the head
# alone (16: the kernel -5.7 %, the training step -3.3 %, tools/experiments/r4_pipe_ab.sh).  The head alone is a SYSTEMATIC
# perturbation of the weights (2^-12 per element, the same for every sample), so its effect on the weight gradients does not
# average over the batch -- and for the same reason it can be measured on a few rays: the relative difference between the two
# arithmetics on the first 64 rays of a batch predicts the difference on 8192 rays within 2 %
# (tools/experiments/r4_hi_only_accuracy.py, profiles/r4_ab/r4_hi_only_accuracy.log: probe 5.2e-4 at default initialisation, 5.0e-4 with
# hidden weights x 2, 7.5e-4 at x 3, 8.5e-4 at x 4; against fp32 gradients: head + remainder 2.3 ... 2.8e-4 / 4.0e-4 / 6.6e-4, head
# alone 5.3 ... 6.0e-4 / 9.2e-4 / 8.4e-4).  Every PROBE_EVERY-th parameter version (and at the first pipelined backward of a model)
# both arithmetics run on those rays; the head alone is used while the worst weight tensor differs by at most PIPE_W_LIMIT, which
# keeps the gradients within ~0.6 of SURVEY 8d's 1e-3.  No collective: under data parallelism every rank decides for itself (the
# all-reduced gradient, and with it every replica, is the same on all ranks whichever arithmetic produced a rank's share).
PIPE_W_PROBE_RAYS = 64
PIPE_W_LIMIT = 6e-4


def _pipe_w_probe(packed, call_prefix):
    """Runs the pipelined backward on the first PIPE_W_PROBE_RAYS rays in both arithmetics into scratch gradients and leaves the
    worst relative difference of a weight tensor in a pinned host word behind an event (read at once for the first probe)."""
    dev = packed.device
    if packed._pipe_probe_bufs is None:
        packed._pipe_probe_bufs = [packed.kernel_shaped(), packed.kernel_shaped()]
    for hi_only, (gW, gb) in zip((0, 1), packed._pipe_probe_bufs):
        call_prefix(gW, gb, hi_only)
    (a, _), (b, _) = packed._pipe_probe_bufs
    diff = torch._foreach_norm(torch._foreach_sub(b, a))
    base = torch._foreach_norm(a)
    units = torch.nan_to_num((torch.stack(diff) / torch.stack(base)).max().reshape(1), nan=float('inf'))
    first = packed.pipe_w_probe is None
    packed._pipe_w_pending = _DeferredWord(units, dev)
    packed._pipe_probe_version = packed._version
    _pipe_w_apply(packed, block=first or not PROBE_ASYNC)


def _pipe_w_apply(packed, block: bool = False):
    word = packed._pipe_w_pending
    if word is None or not word.ready(wait=block):
        return
    packed._pipe_w_pending = None
    packed.pipe_w_probe = float(word.host[0])
    packed.pipe_hi_only = packed.pipe_w_probe <= PIPE_W_LIMIT


def _mlp_backward_pipe(packed: PackedMLP, g_raw, absmax, stash, pipe_bytes: int, grad_weights, grad_biases, accumulate: bool):
    n, s = g_raw.shape[0], g_raw.shape[1]
    dev = g_raw.device
    ws = _pipe_workspace(dev, pipe_bytes)
    flags = _pipe_flags()

    def launch(n_rays, gw, gb, acc, fl):
        _l.call(dev, 'sunerf_mlp_backward_pipe', packed.d_filter, packed.n_linear, packed.d_out, _ptr(packed.transposed()), _ptr(stash),
                _ptr(g_raw), _ptr(absmax), n_rays, s, _ptr(ws), pipe_bytes, _ptr_array(gw), _ptr_array(gb), int(acc), fl, _stream(dev))
    if pipe_w_mode() == 'auto':
        with packed._lock:
            due = packed._pipe_probe_version is None or packed._version - packed._pipe_probe_version >= PROBE_EVERY
            if due and n >= PIPE_W_PROBE_RAYS and packed._pipe_w_pending is None:
                # on the first rays: a prefix of g_raw and of the (ray-major) stash
                _pipe_w_probe(packed, lambda gw, gb, hi_only: launch(PIPE_W_PROBE_RAYS, gw, gb, 0, (flags & ~0x81) | hi_only))
            _pipe_w_apply(packed)
            if packed.pipe_hi_only:
                flags |= 1
    launch(n, grad_weights, grad_biases, accumulate, flags)


# ---- the fp32 backward (csrc/bwd_exact.hip) ------------------------------------------------------------------------------------
_exact_ws = {}          # (device, stream) -> workspace of the fp32 backward (either kernel)


def _mlp_backward_exact(packed: PackedMLP, g_raw, query, grad_weights, grad_biases, accumulate: bool, chunked: bool = False):
    """``chunked``: the any-size kernel (sunerf_mlp_backward_exact_chunked, workspace independent of the batch), else the
    small-batch one."""
    lib = _l.load()
    dev = g_raw.device
    n, s = g_raw.shape[0], g_raw.shape[1]
    weights, biases = packed.kernel_params()
    nl = packed.n_linear
    if chunked:
        nbytes = lib.sunerf_mlp_backward_exact_chunked_workspace_bytes(packed.d_filter, nl)
    else:
        nbytes = lib.sunerf_mlp_backward_exact_workspace_bytes(n * s, packed.d_filter, nl)
    ws = _workspace(_exact_ws, dev, nbytes)
    if query[0] == 'rays':
        _, o, d, t, z = query
        o, d = _dev(o, 'rays_o', (n, 3)), _dev(d, 'rays_d', (n, 3))
        t, z = _dev(t.reshape(-1), 'times', (n,)), _dev(z, 'z_vals', (n, s))
        args = (_ptr(o), _ptr(d), _ptr(t), _ptr(z), None)
    else:
        pts = _dev(query[1], 'points', (n * s, 4))
        args = (None, None, None, None, _ptr(pts))
    g = g_raw if g_raw.shape[-1] == packed.d_out else g_raw[..., :packed.d_out]       # (N, S, d_out), densely packed
    g = _dev(g, 'g_raw')
    _l.call(dev, 'sunerf_mlp_backward_exact_chunked' if chunked else 'sunerf_mlp_backward_exact', _ptr_array(weights), _ptr_array(biases),
            nl, packed.d_filter, packed.d_out, *args, n, s, _ptr(g), _ptr(ws), nbytes, _ptr_array(grad_weights), _ptr_array(grad_biases),
            int(accumulate), _stream(dev))


def mlp_input_backward(packed: PackedMLP, g_raw, query, grad_weights=None, grad_biases=None, accumulate: bool = False,
                       wanted=(True, True, True, True)):
    """Gradients w.r.t. the query of the MLP from the gradient w.r.t. its raw output (csrc/bwd_exact.hip:
    sunerf_mlp_input_grad_exact, fp32 throughout).  ``query``: ``('points', points (M, 4))`` with ``g_raw`` (M, >= d_out) -> the
    (M, 4) point gradient; or ``('rays', rays_o, rays_d, times, z_vals)`` with ``g_raw`` (N, S, >= d_out) -> ``(g_rays_o (N, 3),
    g_rays_d (N, 3), g_times (N,), g_z_vals (N, S))``, an entry None where ``wanted`` says so.  Given ``grad_weights`` /
    ``grad_biases`` (model shapes), the parameter gradients are filled / added to (``accumulate``) in the same call, bit-identical
    to :func:`_mlp_backward_exact` ``(chunked=True)``'s."""
    lib = _l.load()
    dev = g_raw.device
    nl = packed.n_linear
    f32 = dict(dtype=torch.float32, device=dev)
    if query[0] == 'rays':
        _, o, d, t, z = query
        n, s = z.shape
        o, d = _dev(o, 'rays_o', (n, 3)), _dev(d, 'rays_d', (n, 3))
        t, z = _dev(t.reshape(-1), 'times', (n,)), _dev(z, 'z_vals', (n, s))
        g = g_raw.reshape(n, s, -1)[..., :packed.d_out]
        outs = [torch.empty(shape, **f32) if w else None for w, shape in zip(wanted, ((n, 3), (n, 3), (n,), (n, s)))]
        if not any(w is not None for w in outs):
            raise ValueError('mlp_input_backward: no ray gradient wanted')
        args = (_ptr(o), _ptr(d), _ptr(t), _ptr(z), None)
        out_ptrs = (None,) + tuple(_ptr(x) for x in outs)
        result = tuple(outs)
    else:
        n, s = query[1].shape[0], 1
        pts = _dev(query[1], 'points', (n, 4))
        g = g_raw.reshape(n, -1)[:, :packed.d_out]
        result = torch.empty(n, 4, **f32)
        outs = [result]
        args = (None, None, None, None, _ptr(pts))
        out_ptrs = (_ptr(result), None, None, None, None)
    g = _dev(g, 'g_raw')
    params = grad_weights is not None
    GW = GB = None
    kernel_accumulate, fold = accumulate, None
    if params:
        kernel_w, kernel_b, kernel_accumulate, fold = packed.stage_grads(grad_weights, grad_biases, accumulate)
        GW, GB = _ptr_array(kernel_w), _ptr_array(kernel_b)
    if n * s == 0:
        zero = [x for x in outs if x is not None]
        if params and not accumulate:
            zero += [*grad_weights, *grad_biases]
        for t in zero:
            t.zero_()
        return result
    weights, biases = packed.kernel_params()
    nbytes = lib.sunerf_mlp_input_grad_exact_workspace_bytes(packed.d_filter, nl)
    ws = _workspace(_exact_ws, dev, nbytes)
    _l.call(dev, 'sunerf_mlp_input_grad_exact', _ptr_array(weights), _ptr_array(biases), nl, packed.d_filter, packed.d_out, *args, n, s,
            _ptr(g), _ptr(ws), nbytes, GW, GB, int(kernel_accumulate), *out_ptrs, _stream(dev))
    if params:
        fold()
    return result


AIA_WAVELENGTHS = (94, 131, 171, 193, 211, 304, 335)


def _dt_fwd(entry, table, m, raw, z_vals, rays_o, rays_d, wavelengths, log_abs, vol_c, base_log_density, base_log_temperature,
            pixel_intensity_factor, reg_radius, want_epilogues):
    """Forward of the DT integral through ``entry``.  ``table(dev)``: the entry point's table arguments, checked (the AIA pair, or
    those of a response set); ``m``: the channels of ``log_abs``."""
    n, s = z_vals.shape
    dev = z_vals.device
    w = wavelengths.shape[1]
    raw = _dev(raw, 'raw', (n, s, 2)); z_vals = _dev(z_vals, 'z_vals', (n, s))
    rays_o = _dev(rays_o, 'rays_o', (n, 3)); rays_d = _dev(rays_d, 'rays_d', (n, 3))
    wavelengths = _dev(wavelengths.to(torch.float32), 'wavelengths', (n, w))
    table = table(dev)
    log_abs = _dev(log_abs.detach(), 'log_abs', (m,)); vol_c = _dev(vol_c.detach().reshape(1), 'vol_c', (1,))
    f32 = dict(dtype=torch.float32, device=dev)
    out = {'image': torch.empty(n, w, **f32), 'weights': torch.empty(n, s, **f32), 'reg_q': torch.empty(n, s, **f32)}
    hm = am = reg = None
    if want_epilogues:
        hm, am, reg = torch.empty(n, **f32), torch.empty(n, **f32), torch.empty(n, s, **f32)
    _l.call(dev, entry, _ptr(raw), _ptr(z_vals), _ptr(rays_o), _ptr(rays_d), _ptr(wavelengths), w, *table, _ptr(log_abs),
            _ptr(vol_c), float(base_log_density), float(base_log_temperature), float(pixel_intensity_factor), float(reg_radius),
            n, s, _ptr(out['image']), _ptr(out['weights']), _ptr(out['reg_q']), _ptr(hm), _ptr(am), _ptr(reg), _stream(dev))
    if want_epilogues:
        out.update(height_map=hm, absorption_map=am, regularization=reg)
    return out


def _dt_bwd(entry, table, m, raw, z_vals, rays_o, rays_d, wavelengths, log_abs, vol_c, base_log_density, base_log_temperature,
            pixel_intensity_factor, reg_radius, g_image, per_sample, fits=None):
    """Launches DT integral backward ``entry`` with the (N,S) output gradients ``per_sample`` ((name, tensor or None) pairs,
    in the entry point's order) -> (g_raw, g_log_abs (m,), g_vol_c, absmax).  ``table(dev)`` / ``m``: as :func:`_dt_fwd`;
    ``fits(n, s, w)``: raises for a shape the entry point would refuse."""
    n, s = z_vals.shape
    dev = z_vals.device
    w = wavelengths.shape[1]
    raw = _dev(raw, 'raw', (n, s, 2)); z_vals = _dev(z_vals, 'z_vals', (n, s))
    rays_o = _dev(rays_o, 'rays_o', (n, 3)); rays_d = _dev(rays_d, 'rays_d', (n, 3))
    wavelengths = _dev(wavelengths.to(torch.float32), 'wavelengths', (n, w))
    log_abs = _dev(log_abs.detach(), 'log_abs', (m,)); vol_c = _dev(vol_c.detach().reshape(1), 'vol_c', (1,))
    g_image = _dev(g_image, 'g_image', (n, w))
    per_sample = [None if g is None else _dev(g, name, (n, s)) for name, g in per_sample]
    if fits is not None:
        fits(n, s, w)
    f32 = dict(dtype=torch.float32, device=dev)
    g_raw = torch.empty(n, s, 2, **f32)
    small = torch.empty(m + 2, **f32)
    g_la, g_vc, absmax = small[:m], small[m:m + 1], small[m + 1:m + 2].view(torch.int32)
    _l.call(dev, entry, _ptr(raw), _ptr(z_vals), _ptr(rays_o), _ptr(rays_d), _ptr(wavelengths), w, *table(dev), _ptr(log_abs),
            _ptr(vol_c), float(base_log_density), float(base_log_temperature), float(pixel_intensity_factor), float(reg_radius),
            n, s, _ptr(g_image), *[_ptr(g) for g in per_sample], _ptr(g_raw), _ptr(g_la), _ptr(g_vc), _ptr(absmax), _stream(dev))
    return g_raw, g_la, g_vc, absmax


def dt_integral_fwd(raw, z_vals, rays_o, rays_d, wavelengths, table_logt, table_resp, log_abs, vol_c, base_log_density,
                    base_log_temperature, pixel_intensity_factor, reg_radius, want_epilogues=False):
    """DT radiative-transfer integral on the raw MLP output (density_temperature.py:192-274)."""
    def table(dev):
        return _ptr(_dev(table_logt, 'table_logt', (7, 101))), _ptr(_dev(table_resp, 'table_resp', (7, 101)))
    return _dt_fwd('sunerf_dt_integral_fwd', table, 7, raw, z_vals, rays_o, rays_d, wavelengths, log_abs, vol_c, base_log_density,
                   base_log_temperature, pixel_intensity_factor, reg_radius, want_epilogues)


def simple_star_field(rays_o, rays_d, z_vals, rho_0: float, h0: float, T0: float, Rs: float, t_photosphere: float):
    """SimpleStar.forward (stellar_model.py:53-102) at the sample points of every ray -> raw (N, S, 2) = (ln rho, log10 T)."""
    n, s = z_vals.shape
    rays_o = _dev(rays_o, 'rays_o', (n, 3)); rays_d = _dev(rays_d, 'rays_d', (n, 3)); z_vals = _dev(z_vals, 'z_vals', (n, s))
    raw = torch.empty(n, s, 2, dtype=torch.float32, device=z_vals.device)
    _l.call(z_vals.device, 'sunerf_simple_star_field', _ptr(rays_o), _ptr(rays_d), _ptr(z_vals), n, s, float(rho_0),
            float(h0), float(T0), float(Rs), float(t_photosphere), _ptr(raw), _stream(z_vals.device))
    return raw


def _dt_integral_bwd(entry, raw, z_vals, rays_o, rays_d, wavelengths, table_logt, table_resp, log_abs, vol_c,
                     base_log_density, base_log_temperature, pixel_intensity_factor, reg_radius, g_image, per_sample):
    """Launches DT integral backward ``entry`` with the (N,S) output gradients ``per_sample`` ((name, tensor or None) pairs,
    in the entry point's order) -> (g_raw, g_log_abs, g_vol_c, absmax)."""
    return _dt_bwd(entry, lambda dev: (_ptr(table_logt), _ptr(table_resp)), 7, raw, z_vals, rays_o, rays_d, wavelengths, log_abs,
                   vol_c, base_log_density, base_log_temperature, pixel_intensity_factor, reg_radius, g_image, per_sample)


def dt_integral_bwd(raw, z_vals, rays_o, rays_d, wavelengths, table_logt, table_resp, log_abs, vol_c, base_log_density,
                    base_log_temperature, pixel_intensity_factor, reg_radius, g_image, g_reg):
    """-> (g_raw (N,S,2), g_log_abs (7,), g_vol_c (1,), absmax).  The two scalar-head gradients are adjacent views of one buffer
    (``g_log_abs.storage`` holds [7 channels, vol_c, absmax]): one clear in the entry point, one add into a flat gradient bucket."""
    return _dt_integral_bwd('sunerf_dt_integral_bwd', raw, z_vals, rays_o, rays_d, wavelengths, table_logt, table_resp, log_abs,
                            vol_c, base_log_density, base_log_temperature, pixel_intensity_factor, reg_radius, g_image,
                            [('g_reg', g_reg)])


def dt_integral_bwd_full(raw, z_vals, rays_o, rays_d, wavelengths, table_logt, table_resp, log_abs, vol_c, base_log_density,
                         base_log_temperature, pixel_intensity_factor, reg_radius, g_image, g_reg, g_weights, g_reg_q):
    """:func:`dt_integral_bwd` for gradients w.r.t. all three outputs of raw2outputs (density_temperature.py:267-271): also
    ``g_weights`` / ``g_reg_q`` (N,S) (either may be None) -> (g_raw (N,S,2), g_log_abs (7,), g_vol_c (1,), absmax), the two
    scalar-head gradients adjacent in one buffer as there."""
    return _dt_integral_bwd('sunerf_dt_integral_bwd_full', raw, z_vals, rays_o, rays_d, wavelengths, table_logt, table_resp,
                            log_abs, vol_c, base_log_density, base_log_temperature, pixel_intensity_factor, reg_radius, g_image,
                            [('g_reg', g_reg), ('g_weights', g_weights), ('g_reg_q', g_reg_q)])


# ---- the same integral against a response set (include/sunerf_hip_response.h, sunerf_hip/response.py) ------------------------
def _response_set_args(response_set, dev):
    """The C ABI's ``n_channels, n_nodes_total, offsets, codes, logt, resp`` of a ``ResponseSet`` on ``dev``."""
    offsets, codes, logt, resp = response_set.to(dev)
    return (response_set.n_channels, response_set.n_nodes, _ptr(offsets), _ptr(codes), _ptr(logt), _ptr(resp))


def dt_response_bwd_lds_bytes(n_samples: int, n_wavelengths: int, n_nodes_total: int) -> int:
    """LDS bytes the response-set backward needs: a shape above 160 KiB is refused (``response_set.fits`` says which fit)."""
    return int(_l.load().sunerf_dt_response_bwd_lds_bytes(int(n_samples), int(n_wavelengths), int(n_nodes_total)))


def dt_response_fwd(raw, z_vals, rays_o, rays_d, wavelengths, response_set, log_abs, vol_c, base_log_density,
                    base_log_temperature, pixel_intensity_factor, reg_radius, want_epilogues=False):
    """:func:`dt_integral_fwd` against ``response_set`` (a ``sunerf_hip.response.ResponseSet``): ``wavelengths`` (N, W <= 8) holds
    the set's channel codes, ``log_abs`` is (M,) in set order."""
    return _dt_fwd('sunerf_dt_response_fwd', lambda dev: _response_set_args(response_set, dev), response_set.n_channels, raw, z_vals,
                   rays_o, rays_d, wavelengths, log_abs, vol_c, base_log_density, base_log_temperature, pixel_intensity_factor,
                   reg_radius, want_epilogues)


def _dt_response_bwd(entry, raw, z_vals, rays_o, rays_d, wavelengths, response_set, log_abs, vol_c, base_log_density,
                     base_log_temperature, pixel_intensity_factor, reg_radius, g_image, per_sample):
    """:func:`_dt_integral_bwd` for the response-set entry points -> (g_raw, g_log_abs (M,), g_vol_c, absmax)."""
    def fits(n, s, w):
        if n > 0 and dt_response_bwd_lds_bytes(s, w, response_set.n_nodes) > 160 * 1024:
            raise ValueError(f'{entry}: {s} samples x {w} columns with {response_set.n_nodes} response nodes need more than the 160 KiB '
                             f'of LDS of a compute unit (at most {response_set.max_samples(w)} samples at this width)')
    return _dt_bwd(entry, lambda dev: _response_set_args(response_set, dev), response_set.n_channels, raw, z_vals, rays_o, rays_d,
                   wavelengths, log_abs, vol_c, base_log_density, base_log_temperature, pixel_intensity_factor, reg_radius, g_image,
                   per_sample, fits)


def dt_response_bwd(raw, z_vals, rays_o, rays_d, wavelengths, response_set, log_abs, vol_c, base_log_density,
                    base_log_temperature, pixel_intensity_factor, reg_radius, g_image, g_reg):
    """:func:`dt_integral_bwd` against ``response_set`` -> (g_raw (N,S,2), g_log_abs (M,), g_vol_c (1,), absmax), the scalar
    gradients adjacent views of one buffer as there."""
    return _dt_response_bwd('sunerf_dt_response_bwd', raw, z_vals, rays_o, rays_d, wavelengths, response_set, log_abs, vol_c,
                            base_log_density, base_log_temperature, pixel_intensity_factor, reg_radius, g_image,
                            [('g_reg', g_reg)])


def dt_response_bwd_full(raw, z_vals, rays_o, rays_d, wavelengths, response_set, log_abs, vol_c, base_log_density,
                         base_log_temperature, pixel_intensity_factor, reg_radius, g_image, g_reg, g_weights, g_reg_q):
    """:func:`dt_integral_bwd_full` against ``response_set``."""
    return _dt_response_bwd('sunerf_dt_response_bwd_full', raw, z_vals, rays_o, rays_d, wavelengths, response_set, log_abs,
                            vol_c, base_log_density, base_log_temperature, pixel_intensity_factor, reg_radius, g_image,
                            [('g_reg', g_reg), ('g_weights', g_weights), ('g_reg_q', g_reg_q)])


def simple_star_field_dev(rays_o, rays_d, z_vals, params, t_photosphere: float):
    """:func:`simple_star_field` with the stellar parameters read on the device: ``params`` (4,) fp32 = (Rs, h0, T0, rho_0),
    the order of ``SimpleStar.stellar_parameters`` -> raw (N, S, 2) = (ln rho, log10 T), bit-identical to the host-float form."""
    n, s = z_vals.shape
    dev = z_vals.device
    rays_o = _dev(rays_o, 'rays_o', (n, 3)); rays_d = _dev(rays_d, 'rays_d', (n, 3)); z_vals = _dev(z_vals, 'z_vals', (n, s))
    params = _dev(params.detach(), 'params', (4,))
    raw = torch.empty(n, s, 2, dtype=torch.float32, device=dev)
    _l.call(dev, 'sunerf_simple_star_field_dev', _ptr(rays_o), _ptr(rays_d), _ptr(z_vals), n, s, _ptr(params),
            float(t_photosphere), _ptr(raw), _stream(dev))
    return raw


def simple_star_bwd(rays_o, rays_d, z_vals, params, t_photosphere: float, g_raw, out: Optional[torch.Tensor] = None):
    """d loss / d (Rs, h0, T0, rho_0) of :func:`simple_star_field_dev` given ``g_raw`` (N, S, 2) -> (4,) fp32.  ``out``: a (4,)
    contiguous fp32 tensor (e.g. the parameters' slice of a flat gradient buffer) the result is ADDED to; returned."""
    n, s = z_vals.shape
    dev = z_vals.device
    rays_o = _dev(rays_o, 'rays_o', (n, 3)); rays_d = _dev(rays_d, 'rays_d', (n, 3)); z_vals = _dev(z_vals, 'z_vals', (n, s))
    params = _dev(params.detach(), 'params', (4,))
    g_raw = _dev(g_raw, 'g_raw', (n, s, 2))
    accumulate = out is not None
    if out is None:
        out = torch.empty(4, dtype=torch.float32, device=dev)
    elif not out.is_contiguous() or out.shape != (4,) or out.dtype != torch.float32 or out.device != dev:
        raise ValueError('out must be a contiguous (4,) float32 tensor on the device of the rays')
    ws = torch.empty(_l.load().sunerf_simple_star_bwd_workspace_bytes(), dtype=torch.uint8, device=dev)
    _l.call(dev, 'sunerf_simple_star_bwd', _ptr(rays_o), _ptr(rays_d), _ptr(z_vals), n, s, _ptr(params), float(t_photosphere),
            _ptr(g_raw), _ptr(ws), ws.numel(), _ptr(out), 1 if accumulate else 0, _stream(dev))
    return out


# ---- MHD simulation cube (csrc/mhd.hip) -----------------------------------------------------------------------------------
class MhdFrame(ctypes.Structure):
    """``SunerfMhdFrame`` of include/sunerf_hip.h: where one resident frame's nodes, axes and bucket tables live."""
    _fields_ = [('data', ctypes.c_void_p), ('axis', ctypes.c_void_p * 3), ('bucket', ctypes.c_void_p * 3),
                ('n', ctypes.c_int * 3), ('nb', ctypes.c_int * 3), ('lo', ctypes.c_float * 3), ('hi', ctypes.c_float * 3),
                ('inv_width', ctypes.c_float * 3), ('reserved', ctypes.c_int)]


MHD_MAX_BUCKETS = 1 << 16


def mhd_bucket_table(axis: torch.Tensor) -> Tuple[torch.Tensor, float]:
    """Uniform bucket table of one strictly increasing fp32 axis for the kernel's cell search: ``(table int32 [nb], nb /
    (hi - lo))``, ``table[b]`` = the cell ``searchsorted(axis, edge_b, 'right') - 1`` (clipped to [0, n - 2]) holding the lower
    edge of bucket b.  ``nb`` = span / smallest spacing (at most ``MHD_MAX_BUCKETS``): a handful of nodes per bucket even on
    PSI's clustered r grid, so the kernel's walk from ``table[b]`` to the point's cell stays short."""
    g = axis.detach().cpu().double()
    n = g.numel()
    span = float(g[-1] - g[0])
    nb = int(min(MHD_MAX_BUCKETS, max(1, -(-span // float((g[1:] - g[:-1]).min())))))
    edges = g[0] + torch.arange(nb, dtype=torch.float64) * (span / nb)
    table = (torch.searchsorted(g, edges, right=True) - 1).clamp_(0, n - 2).to(torch.int32)
    return table, float(torch.tensor(nb / span, dtype=torch.float32))


def mhd_frame(data: torch.Tensor, axes: Sequence[torch.Tensor]) -> Tuple[MhdFrame, Tuple[torch.Tensor, ...]]:
    """Descriptor of one resident frame: ``data`` (n_phi, n_theta, n_r, 2) fp32 (rho, T) and its three fp32 axes
    (phi, theta, r), all on the device.  Returns the descriptor and the tensors it points into (the bucket tables are made
    here and must be kept alive with the data)."""
    dev = data.device
    if data.dtype != torch.float32 or not data.is_contiguous() or data.dim() != 4 or data.shape[3] != 2:
        raise ValueError('data must be a contiguous (n_phi, n_theta, n_r, 2) float32 tensor')
    desc = MhdFrame()
    keep = [data]
    desc.data = data.data_ptr()
    for k, ax in enumerate(axes):
        ax = _dev(ax, 'axis', (data.shape[k],))
        if ax.numel() < 2 or not bool((ax[1:] > ax[:-1]).all()):
            raise ValueError('every MHD grid axis needs at least two strictly increasing nodes')
        table, inv_width = mhd_bucket_table(ax)
        table = table.to(dev)
        keep += [ax, table]
        desc.axis[k], desc.bucket[k] = ax.data_ptr(), table.data_ptr()
        desc.n[k], desc.nb[k] = ax.numel(), table.numel()
        desc.lo[k], desc.hi[k], desc.inv_width[k] = float(ax[0]), float(ax[-1]), inv_width
    return desc, tuple(keep)


def _mhd_tables(frames, slot, ffirst: int, flast: int, dev):
    if ctypes.sizeof(MhdFrame) != _l.load().sunerf_mhd_frame_bytes():
        raise _l.SunerfHipError('SunerfMhdFrame layout differs between the library and sunerf_hip.ops.MhdFrame')
    if (not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.device != dev
            or frames.numel() % ctypes.sizeof(MhdFrame) or not frames.is_contiguous()):
        raise ValueError('frames must be a contiguous uint8 device tensor of SunerfMhdFrame records on the device of the inputs')
    if (not isinstance(slot, torch.Tensor) or slot.dtype != torch.int32 or slot.device != dev
            or tuple(slot.shape) != (flast - ffirst + 1,) or not slot.is_contiguous()):
        raise ValueError(f'slot must be a contiguous int32 ({flast - ffirst + 1},) tensor on the device of the inputs')


def _mhd_status(status):
    if int(status.item()) != 0:
        raise _l.SunerfHipError('sunerf_mhd_field: a point needed a frame that is not resident (its output is NaN)')


def mhd_field(rays_o, rays_d, z_vals, times, frames, slot, ffirst: int, flast: int):
    """MHDModel.forward (mhd_model.py:76-142) at the samples o + d z of every ray at its time ``times`` (N, 1) -> raw
    (N, S, 2) = (ln rho, log10 T).  ``frames`` / ``slot``: the resident-frame table (uint8 records of ``MhdFrame``) and the
    int32 slot of every frame ffirst..flast (-1: not resident).  Raises when a point needed a frame that is not resident."""
    n, s = z_vals.shape
    dev = z_vals.device
    rays_o = _dev(rays_o, 'rays_o', (n, 3)); rays_d = _dev(rays_d, 'rays_d', (n, 3)); z_vals = _dev(z_vals, 'z_vals', (n, s))
    times = _dev(times, 'times').reshape(-1)
    if times.shape != (n,):
        raise ValueError(f'times has {times.numel()} entries, expected one per ray ({n})')
    _mhd_tables(frames, slot, ffirst, flast, dev)
    raw = torch.empty(n, s, 2, dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    _l.call(dev, 'sunerf_mhd_field', _ptr(rays_o), _ptr(rays_d), _ptr(z_vals), _ptr(times), n, s, _ptr(frames), _ptr(slot),
            int(ffirst), int(flast), _ptr(raw), _ptr(status), _stream(dev))
    _mhd_status(status)
    return raw


def mhd_field_points(points, frames, slot, ffirst: int, flast: int):
    """:func:`mhd_field` at free-standing points (M, 4) = (x, y, z, t) -> (M, 2)."""
    dev = points.device
    points = _dev(points, 'points')
    if points.dim() != 2 or points.shape[1] != 4:
        raise ValueError(f'points has shape {tuple(points.shape)}, expected (M, 4)')
    if points.data_ptr() % 16:                  # the kernel reads a point as one 16-byte load
        points = points.clone()
    _mhd_tables(frames, slot, ffirst, flast, dev)
    m = points.shape[0]
    raw = torch.empty(m, 2, dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    _l.call(dev, 'sunerf_mhd_field_points', _ptr(points), m, _ptr(frames), _ptr(slot), int(ffirst), int(flast), _ptr(raw),
            _ptr(status), _stream(dev))
    _mhd_status(status)
    return raw


# ---- white-light Thomson scattering (thompson.py:17-109) ------------------------------------------------------------------
def _thomson_inputs(raw, z_vals, rays_o, rays_d, constants):
    n, s = z_vals.shape
    if raw.dim() != 3 or raw.shape[:2] != (n, s) or raw.shape[2] not in (1, 2):
        raise ValueError(f'raw has shape {tuple(raw.shape)}, expected ({n}, {s}, 1 or 2)')
    raw = _dev(raw.detach(), 'raw'); z_vals = _dev(z_vals, 'z_vals', (n, s))
    rays_o = _dev(rays_o, 'rays_o', (n, 3)); rays_d = _dev(rays_d, 'rays_d', (n, 3))
    names = ('solar_radius', 'limb_darkening_coeff', 'C_0')
    constants = [_dev(c.detach().reshape(1), name, (1,)) for c, name in zip(constants, names)]
    return raw, z_vals, rays_o, rays_d, constants


def thomson_integral_fwd(raw, z_vals, rays_o, rays_d, constants, kappa: float):
    """Thomson-scattering integral on the log density ``raw[..., 0]`` (N, S, C in {1, 2}), rho = exp(kappa raw0).
    ``constants``: the module's (solar_radius, limb_darkening_coeff, C_0) buffers, read on the device.  Returns dict(pixel_B
    (N,2), pixel_density, distance_from_sun, distance_from_obs (N,), weights (N,S))."""
    n, s = z_vals.shape
    dev = z_vals.device
    raw, z_vals, rays_o, rays_d, (rs, ld, c0) = _thomson_inputs(raw, z_vals, rays_o, rays_d, constants)
    f32 = dict(dtype=torch.float32, device=dev)
    out = {'pixel_B': torch.empty(n, 2, **f32), 'pixel_density': torch.empty(n, **f32),
           'distance_from_sun': torch.empty(n, **f32), 'distance_from_obs': torch.empty(n, **f32),
           'weights': torch.empty(n, s, **f32)}
    _l.call(dev, 'sunerf_thomson_integral_fwd', _ptr(raw), raw.shape[2], float(kappa), _ptr(z_vals), _ptr(rays_o),
            _ptr(rays_d), _ptr(rs), _ptr(ld), _ptr(c0), n, s, _ptr(out['pixel_B']), _ptr(out['pixel_density']),
            _ptr(out['distance_from_sun']), _ptr(out['distance_from_obs']), _ptr(out['weights']), _stream(dev))
    return out


def thomson_integral_bwd(raw, z_vals, rays_o, rays_d, constants, kappa: float, g_pixel_b=None, g_pixel_density=None,
                         g_distance_from_sun=None, g_distance_from_obs=None, g_weights=None):
    """d / d raw of :func:`thomson_integral_fwd` for the gradients of any subset of its five outputs (None = absent) ->
    (g_raw (N,S,C), absmax): channel 1 of g_raw is 0; ``absmax`` is the int32 bit pattern of max |g_raw| that
    :func:`mlp_backward` takes."""
    n, s = z_vals.shape
    dev = z_vals.device
    raw, z_vals, rays_o, rays_d, (rs, ld, c0) = _thomson_inputs(raw, z_vals, rays_o, rays_d, constants)
    g_pixel_b = None if g_pixel_b is None else _dev(g_pixel_b, 'g_pixel_B', (n, 2))
    g_pixel_density = None if g_pixel_density is None else _dev(g_pixel_density, 'g_pixel_density', (n,))
    g_distance_from_sun = None if g_distance_from_sun is None else _dev(g_distance_from_sun, 'g_distance_from_sun', (n,))
    g_distance_from_obs = None if g_distance_from_obs is None else _dev(g_distance_from_obs, 'g_distance_from_obs', (n,))
    g_weights = None if g_weights is None else _dev(g_weights, 'g_weights', (n, s))
    g_raw = torch.empty(n, s, raw.shape[2], dtype=torch.float32, device=dev)
    absmax = torch.empty(1, dtype=torch.int32, device=dev)
    _l.call(dev, 'sunerf_thomson_integral_bwd', _ptr(raw), raw.shape[2], float(kappa), _ptr(z_vals), _ptr(rays_o),
            _ptr(rays_d), _ptr(rs), _ptr(ld), _ptr(c0), n, s, _ptr(g_pixel_b), _ptr(g_pixel_density),
            _ptr(g_distance_from_sun), _ptr(g_distance_from_obs), _ptr(g_weights), _ptr(g_raw), _ptr(absmax), _stream(dev))
    return g_raw, absmax
