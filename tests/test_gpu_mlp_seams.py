"""The MLP kernels sample by sample and chunk by chunk against float64, at the seams of their decompositions.

Sum-level gates (a tensor's relative norm over a batch or a 64-ray region) cannot see a fault confined to one 32-sample chunk.
Here:
(a) forward: raw of EVERY sample against float64 (render_pass_f64's MLP, plain torch): |raw - raw64| <= 1e-4 under AUTO and
    EXACT -- the north-star budget, the image's relative error is r0's absolute error --, max(1e-4, 5e-5 max|raw|) under forced
    FAST (test_gpu_backward); the inference forward and the training forward in both stash formats;
(b) backward: one probe per call.  g_raw is zero except on one sample or one 32-sample chunk (tests/mlp_seams.py lists the chunks
    at every boundary of each kernel's decomposition); the gradient buffers are NaN-filled first; every weight and bias tensor is
    compared with float64 autograd over the probe alone (oracle mlp_probe_f64), as a relative L2 norm;
(c) the shapes: sample counts around every chunk size, other and padded widths, fewer chunks than pipelines, pipeline boundaries
    mid-ray, the fp32 any-size backward's seams, loops of the forward over a capped grid, full-size batches past 2^31 .. 2^34
    bytes of stash;
(d) the dynamic range of g_raw: 2^-140 ... 2^126 in r0 only and in r1 only, all zero, one NaN / Inf.

Routes: 'pipe hilo' / 'pipe hi' (bwd_pipe.hip with SUNERF_PIPE_HI_ONLY=0 / 1), 'classic' (render_bwd.hip dgrad + wgrad.hip),
'exact' (the fp32 small-batch kernel), 'chunked' (the fp32 any-size kernel).  Bounds per tensor: the fp16 routes
conftest.fp16_chain_bounds of the probe's own g_raw (for one sample kappa = 1; the pipelined route with the sources its phase
stash and single W^T add, pipe_bounds; the out layer at least its worst case, out_layer_worst_case), the fp32 routes 1e-4
(test_gpu_exact).  Every test prints its worst ratio of error to bound with the chunk, the layer and the tensor where it is
reached."""
import math

import pytest
import torch

import mlp_seams as sm
import sunerf_oracle as orc
from conftest import fp16_chain_bounds

pytestmark = pytest.mark.gpu

REG = 1.2
FP32_BOUND = 1e-4
NAN = float('nan')
ENV = ('SUNERF_FORWARD_PRECISION', 'SUNERF_BACKWARD', 'SUNERF_BACKWARD_PRECISION', 'SUNERF_PIPE_HI_ONLY', 'SUNERF_STASH',
       'SUNERF_EXACT_BACKWARD_SAMPLES', 'SUNERF_GRID_CAP_FWD', 'SUNERF_GRID_CAP_DGRAD', 'SUNERF_GRID_CAP_WGRAD')
ROUTES = ('pipe hilo', 'pipe hi', 'classic', 'exact', 'chunked')
FP32_ROUTES = ('exact', 'chunked')


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available()
    from sunerf_hip import ops as _ops
    return _ops


@pytest.fixture
def env(monkeypatch, ops):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(ops, '_backward_forced', None)
    ops.pipe_status(raise_on_failure=False)
    return monkeypatch


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _params(d_model, n_layers, seed=7):
    params = orc.init_params(d_filter=d_model, n_layers=n_layers, seed=seed)
    params[-1] = (params[-1][0] * 4, params[-1][1])          # absorption active on about half of the samples (test_gpu_pipe._case)
    return [(W.cuda(), b.cuda()) for W, b in params]


def _rays(n, S, seed=0):
    side = math.isqrt(n - 1) + 1
    o, d = orc.synthetic_rays(side)
    gen = torch.Generator().manual_seed(1000 * seed + 7 * n + S)
    o, d = o[:n], d[:n] * (0.9 + 0.2 * torch.rand(n, 1, generator=gen))
    t = torch.rand(n, 1, generator=gen) * 5.
    z = orc.stratified_z(o, d, orc.linspace_t_vals(S), torch.tensor(1.3), torch.tensor(1.0))
    return [x.contiguous().cuda() for x in (o, d, t, z)]


def _raw64(params, o, d, t, z, rays=1024):
    """raw of every sample in float64: render_pass_f64's points and MLP on the GPU in ray chunks (plain torch, none of the project's
    kernels)."""
    p64 = [(W.double(), b.double()) for W, b in params]
    N, S = z.shape
    out = torch.empty(N, S, p64[-1][0].shape[0], dtype=torch.float64, device=z.device)
    with torch.no_grad():
        for b in range(0, N, rays):
            sl = slice(b, b + rays)
            pts = orc.points_on_rays(o[sl], d[sl], z[sl])
            q = torch.cat([pts, t[sl][:, None].expand(-1, S, -1)], -1).double()
            out[sl] = orc.mlp_forward(p64, q.reshape(-1, 4)).reshape(-1, S, out.shape[-1])
    return out


def _packed(ops, params, mode):
    prec = {'auto': None, 'exact': ops.PRECISION_EXACT, 'fast': ops.PRECISION_FAST}[mode]
    packed = ops.PackedMLP([W for W, _ in params], [b for _, b in params], precision=prec)
    assert packed.auto == (mode == 'auto')
    return packed


def _raw_units(raw, raw64, mode):
    """max over samples of |raw - raw64| / bound, and the (ray, sample) where it is reached."""
    tol = 1e-4 if mode != 'fast' else max(1e-4, 5e-5 * raw64.abs().max().item())
    err = (raw.double() - raw64).abs().amax(-1)
    err = torch.nan_to_num(err, nan=math.inf)
    flat = int(err.argmax())
    return err.reshape(-1)[flat].item() / tol, divmod(flat, raw.shape[1])


def _use_route(ops, env, route):
    """The policy under which ops.mlp_backward takes `route`; set before the training forward, which writes the stash it reads."""
    for k in ('SUNERF_PIPE_HI_ONLY', 'SUNERF_STASH', 'SUNERF_BACKWARD_PRECISION', 'SUNERF_EXACT_BACKWARD_SAMPLES'):
        env.delenv(k, raising=False)
    env.setattr(ops, '_backward_forced', None)
    if route.startswith('pipe'):
        env.setattr(ops, '_backward_forced', 'pipe')
        env.setenv('SUNERF_PIPE_HI_ONLY', '1' if route == 'pipe hi' else '0')
    elif route == 'classic':
        env.setattr(ops, '_backward_forced', 'classic')
    elif route == 'exact':
        env.setenv('SUNERF_EXACT_BACKWARD_SAMPLES', str(1 << 40))
    else:
        env.setenv('SUNERF_BACKWARD_PRECISION', 'exact')


def pipe_bounds(bounds, n_linear, hi_only):
    """conftest.fp16_chain_bounds for the pipelined backward.  It reads the 16-bit phase stash: the activation operand X of a weight
    gradient is sin of a quantised phase (up to pi / 65535 off, sunerf_common.h:96-101) rounded to fp16, two roundings where the
    fp16 stash has one -- one more error source for the weights than the model's 2 (L - 1 - l) + 2 (measured without it: up to
    1.05 x the model on layer L - 2 of 32-sample probes).  A single fp16 W^T (SUNERF_PIPE_HI_ONLY=1) rounds the weights of every
    hidden layer the chain passes from the output down to layer l once more (the out layer's W^T is a single fp16 operand in both
    arithmetics): L - 2 - l more sources, the same for every sample, so they do not average over the probe (kappa -> max(kappa, 1)):
        weights  max(1e-3, 1.6 x 2^-12 sqrt((2 (L - 1 - l) + 3) kappa^2 + hi (L - 2 - l) max(kappa, 1)^2)),
        biases   max(1e-3, 1.6 x 2^-12 sqrt((2 (L - 1 - l) + 1) kappa^2 + hi (L - 2 - l) max(kappa, 1)^2))."""
    out = []
    for l, ((kw, bw), (kb, bb)) in enumerate(bounds):
        src, extra = 2 * (n_linear - 1 - l) + 1, (max(0, n_linear - 2 - l) if hi_only else 0)
        w = 1.6 * 2.0 ** -12 * math.sqrt((src + 2) * kw ** 2 + extra * max(kw, 1.0) ** 2)
        b = 1.6 * 2.0 ** -12 * math.sqrt(src * kb ** 2 + extra * max(kb, 1.0) ** 2)
        out.append((max(bw, w), max(bb, b)))
    return out


def out_layer_worst_case(params, o, d, t, z, ray, s0, s1, g, phase):
    """The out layer's gradients are sums over the probe of products of at most two fp16 operands, g_raw (scaled by a power of two)
    and the last activations H (for db: g alone).  fp16_chain_bounds models every operand's rounding as an independent 2^-12 and
    keeps a 1.6 margin: right for the long sums of a batch, but a probe of 1 ... 32 terms and one or two sources does not average,
    and its error can reach the worst case of round-to-nearest, 2^-11 per operand (measured up to 1.4 x that model on the out layer,
    where the hidden layers stay below 0.8 x).  The worst case, as absolute norms:
        dW_out: || sum_n |g_n| (2 x 2^-11 |h_n| + e) ||,   db_out: 2^-11 || sum_n |g_n| ||,
    e = pi / 65535, the largest error of sin decoded from the 16-bit phase stash (sunerf_common.h:96-101), for the pipelined route."""
    idx = torch.tensor([(ray, s) for s in range(s0, s1)], device=z.device)
    r, s = idx[:, 0], idx[:, 1]
    pts = orc.points_on_rays(o[r], d[r], z[r, s][:, None])[:, 0]
    q = torch.cat([pts, t.reshape(-1, 1)[r]], -1).double()
    _, hidden = orc.mlp_forward([(W.double(), b.double()) for W, b in params], q, return_hidden=True)
    ga = g.double().abs().to(q.device)
    e = math.pi / 65535 if phase else 0.0
    return (ga.T @ (2 * 2.0 ** -11 * hidden[-1].abs() + e)).norm().item(), 2.0 ** -11 * ga.sum(0).norm().item()


class Batch:
    """One network, one batch and the training forward of one route: what every probe of that route runs against."""

    def __init__(self, ops, env, route, d_model, n_layers, n_rays, S, mode='exact', seed=0):
        self.ops, self.route, self.N, self.S = ops, route, n_rays, S
        self.params = _params(d_model, n_layers)
        self.o, self.d, self.t, self.z = _rays(n_rays, S, seed)
        self.L, self.d_out = len(self.params), self.params[-1][0].shape[0]
        _use_route(ops, env, route)
        self.packed = _packed(ops, self.params, mode)
        self.D = self.packed.d_filter
        self.fwd = ops.emission_render_fwd(self.packed, self.o, self.d, self.t, self.z, REG, training=True)
        if route in FP32_ROUTES:
            return
        fmt = ops.stash_format_of(self.fwd['stash'], n_rays, S, self.packed)
        assert fmt == (ops.STASH_PHASE if route.startswith('pipe') else ops.STASH_FP16), (route, fmt)

    def backward(self, g_raw, onto=None):
        """ops.mlp_backward on g_raw (N, S, 2) with absmax = the bit pattern of its own max |g_raw|, into NaN-filled buffers (or
        added onto copies of ``onto``)."""
        ops = self.ops
        absmax = g_raw.abs().max().reshape(1).contiguous().view(torch.int32)
        if onto is None:
            gW = [torch.full_like(W, NAN) for W, _ in self.params]
            gb = [torch.full_like(b, NAN) for _, b in self.params]
        else:
            gW, gb = [x.clone() for x in onto[0]], [x.clone() for x in onto[1]]
        ops.mlp_backward(self.packed, g_raw, absmax, self.fwd['stash'], gW, gb, accumulate=onto is not None,
                         query=('rays', self.o, self.d, self.t, self.z))
        torch.cuda.synchronize()
        if self.route.startswith('pipe'):
            assert ops.pipe_status(raise_on_failure=False) == 0
        return gW, gb

    def probe(self, ray, s0, s1, g, onto=None):
        """g (s1 - s0, 2) on samples [s0, s1) of `ray`, zero elsewhere -> (kernel gradients, float64 gradients)."""
        g_raw = torch.zeros(self.N, self.S, 2, device='cuda')
        g_raw[ray, s0:s1] = g.to(g_raw)
        got = self.backward(g_raw, onto)
        _, want = orc.mlp_probe_f64(self.params, self.o, self.d, self.t, self.z, [(ray, s) for s in range(s0, s1)],
                                    g[:, :self.d_out].cuda())
        return got, want

    def bounds(self, ray, s0, s1, g, want):
        """[(weight bound, bias bound)] per layer for a probe; the out layer's also at least its worst case (out_layer_worst_case)."""
        if self.route in FP32_ROUTES:
            return [(FP32_BOUND, FP32_BOUND)] * self.L
        sl = slice(ray, ray + 1)
        bw, bb = fp16_chain_bounds(self.params, self.o[sl], self.d[sl], self.t[sl], self.z[sl, s0:s1], g[None].cuda())
        if self.route.startswith('pipe'):
            out = pipe_bounds(list(zip(bw, bb)), self.L, self.route == 'pipe hi')
        else:
            out = [(w, b) for (_, w), (_, b) in zip(bw, bb)]
        ew, eb = out_layer_worst_case(self.params, self.o, self.d, self.t, self.z, ray, s0, s1, g[:, :self.d_out],
                                      self.route.startswith('pipe'))
        out[-1] = (max(out[-1][0], ew / want[-1][0].norm().item()), max(out[-1][1], eb / want[-1][1].norm().item()))
        return out


def _ratios(got, want, bounds, floor=None):
    """[(layer, 'W' / 'b', ratio)]: ||got - want|| / (bound ||want|| + floor(l) sqrt(numel)); non-finite got -> inf.  ``floor(l)``:
    an absolute per-element floor (subnormal results)."""
    out = []
    for l, (g, r, bd) in enumerate(zip(zip(*got), want, bounds)):
        for kind, x, y, b in (('W', g[0], r[0], bd[0]), ('b', g[1], r[1], bd[1])):
            x = x.double()
            if not bool(torch.isfinite(x).all()):
                out.append((l, kind, math.inf))
                continue
            err = (x - y).norm().item()
            allow = b * y.norm().item() + (floor(l) * math.sqrt(y.numel()) if floor else 0.0)
            out.append((l, kind, err / allow if allow > 0 else (0.0 if err == 0 else math.inf)))
    return out


def _run_probes(batch, probes, label, gen=None, single_samples=True):
    """One probe per (ray, s0, s1, why), plus the first and the last sample of the batch alone; asserts every tensor of every probe
    within its bound and prints the worst ratio."""
    gen = gen or torch.Generator().manual_seed(batch.N * 1000 + batch.S)
    probes = list(probes)
    if single_samples:
        probes += [(0, 0, 1, 'first sample alone'), (batch.N - 1, batch.S - 1, batch.S, 'last sample alone')]
    worst, fails = (0.0, ''), []
    for ray, s0, s1, why in probes:
        g = torch.randn(s1 - s0, 2, generator=gen)
        got, want = batch.probe(ray, s0, s1, g)
        for l, kind, r in _ratios(got, want, batch.bounds(ray, s0, s1, g, want)):
            where = f'{why} (ray {ray}, samples {s0}..{s1 - 1}), layer {l} {kind}'
            if r > worst[0]:
                worst = (r, where)
            if not r <= 1.0:
                fails.append(f'{where}: {r:.3g} x the bound')
    print(f'\n  {label} [{batch.route}]: {len(probes)} probes, worst error / bound {worst[0]:.3f} at {worst[1]}')
    assert not fails, fails[:10]
    return worst[0]


def _seams(batch, fwd_grid=None, dgrad_grid=None, wgrad_cus=None):
    N, S, cus = batch.N, batch.S, _cus()
    seams = sm.chunk_seams(N, S)
    seams.update(sm.forward_seams(N, S, fwd_grid or cus))
    if batch.route.startswith('pipe'):
        seams.update(sm.pipe_seams(N, S, batch.L, cus))
    elif batch.route == 'classic':
        seams.update(sm.dgrad_seams(N, S, dgrad_grid or cus))
        seams.update(sm.wgrad_seams(N, S, batch.ops.wgrad_split(batch.L, wgrad_cus or cus, batch.D)))
    elif batch.route == 'chunked':
        seams.update(sm.exact_seams(N, S, batch.D))
    return seams


# ---- (a) forward, every sample ----------------------------------------------------------------------------------------

FWD_SHAPES = ([(256, 8, 5, S, 0) for S in (2, 31, 32, 33, 63, 64, 65, 127, 128, 129)]
              + [(64, 3, 9, 65, 0), (128, 4, 9, 65, 0), (512, 8, 6, 65, 0), (512, 2, 5, 33, 0), (100, 8, 7, 33, 0)]
              + [(256, 8, 1025, 33, 0),                                    # 257 groups of 4 rays over 256 workgroups: a second sweep
                 (256, 8, 37, 65, 3), (512, 8, 37, 33, 3), (64, 3, 37, 33, 3)])   # 10 groups over a grid capped at 3


@pytest.mark.parametrize('d_model,n_layers,n,S,cap', FWD_SHAPES,
                         ids=[f'{L}x{D}-{n}x{S}' + (f'-cap{c}' if c else '') for D, L, n, S, c in FWD_SHAPES])
def test_forward_every_sample_against_float64(ops, env, d_model, n_layers, n, S, cap):
    if cap:
        env.setenv('SUNERF_GRID_CAP_FWD', str(cap))
    assert len(sm.forward_seam_rays(n, cap or _cus())) >= (2 if n > 1000 or cap else 1)
    params = _params(d_model, n_layers)
    o, d, t, z = _rays(n, S)
    raw64 = _raw64(params, o, d, t, z)
    worst = {}
    for mode in ('auto', 'exact', 'fast'):
        packed = _packed(ops, params, mode)
        kinds = ['inference', 'training fp16'] + (['training phase'] if packed.d_filter == 256 and n_layers >= 2 else [])
        for kind in kinds:
            env.delenv('SUNERF_STASH', raising=False)
            if kind == 'inference':
                out = ops.emission_render_fwd(packed, o, d, t, z, REG, want_raw=True)
            else:
                if kind == 'training fp16':
                    env.setenv('SUNERF_STASH', 'fp16')
                out = ops.emission_render_fwd(packed, o, d, t, z, REG, training=True)
                fmt = ops.stash_format_of(out['stash'], n, S, packed)
                assert fmt == (ops.STASH_FP16 if kind == 'training fp16' else ops.STASH_PHASE), kind
            torch.cuda.synchronize()
            units, where = _raw_units(out['raw'], raw64, mode)
            worst[f'{mode}/{kind}'] = (units, where)
    print(f'\n  forward {n_layers} x {d_model}, {n} x {S}' + (f', grid cap {cap}' if cap else '') + ': worst |raw - raw64| / bound '
          + ', '.join(f'{k} {u:.3f} at {w}' for k, (u, w) in worst.items()))
    assert all(u <= 1.0 for u, _ in worst.values()), worst


# ---- (b) + (c) backward probes at the seams ---------------------------------------------------------------------------

SWEEP = [(n, S) for S in (2, 31, 32, 33, 63, 64, 65, 127, 128, 129) for n in (1, 3, 5)]


@pytest.mark.parametrize('route', ('pipe hilo', 'pipe hi', 'classic', 'exact'))
@pytest.mark.parametrize('n,S', SWEEP, ids=[f'{n}x{S}' for n, S in SWEEP])
def test_backward_probes_around_every_chunk_size(ops, env, route, n, S):
    b = Batch(ops, env, route, 256, 8, n, S)
    _run_probes(b, sm.as_probes(_seams(b), S), f'8 x 256, {n} x {S}')


WIDTHS = [(64, 3, 6, 65), (128, 4, 6, 65), (512, 8, 6, 65), (512, 2, 5, 33), (100, 8, 5, 33)]


@pytest.mark.parametrize('route', ('classic', 'exact'))
@pytest.mark.parametrize('d_model,n_layers,n,S', WIDTHS, ids=[f'{L}x{D}-{n}x{S}' for D, L, n, S in WIDTHS])
def test_backward_probes_at_other_widths(ops, env, route, d_model, n_layers, n, S):
    b = Batch(ops, env, route, d_model, n_layers, n, S)
    _run_probes(b, sm.as_probes(_seams(b), S), f'{n_layers} x {d_model}, {n} x {S}')


@pytest.mark.parametrize('route', ('pipe hilo', 'pipe hi', 'classic'))
def test_backward_probes_with_fewer_chunks_than_pipelines_and_workgroups(ops, env, route):
    b = Batch(ops, env, route, 256, 8, 1, 33)
    _run_probes(b, [(0, s, s + 1, f'sample {s} alone') for s in (0, 31, 32)] + sm.as_probes(_seams(b), 33), '8 x 256, 1 x 33')


@pytest.mark.parametrize('route', ('pipe hilo', 'pipe hi'))
@pytest.mark.parametrize('n_layers', (8, 5))
def test_pipe_probes_at_pipeline_boundaries_mid_ray(ops, env, route, n_layers):
    b = Batch(ops, env, route, 256, n_layers, 2048, 128)
    seams = _seams(b)
    assert n_layers == 8 or any(c % 4 for c in seams)           # 24 pipelines of 342 chunks: boundaries inside a ray
    _run_probes(b, sm.as_probes(seams, 128), f'{n_layers} x 256, 2048 x 128 ({sm.pipe_pipelines(b.L)} pipelines)')


def test_chunked_fp32_probes_at_its_seams(ops, env):
    b = Batch(ops, env, 'chunked', 256, 8, 2048, 97)
    seams = _seams(b)
    assert sum('fp32 chunk seam' in why for why in seams.values()) >= 6
    _run_probes(b, sm.as_probes(seams, 97), '8 x 256, 2048 x 97')


@pytest.mark.parametrize('route', ('pipe hilo', 'classic'))
def test_backward_probes_behind_the_forward_and_dgrad_loops(ops, env, route):
    """The stash slices the forward writes in its second sweep (1025 rays on 256 workgroups; 37 rays on a grid capped at 3); the
    classic backward with its own loops capped too (dgrad grid 3, wgrad as if on 40 CUs: 4 slices whose edges fall inside rays)."""
    b = Batch(ops, env, route, 256, 8, 1025, 33)
    _run_probes(b, sm.as_probes(_seams(b), 33), '8 x 256, 1025 x 33')
    env.setenv('SUNERF_GRID_CAP_FWD', '3')
    if route == 'classic':
        env.setenv('SUNERF_GRID_CAP_DGRAD', '3')
        env.setenv('SUNERF_GRID_CAP_WGRAD', '40')
    b = Batch(ops, env, route, 256, 8, 37, 65)
    _run_probes(b, sm.as_probes(_seams(b, fwd_grid=3, dgrad_grid=3, wgrad_cus=40), 65), '8 x 256, 37 x 65, capped grids')


def test_accumulate_adds_a_probe_onto_a_known_buffer(ops, env):
    """accumulate=True on every route: buffer + the probe's gradients, to the probe's bound plus the fp32 rounding of the sum."""
    gen = torch.Generator().manual_seed(5)
    worst = {}
    for route in ROUTES:
        b = Batch(ops, env, route, 256, 8, 3, 65)
        g = torch.randn(32, 2, generator=gen)
        _, want = b.probe(1, 32, 64, g)
        onto = ([(torch.randn(W.shape, generator=gen) * w.abs().max().item()).float().cuda() for (W, _), (w, _) in zip(b.params, want)],
                [(torch.randn(B.shape, generator=gen) * bb.abs().max().item()).float().cuda() for (_, B), (_, bb) in zip(b.params, want)])
        got, _ = b.probe(1, 32, 64, g, onto=onto)
        bounds = b.bounds(1, 32, 64, g, want)
        r = 0.0
        for l, ((gw, gb), (rw, rb), (bw, bb), ow, ob) in enumerate(zip(zip(*got), want, bounds, *onto)):
            for x, y, bd, o in ((gw, rw, bw, ow), (gb, rb, bb, ob)):
                err = (x.double() - o.double() - y).norm().item()
                r = max(r, err / (bd * y.norm().item() + 2.0 ** -23 * o.norm().item()))
        worst[route] = r
    print('\n  accumulate: worst error / bound ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst


# ---- full size ---------------------------------------------------------------------------------------------------------

def test_full_size_pipe_every_sample_and_every_seam(ops, env):
    """bench.py's batch, 32768 x 128 on the 8 x 256 network: the AUTO training forward with the 16-bit phase stash (18 GB: its byte
    offsets pass 2^31 ... 2^34), raw of all 4.2e6 samples against float64; then pipelined-backward probes at the first and last
    chunk and the first ring wraps of all 16 pipelines, the prologue's ranges and the stash offsets, under both W^T settings."""
    b = Batch(ops, env, 'pipe hilo', 256, 8, 32768, 128, mode='auto')
    units, where = _raw_units(b.fwd['raw'], _raw64(b.params, b.o, b.d, b.t, b.z), 'auto')
    print(f'\n  full size 8 x 256, 32768 x 128: AUTO forward chose {ops.PRECISION_NAMES[b.packed.precision]}, '
          f'worst |raw - raw64| / 1e-4 = {units:.3f} at (ray, sample) {where}')
    assert units <= 1.0
    seams = sm.pipe_seams(b.N, b.S, b.L, _cus())
    seams.update(sm.chunk_seams(b.N, b.S))
    offsets = sm.offset_seams(b.N, b.S, 256, b.L, sm.STASH_PHASE)
    assert len(offsets) == 8
    seams.update(offsets)
    probes = sm.as_probes(seams, b.S)
    _run_probes(b, probes, 'full size, SUNERF_PIPE_HI_ONLY=0')
    env.setenv('SUNERF_PIPE_HI_ONLY', '1')
    b.route = 'pipe hi'
    _run_probes(b, probes, 'full size, SUNERF_PIPE_HI_ONLY=1')


def test_full_size_classic_at_the_reference_width(ops, env):
    """8192 x 128 on the 8 x 512 network through dgrad + wgrad: the fp16 stash (17 GB) past 2^31 ... 2^34, the dz stash (8.6 GB)
    past 2^31 and 2^32, the 7 wgrad slices, raw of every sample against float64."""
    b = Batch(ops, env, 'classic', 512, 8, 8192, 128, mode='auto')
    units, where = _raw_units(b.fwd['raw'], _raw64(b.params, b.o, b.d, b.t, b.z), 'auto')
    print(f'\n  full size 8 x 512, 8192 x 128: AUTO forward chose {ops.PRECISION_NAMES[b.packed.precision]}, '
          f'worst |raw - raw64| / 1e-4 = {units:.3f} at (ray, sample) {where}')
    assert units <= 1.0
    seams = _seams(b)
    offsets = sm.offset_seams(b.N, b.S, 512, b.L, sm.STASH_FP16)
    offsets.update(sm.dz_offset_seams(b.N, b.S, 512, b.L))
    assert len(offsets) == 12
    seams.update(offsets)
    _run_probes(b, sm.as_probes(seams, b.S), 'full size 8 x 512')


def test_pipe_workspace_restatement_on_the_device(ops):
    lib = ops._l.load()
    assert _cus() == 256
    for n, S, nl in ((1, 33, 9), (2048, 128, 9), (2048, 128, 6), (32768, 128, 9)):
        got = lib.sunerf_bwd_pipe_workspace_bytes(n, S, 256, nl)
        assert got > 0 and got == sm.pipe_workspace_bytes(n, S, nl), (n, S, nl)


# ---- (d) dynamic range of g_raw ---------------------------------------------------------------------------------------

MAGNITUDES = (-140, -126, -120, 0, 100, 126)


@pytest.mark.parametrize('route', ROUTES)
def test_dynamic_range_of_g_raw(ops, env, route):
    """One sample, g = +-2^e in r0 only and in r1 only.  Against float64 with the relative bound of the route and an absolute floor
    per element of the fp32 subnormal spacing 2^-149 times the number of products summed on the way from g_raw to an element of
    layer l's gradients, D (L - l): below 2^-126 fp32 itself (the reference's arithmetic) keeps no more than that."""
    b = Batch(ops, env, route, 256, 8, 3, 65)
    gen = torch.Generator().manual_seed(3)
    fails, report = [], []
    for e in MAGNITUDES:
        for ch in (0, 1):
            g = torch.zeros(1, 2)
            g[0, ch] = (1.0 if torch.rand(1, generator=gen).item() < 0.5 else -1.0) * 2.0 ** e
            got, want = b.probe(1, 40, 41, g)
            unit = b.bounds(1, 40, 41, g, want)
            rs = _ratios(got, want, unit, floor=lambda l: 2.0 ** -149 * b.D * (b.L - l))
            worst = max(rs, key=lambda x: x[2])
            report.append(f'2^{e} r{ch} {worst[2]:.3f}')
            if not worst[2] <= 1.0:
                fails.append(f'2^{e} in r{ch}: layer {worst[0]} {worst[1]} at {worst[2]:.3g} x the bound')
    print(f'\n  dynamic range [{route}]: worst error / bound ' + ', '.join(report))
    assert not fails, fails


@pytest.mark.parametrize('route', ROUTES)
def test_zero_and_non_finite_g_raw(ops, env, route):
    """All-zero g_raw: every gradient exactly +0.0.  One NaN / +-Inf sample: non-finite gradients somewhere, so that ClipAdam's guard
    skips the step (test_gpu_train_step covers the skip)."""
    b = Batch(ops, env, route, 256, 8, 3, 65)
    gW, gb = b.backward(torch.zeros(b.N, b.S, 2, device='cuda'))
    for i, x in enumerate(gW + gb):
        assert bool((x == 0).all()) and not bool(torch.signbit(x).any()), (route, i)
    for bad in (NAN, math.inf, -math.inf):
        for ch in (0, 1):
            g_raw = torch.zeros(b.N, b.S, 2, device='cuda')
            g_raw[1, 40, ch] = bad
            g_raw[2, 3] = 0.25                     # and a finite sample elsewhere
            gW, gb = b.backward(g_raw)
            assert any(not bool(torch.isfinite(x).all()) for x in gW + gb), (route, bad, ch)
