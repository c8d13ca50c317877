"""One case builder per entry point of the C ABI (include/sunerf_hip.h), for tests/test_gpu_abi_extents.py and
tests/test_abi_extents_host.py.

``CASES[name] = (builder, shapes)``.  ``builder(shape, device)`` returns a :class:`Case`: the full argument
tuple of ``lib.call(dev, name, ...)`` in which every pointer is a buffer of a guarded arena (tests/abi_arena.py) tagged IN, OUT,
INOUT or WORKSPACE and sized FROM THE HEADER's shape comment (not from the Python wrappers: the case is a check of that
documentation), and ``expected``: the same computation through the project's own wrapper on the same inputs, which proves
that the direct call ran the kernel at that shape.  The wrappers' values are held to float64 by their own test files.

Builders run on ``device='cpu'`` too (the host test checks tags, counts and the order of arguments there); inputs that only a
kernel can make (an activation stash, a packed weight image) are zeros then.

Guard rule (``guard_bytes`` of a buffer): 1 MiB per side, or more where one workgroup's share of the buffer is larger -- given
per buffer below (``_stash_guard``, ``_dz_guard``, ``_pipe_guard``); nothing else in this ABI hands a workgroup more than 1 MiB.

Shapes are the smallest at which a tail can go wrong: 1, one below and one above every tile the kernel uses (named in
``TILES``), and one shape of three tiles with a ragged end.
"""
import ctypes
import functools
import math
import os

import numpy as np
import torch

from abi_arena import IN, INOUT, OUT, WORKSPACE, Absent, Arena, Buffer

F32, F64, I32, I64, U8 = torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8
STREAM = 'STREAM'                 # placeholder of the last argument: the test passes the current stream


class HostPtrs:
    """A host array of device pointers (``const float* const*``): the per-layer tensor lists of the MLP entry points."""

    def __init__(self, buffers):
        self.buffers = list(buffers)

    def value(self):
        return (ctypes.c_void_p * max(1, len(self.buffers)))(*[b.ptr.value for b in self.buffers])


class HostValue:
    """A host-side argument handed over as it is (a struct by value or by reference, a host array)."""

    def __init__(self, value, keep=None):
        self._value, self.keep = value, keep

    def value(self):
        return self._value


class Case:
    def __init__(self, name, shape, arena, args, expected=None, ws_index=None, empty=None, empty_effect=None,
                 reproducible=True, tolerance=None, opaque=(), rejections=()):
        self.name, self.shape, self.arena, self.args = name, shape, arena, list(args)
        self.expected = expected            # callable -> {buffer name: tensor}; every OUT / INOUT buffer that is not opaque
        self.ws_index = ws_index            # position of `workspace_bytes` in args (None: the entry point takes none)
        self.empty = empty                  # {position: value} that turns the call into the documented "nothing to do"
        self.empty_effect = empty_effect    # callable -> {buffer name: tensor}: the documented effect of the empty call
        self.reproducible = reproducible
        # reproducible=False (the reason is in the kernel source and named in the case): callable(name, got, want) that holds the
        # outputs the kernel adds with float atomics to the bound of the kernel's own test file, every other output to its bits
        self.tolerance = tolerance
        self.opaque = set(opaque) & {b.name for b in arena.buffers}           # OUT buffers whose layout the header does not give: compared between runs only
        self.rejections = list(rejections)  # [({position: value}, status)]: calls the header documents as refused, nothing written
        self.expect_status = None           # a documented rejection: the status the call must return, writing nothing

    def ctypes_args(self, stream, overrides=None):
        out = []
        for i, a in enumerate(self.args):
            if overrides and i in overrides:
                a = overrides[i]
            if isinstance(a, (Buffer, Absent)):
                out.append(a.ptr)
            elif isinstance(a, (HostPtrs, HostValue)):
                out.append(a.value())
            elif isinstance(a, str) and a == STREAM:
                out.append(stream)
            else:
                out.append(a)
        return out


class Ctx:
    """What a builder works with: the arena of the case and shorthands for tagged buffers."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.gpu = self.device.type == 'cuda'
        self.arena = Arena(self.device)

    def IN(self, name, data, dtype=None, **kw):
        data = torch.as_tensor(data)
        if dtype is not None:
            data = data.to(dtype)
        return self.arena.alloc(name, IN, data.dtype, data.numel(), data=data.contiguous(), **kw)

    def INOUT(self, name, data, **kw):
        data = torch.as_tensor(data)
        return self.arena.alloc(name, INOUT, data.dtype, data.numel(), data=data.contiguous(), **kw)

    def OUT(self, name, dtype, numel, **kw):
        return self.arena.alloc(name, OUT, dtype, numel, **kw)

    def WS(self, name, nbytes, **kw):
        return self.arena.alloc(name, WORKSPACE, U8, nbytes, **kw)

    def NULL(self, name, tag):
        return Absent(name, tag)


def _lib():
    from sunerf_hip import lib
    return lib.load()


CASES = {}
TILES = {}


def case(name, shapes, tiles):
    def deco(fn):
        CASES[name] = (fn, tuple(shapes))
        TILES[name] = tiles
        return fn
    return deco


def shape_id(shape):
    return '-'.join(str(int(v) if isinstance(v, bool) else v) for v in shape) if isinstance(shape, tuple) else str(shape)


# ---- entry points that touch no device memory ----------------------------------------------------------------------------------
NO_DEVICE_ACCESS = {
    'sunerf_abi_version': 'returns a constant',
    'sunerf_packed_mlp_bytes': 'size query: arithmetic on its arguments',
    'sunerf_packed_mlp_t_bytes': 'size query: arithmetic on its arguments',
    'sunerf_act_stash_bytes': 'size query: arithmetic on its arguments',
    'sunerf_render_workspace_bytes': 'size query: arithmetic on its arguments',
    'sunerf_dz_stash_bytes': 'size query: arithmetic on its arguments',
    'sunerf_wgrad_workspace_bytes': 'size query: arithmetic on its arguments',
    'sunerf_bwd_pipe_workspace_bytes': 'size query: arithmetic on its arguments and the CU count of the current device',
    'sunerf_mlp_backward_exact_workspace_bytes': 'size query: arithmetic on its arguments',
    'sunerf_mlp_backward_exact_chunked_workspace_bytes': 'size query: arithmetic on its arguments',
    'sunerf_mlp_input_grad_exact_workspace_bytes': 'size query: arithmetic on its arguments',
    'sunerf_view_desc_bytes': 'size query: sizeof(SunerfViewDesc)',
    'sunerf_observer_desc_bytes': 'size query: sizeof(SunerfObserverDesc)',
    'sunerf_map_fill_workspace_bytes': 'size query: arithmetic on its arguments',
    'sunerf_simple_star_bwd_workspace_bytes': 'size query: a constant',
    'sunerf_mhd_frame_bytes': 'size query: sizeof(SunerfMhdFrame)',
    'sunerf_train_workspace_bytes': 'size query: a constant',
    'sunerf_image_metrics_workspace_bytes': 'size query: arithmetic on its arguments',
    'sunerf_volume_metrics_workspace_bytes': 'size query: arithmetic on its arguments',
    'sunerf_grid_field_desc_bytes': 'size query: sizeof(SunerfGridFieldDesc)',
    'sunerf_grid_field_bwd_workspace_bytes': 'size query: arithmetic on its arguments',
    'sunerf_bwd_pipe_kernel_time': 'waits for library-owned HIP events and writes two HOST words; no device pointer',
}

# ---- shapes ---------------------------------------------------------------------------------------------------------------------
# per-ray kernels: 256-thread workgroups of four 64-lane waves, a ray per wave or a sample per thread
RAYS = (1, 3, 65)
SAMPLES = (1, 31, 33, 65)
RAY_SHAPES = tuple((n, s) for n in RAYS for s in SAMPLES)
RAY_SHAPES_S2 = tuple((n, max(s, 2)) for n, s in RAY_SHAPES)          # entry points whose header asks for n_samples >= 2
RAY_SHAPES_S3 = tuple((n, max(s, 3)) for n, s in RAY_SHAPES)          # ... for n_samples >= 3 (the DT integral)
# the fused render and the fp16 backward need n_samples >= 2: the smallest batch is one ray of two samples
MLP_SHAPES = tuple((d, n, s) for d in (64, 256) for n, s in ((1, 2), (3, 33), (5, 65)))


@functools.lru_cache(maxsize=None)
def _emission_case(n, s):
    from test_gpu_emission_integral import make_case
    e = make_case(n, max(s, 3), 1000 * n + s)          # the generator needs three samples: S = 1 takes the first of them
    return {k: (v[:, :s].contiguous() if k in ('raw', 'z') else v) for k, v in e.items()}


@functools.lru_cache(maxsize=None)
def _dt_case(n, s, w):
    from test_gpu_dt_integral import make_case
    e = make_case(n, max(s, 3), w, 'nerf_dt', 1000 * n + s)          # as above
    return {k: (v[:, :s].contiguous() if k in ('raw', 'z') else v) for k, v in e.items()}


def _dt_tables():
    from test_gpu_dt_integral import tables
    return tables()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rand(gen, *shape):
    return torch.rand(*shape, generator=gen)


# ---- sampling -------------------------------------------------------------------------------------------------------------------
@case('sunerf_sample_z', [(n, s, kind, jitter) for n, s in RAY_SHAPES for kind, jitter in ((0, False), (1, True))],
      'sampler.hip RS_THREADS 256: one sample per thread, n * S rounded up to whole blocks')
def sample_z(shape, device):
    import sample_z_reference as sz
    n, s, kind, jitter = shape
    c = Ctx(device)
    o, d, _, t_vals, t_rand = sz.make_case(n, s, 1000 * n + s)
    o, d = np.nan_to_num(o, nan=1.0, posinf=1.0, neginf=-1.0), np.nan_to_num(d, nan=1.0, posinf=1.0, neginf=-1.0)
    distance, solar_R = (sz.STRATIFIED_CONSTANTS if kind == sz.STRATIFIED else sz.SPHERICAL_CONSTANTS)[0]
    ro, rd, tv = c.IN('rays_o', o), c.IN('rays_d', d), c.IN('t_vals', t_vals)
    tr = c.IN('t_rand', t_rand) if jitter else c.NULL('t_rand', IN)
    z = c.OUT('z_vals', F32, n * s)

    def expected():
        from sunerf_hip import ops
        return {'z_vals': ops.sample_z(kind, ro.t.view(n, 3), rd.t.view(n, 3), tv.t, distance, solar_R,
                                       t_rand=tr.t.view(n, s) if jitter else None)}
    return Case('sunerf_sample_z', shape, c.arena, [kind, ro, rd, tv, tr, n, s, float(distance), float(solar_R), z, STREAM],
                expected, empty={5: 0})


def _resample_inputs(n, sc, sf, per_ray):
    from test_gpu_resample import make_rays
    z, w = make_rays(n, sc, 100 * n + sc)
    gen = _gen(7 * n + sf)
    u = torch.sort(_rand(gen, n, sf), -1).values if per_ray else torch.linspace(0., 1., sf)
    return z, w, u.contiguous()


RESAMPLE_SHAPES = [(n, sc, sf, per_ray) for n in RAYS for sc, sf in ((3, 1), (31, 33), (33, 31), (65, 65)) for per_ray in (0, 1)]


@case('sunerf_hier_resample', RESAMPLE_SHAPES, 'sampler.hip RS_THREADS 256: one wave of 64 lanes per ray, four rays per block')
def hier_resample(shape, device):
    n, sc, sf, per_ray = shape
    c = Ctx(device)
    z, w, u = _resample_inputs(n, sc, sf, per_ray)
    zb, wb, ub = c.IN('z_vals', z), c.IN('weights', w), c.IN('u', u)
    new_z, z_comb = c.OUT('new_z', F32, n * sf), c.OUT('z_comb', F32, n * (sc + sf))

    def expected():
        from sunerf_hip import ops
        nz, zc = ops.hier_resample(zb.t.view(n, sc), wb.t.view(n, sc), ub.t.view(n, sf) if per_ray else ub.t)
        return {'new_z': nz, 'z_comb': zc}
    return Case('sunerf_hier_resample', shape, c.arena, [zb, wb, ub, per_ray, n, sc, sf, new_z, z_comb, STREAM], expected,
                empty={4: 0})


@case('sunerf_sample_pdf', RESAMPLE_SHAPES, 'sampler.hip RS_THREADS 256: one wave of 64 lanes per ray, four rays per block')
def sample_pdf(shape, device):
    n, nb, sf, per_ray = shape
    c = Ctx(device)
    z, w, u = _resample_inputs(n, nb, sf, per_ray)
    bins, wb, ub = c.IN('bins', z), c.IN('weights', w[:, :nb - 1].contiguous()), c.IN('u', u)
    samples = c.OUT('samples', F32, n * sf)

    def expected():
        from sunerf_hip import ops
        return {'samples': ops.sample_pdf(bins.t.view(n, nb), wb.t.view(n, nb - 1), ub.t.view(n, sf) if per_ray else ub.t)}
    return Case('sunerf_sample_pdf', shape, c.arena, [bins, wb, ub, per_ray, n, nb, sf, samples, STREAM], expected, empty={4: 0})


# ---- line-of-sight integrals ----------------------------------------------------------------------------------------------------
@case('sunerf_emission_integral_fwd', RAY_SHAPES_S2, 'render_bwd.hip IB_THREADS 256: eight rays per workgroup, 32 samples per pass')
def emission_integral_fwd(shape, device):
    n, s = shape
    c = Ctx(device)
    e = _emission_case(n, s)
    raw, z, d = c.IN('raw', e['raw']), c.IN('z_vals', e['z']), c.IN('rays_d', e['d'])
    image, weights, absorption = c.OUT('image', F32, n), c.OUT('weights', F32, n * s), c.OUT('absorption', F32, n * s)

    def expected():
        from sunerf_hip import ops
        im, w, a = ops.emission_integral_fwd(raw.t.view(n, s, 2), z.t.view(n, s), d.t.view(n, 3))
        return {'image': im, 'weights': w, 'absorption': a}
    return Case('sunerf_emission_integral_fwd', shape, c.arena, [raw, z, d, n, s, image, weights, absorption, STREAM], expected,
                empty={3: 0})


@case('sunerf_emission_integral_bwd', [(n, s, full) for n, s in RAY_SHAPES_S2 for full in (0, 1)],
      'render_bwd.hip IB_THREADS 256: eight rays per workgroup, 32 samples per pass')
def emission_integral_bwd(shape, device):
    n, s, full = shape
    c = Ctx(device)
    e = _emission_case(n, s)
    gen = _gen(n * 77 + s)
    raw, z, o, d = c.IN('raw', e['raw']), c.IN('z_vals', e['z']), c.IN('rays_o', e['o']), c.IN('rays_d', e['d'])
    g_image = c.IN('g_image', 0.25 + _rand(gen, n))
    if full:
        g_reg, g_w, g_a = (c.IN(k, 0.5 - _rand(gen, n, s)) for k in ('g_reg', 'g_weights', 'g_absorption'))
    else:
        g_reg, g_w, g_a = (c.NULL(k, IN) for k in ('g_reg', 'g_weights', 'g_absorption'))
    g_raw, absmax = c.OUT('g_raw', F32, n * s * 2), c.OUT('g_absmax', I32, 1)
    g_reg_const, reg_radius = 1e-3, 1.2

    def expected():
        from sunerf_hip import ops
        v = lambda b: b.t.view(n, s) if full else None          # noqa: E731
        g, am = ops.emission_integral_bwd(raw.t.view(n, s, 2), z.t.view(n, s), d.t.view(n, 3), g_image.t, v(g_w), v(g_a),
                                          rays_o=o.t.view(n, 3), g_reg=v(g_reg), g_reg_const=g_reg_const, reg_radius=reg_radius,
                                          return_absmax=True)
        return {'g_raw': g, 'g_absmax': am}
    return Case('sunerf_emission_integral_bwd', shape, c.arena,
                [raw, z, o, d, g_image, g_reg, g_w, g_a, g_reg_const, reg_radius, n, s, g_raw, absmax, STREAM], expected, empty={10: 0},
                empty_effect=lambda: {'g_absmax': torch.zeros(1, dtype=I32)})          # header: an empty batch clears the word


# dt_sweep.h, the end of dt_bwd_kernel ("parameter gradients" and the final atomics): every ray adds its g_log_abs / g_vol_c
# terms to the workgroup's LDS sums with atomicAdd, and every workgroup adds those to the outputs with atomicAdd: from three
# terms on the order of the float adds is free (two terms commute)
DT_ORDERED_RAYS = 2
DT_SHAPES = [(n, s, w, epi) for n, s in RAY_SHAPES_S3 for w, epi in ((1, 0), (7, 1))]


def _dt_inputs(c, n, s, w):
    e = _dt_case(n, s, w)
    lt, resp = _dt_tables()
    b = dict(raw=c.IN('raw', e['raw']), z=c.IN('z_vals', e['z']), o=c.IN('rays_o', e['o']), d=c.IN('rays_d', e['d']),
             wl=c.IN('wavelengths', e['wl']), lt=c.IN('table_logt', lt), resp=c.IN('table_resp', resp),
             la=c.IN('log_abs', e['log_abs'].float()), vc=c.IN('vol_c', e['vol_c'].float()))
    head = [b['raw'], b['z'], b['o'], b['d'], b['wl'], w, b['lt'], b['resp'], b['la'], b['vc'], 10.0, 5.0, float(e['pixel']), 1.25, n, s]
    return e, b, head


def _dt_wrapper_args(b, e, n, s, w):
    return (b['raw'].t.view(n, s, 2), b['z'].t.view(n, s), b['o'].t.view(n, 3), b['d'].t.view(n, 3), b['wl'].t.view(n, w),
            b['lt'].t.view(7, 101), b['resp'].t.view(7, 101), b['la'].t, b['vc'].t, 10.0, 5.0, float(e['pixel']), 1.25)


@case('sunerf_dt_integral_fwd', DT_SHAPES, 'dt_sweep.h DT_THREADS 256: one wave per ray, 64 samples per pass')
def dt_integral_fwd(shape, device):
    n, s, w, epi = shape
    c = Ctx(device)
    e, b, head = _dt_inputs(c, n, s, w)
    image, weights, reg_q = c.OUT('image', F32, n * w), c.OUT('weights', F32, n * s), c.OUT('reg_q', F32, n * s)
    if epi:
        hm, am, reg = c.OUT('height_map', F32, n), c.OUT('absorption_map', F32, n), c.OUT('regularization', F32, n * s)
    else:
        hm, am, reg = (c.NULL(k, OUT) for k in ('height_map', 'absorption_map', 'regularization'))

    def expected():
        from sunerf_hip import ops
        out = ops.dt_integral_fwd(*_dt_wrapper_args(b, e, n, s, w), want_epilogues=bool(epi))
        return {k: out[k] for k in ('image', 'weights', 'reg_q') + (('height_map', 'absorption_map', 'regularization') if epi else ())}
    return Case('sunerf_dt_integral_fwd', shape, c.arena, head + [image, weights, reg_q, hm, am, reg, STREAM], expected, empty={14: 0})


def _dt_bwd(name, shape, device, full):
    n, s, w, with_reg = shape
    c = Ctx(device)
    e, b, head = _dt_inputs(c, n, s, w)
    gen = _gen(n * 31 + s)
    g_image = c.IN('g_image', e['g_image'].float())
    names = ('g_reg', 'g_weights', 'g_reg_q') if full else ('g_reg',)
    per_sample = [c.IN(k, 0.5 - _rand(gen, n, s)) if with_reg else c.NULL(k, IN) for k in names]
    g_raw, g_la, g_vc, absmax = c.OUT('g_raw', F32, n * s * 2), c.OUT('g_log_abs', F32, 7), c.OUT('g_vol_c', F32, 1), c.OUT('g_absmax', I32, 1)

    def expected():
        from sunerf_hip import ops
        fn = ops.dt_integral_bwd_full if full else ops.dt_integral_bwd
        g, la, vc, am = fn(*_dt_wrapper_args(b, e, n, s, w), g_image.t.view(n, w), *[p.t.view(n, s) if with_reg else None for p in per_sample])
        return {'g_raw': g, 'g_log_abs': la, 'g_vol_c': vc, 'g_absmax': am}
    def tolerance(key, got, want):
        """g_log_abs / g_vol_c are added with float atomics, one set per workgroup: the bound of the kernel's own test."""
        import test_gpu_dt_integral as dt
        if key in ('g_log_abs', 'g_vol_c'):
            ref = want.detach().cpu().double()
            assert dt.scalar_rel(got, ref, ref.reshape(-1) == 0) <= dt.SCALAR_GRADIENT_REL, key
        else:
            assert torch.equal(got.reshape(-1).view(I32), want.reshape(-1).view(I32)), key

    # header: an empty batch clears the three scalar outputs
    effect = lambda: {'g_log_abs': torch.zeros(7), 'g_vol_c': torch.zeros(1), 'g_absmax': torch.zeros(1, dtype=I32)}          # noqa: E731
    return Case(name, shape, c.arena, head + [g_image, *per_sample, g_raw, g_la, g_vc, absmax, STREAM], expected, empty={14: 0},
                empty_effect=effect, reproducible=n <= DT_ORDERED_RAYS, tolerance=tolerance)


@case('sunerf_dt_integral_bwd', DT_SHAPES, 'dt_sweep.h DT_THREADS 256: one wave per ray, 64 samples per pass')
def dt_integral_bwd(shape, device):
    return _dt_bwd('sunerf_dt_integral_bwd', shape, device, False)


@case('sunerf_dt_integral_bwd_full', DT_SHAPES, 'dt_sweep.h DT_THREADS 256: one wave per ray, 64 samples per pass')
def dt_integral_bwd_full(shape, device):
    return _dt_bwd('sunerf_dt_integral_bwd_full', shape, device, True)


@case('sunerf_thomson_integral_fwd', [(n, s, ch) for n, s in RAY_SHAPES for ch in (1, 2)],
      'thomson.hip TH_THREADS 256: one wave per ray, 64 samples per pass')
def thomson_integral_fwd(shape, device):
    from test_gpu_thomson import make_case
    n, s, ch = shape
    c = Ctx(device)
    raw_t, z_t, o_t, d_t, kappa = make_case(n, s, ch, 1000 * n + s)
    raw, z, o, d = c.IN('raw', raw_t), c.IN('z_vals', z_t), c.IN('rays_o', o_t), c.IN('rays_d', d_t)
    consts = [c.IN(k, torch.tensor([v], dtype=F32)) for k, v in (('solar_radius', 1.0), ('limb_darkening_coeff', 0.63), ('c0', 1.0))]
    outs = [c.OUT('pixel_b', F32, n * 2), c.OUT('pixel_density', F32, n), c.OUT('distance_from_sun', F32, n),
            c.OUT('distance_from_obs', F32, n), c.OUT('weights', F32, n * s)]

    def expected():
        from sunerf_hip import ops
        r = ops.thomson_integral_fwd(raw.t.view(n, s, ch), z.t.view(n, s), o.t.view(n, 3), d.t.view(n, 3), [k.t for k in consts], kappa)
        return {'pixel_b': r['pixel_B'], **{k: r[k] for k in ('pixel_density', 'distance_from_sun', 'distance_from_obs', 'weights')}}
    return Case('sunerf_thomson_integral_fwd', shape, c.arena, [raw, ch, float(kappa), z, o, d, *consts, n, s, *outs, STREAM], expected,
                empty={9: 0})


@case('sunerf_thomson_integral_bwd', [(n, s, ch, full) for n, s in RAY_SHAPES for ch, full in ((1, 1), (2, 0))],
      'thomson.hip TH_THREADS 256: one wave per ray, 64 samples per pass')
def thomson_integral_bwd(shape, device):
    from test_gpu_thomson import make_case
    n, s, ch, full = shape
    c = Ctx(device)
    raw_t, z_t, o_t, d_t, kappa = make_case(n, s, ch, 1000 * n + s)
    gen = _gen(n * 13 + s)
    raw, z, o, d = c.IN('raw', raw_t), c.IN('z_vals', z_t), c.IN('rays_o', o_t), c.IN('rays_d', d_t)
    consts = [c.IN(k, torch.tensor([v], dtype=F32)) for k, v in (('solar_radius', 1.0), ('limb_darkening_coeff', 0.63), ('c0', 1.0))]
    g_b = c.IN('g_pixel_b', 0.5 - _rand(gen, n, 2))
    if full:
        g_den, g_sun, g_obs = (c.IN(k, 0.5 - _rand(gen, n)) for k in ('g_pixel_density', 'g_distance_from_sun', 'g_distance_from_obs'))
        g_w = c.IN('g_weights', 0.5 - _rand(gen, n, s))
        absmax = c.OUT('g_absmax', I32, 1)
    else:
        g_den, g_sun, g_obs, g_w = (c.NULL(k, IN) for k in ('g_pixel_density', 'g_distance_from_sun', 'g_distance_from_obs', 'g_weights'))
        absmax = c.NULL('g_absmax', OUT)                  # header: may be NULL
    g_raw = c.OUT('g_raw', F32, n * s * ch)

    def expected():
        from sunerf_hip import ops
        v = lambda b, *sh: b.t.view(*sh) if full else None          # noqa: E731
        g, am = ops.thomson_integral_bwd(raw.t.view(n, s, ch), z.t.view(n, s), o.t.view(n, 3), d.t.view(n, 3), [k.t for k in consts], kappa,
                                         g_b.t.view(n, 2), v(g_den, n), v(g_sun, n), v(g_obs, n), v(g_w, n, s))
        return {'g_raw': g, 'g_absmax': am} if full else {'g_raw': g}
    return Case('sunerf_thomson_integral_bwd', shape, c.arena,
                [raw, ch, float(kappa), z, o, d, *consts, n, s, g_b, g_den, g_sun, g_obs, g_w, g_raw, absmax, STREAM], expected, empty={9: 0},
                empty_effect=lambda: {'g_absmax': torch.zeros(1, dtype=I32)} if full else {})      # header: an empty batch clears the word


@case('sunerf_dem_integral', [(n, s, k, mode) for n, s in RAY_SHAPES_S2 for k, mode in ((2, 0), (33, 1), (128, 2))],
      'dem.hip DEM_THREADS 256: one wave per ray, 64 samples per pass, K <= 128 nodes as two per lane')
def dem_integral(shape, device):
    import dem_reference as dr
    n, s, k, mode = shape                 # mode 0: em only, no mask, thin; 1: every output, mask; 2: every output, absorption
    c = Ctx(device)
    e = dr.make_case(n, s, dr.grid_nodes(k), 1000 * n + s)
    masked = mode == 1
    if masked:
        e = dr.add_mask(e)
    r_in, r_out = e.get('r_range', (0.0, math.inf))
    raw, z, nodes = c.IN('raw', e['raw']), c.IN('z_vals', e['z']), c.IN('logt_nodes', e['nodes'])
    o, d = (c.IN('rays_o', e['o']), c.IN('rays_d', e['d'])) if masked else (c.NULL('rays_o', IN), c.NULL('rays_d', IN))
    la_value = dr.log_abs_of(e, 'thick') if mode == 2 and e['tau1'] > 0 else None
    la = c.IN('log_abs', torch.tensor([la_value], dtype=F32)) if la_value is not None else c.NULL('log_abs', IN)
    em = c.OUT('em', F32, n)
    if mode:
        dem, mean, col = c.OUT('dem', F32, n * k), c.OUT('logt_mean', F32, n), c.OUT('column', F32, n)
    else:
        dem, mean, col = c.NULL('dem', OUT), c.NULL('logt_mean', OUT), c.NULL('column', OUT)

    def expected():
        from sunerf_hip import dem as dem_mod
        want = ('dem', 'em', 'logt_mean', 'column') if mode else ('em',)
        return dem_mod.dem_integral(raw.t.view(n, s, 2), z.t.view(n, s), nodes.t, base=dr.BASE, log_abs=la.t if la_value is not None else None,
                                    rays_o=o.t.view(n, 3) if masked else None, rays_d=d.t.view(n, 3) if masked else None,
                                    r_range=(r_in, r_out), want=want)
    return Case('sunerf_dem_integral', shape, c.arena,
                [raw, z, o, d, nodes, k, dr.BASE[0], dr.BASE[1], la, float(r_in), float(r_out), n, s, dem, em, mean, col, STREAM], expected,
                empty={11: 0})


@case('sunerf_column_stats', [(n, s, p) for n, s in RAY_SHAPES_S2 for p in (0, 1)], 'columns.hip CS_THREADS 256: one wave per column, four per workgroup')
def column_stats(shape, device):
    n, s, profiles = shape
    c = Ctx(device)
    e = _emission_case(n, s)
    raw, z_row, d = c.IN('raw', e['raw'].clamp(-20., 20.)), c.IN('z_row', e['z'][0]), c.IN('rays_d', e['d'])
    height, column = c.OUT('emission_height', F32, n), c.OUT('emission_column', F32, n)
    if profiles:
        em, ab = c.OUT('emission', F32, n * s), c.OUT('absorption', F32, n * s)
    else:
        em, ab = c.NULL('emission', OUT), c.NULL('absorption', OUT)

    def expected():
        from sunerf_hip import maps
        return maps.column_stats(raw.t.view(n, s, 2), z_row.t, d.t.view(n, 3), height_scale=1.5, profiles=bool(profiles))
    return Case('sunerf_column_stats', shape, c.arena, [raw, z_row, d, n, s, 1.5, height, column, em, ab, STREAM], expected, empty={3: 0})


# ---- analytic and tabulated fields ----------------------------------------------------------------------------------------------
STAR = dict(rho_0=2.0e8, h0=0.12, T0=1.3e6, Rs=1.1, t_photosphere=5777.0)


def _star_rays(c, n, s):
    e = _dt_case(n, s, 1)
    return c.IN('rays_o', e['o']), c.IN('rays_d', e['d']), c.IN('z_vals', e['z'])


@case('sunerf_simple_star_field', RAY_SHAPES, 'dt.hip DT_THREADS 256: one sample per thread')
def simple_star_field(shape, device):
    n, s = shape
    c = Ctx(device)
    o, d, z = _star_rays(c, n, s)
    raw = c.OUT('raw', F32, n * s * 2)

    def expected():
        from sunerf_hip import ops
        return {'raw': ops.simple_star_field(o.t.view(n, 3), d.t.view(n, 3), z.t.view(n, s), **STAR)}
    return Case('sunerf_simple_star_field', shape, c.arena,
                [o, d, z, n, s, STAR['rho_0'], STAR['h0'], STAR['T0'], STAR['Rs'], STAR['t_photosphere'], raw, STREAM], expected, empty={3: 0})


def _star_params(c):
    return c.IN('params', torch.tensor([STAR['Rs'], STAR['h0'], STAR['T0'], STAR['rho_0']], dtype=F32))


@case('sunerf_simple_star_field_dev', RAY_SHAPES, 'dt.hip DT_THREADS 256: one sample per thread')
def simple_star_field_dev(shape, device):
    n, s = shape
    c = Ctx(device)
    o, d, z = _star_rays(c, n, s)
    params, raw = _star_params(c), c.OUT('raw', F32, n * s * 2)

    def expected():
        from sunerf_hip import ops
        return {'raw': ops.simple_star_field_dev(o.t.view(n, 3), d.t.view(n, 3), z.t.view(n, s), params.t, STAR['t_photosphere'])}
    return Case('sunerf_simple_star_field_dev', shape, c.arena, [o, d, z, n, s, params, STAR['t_photosphere'], raw, STREAM], expected, empty={3: 0})


@case('sunerf_simple_star_bwd', [(n, s, acc) for n, s in RAY_SHAPES for acc in (0, 1)],
      'dt.hip STAR_BWD_THREADS 256: per-workgroup fp64 partials in the workspace, a second launch adds them')
def simple_star_bwd(shape, device):
    n, s, acc = shape
    c = Ctx(device)
    o, d, z = _star_rays(c, n, s)
    params = _star_params(c)
    g_raw = c.IN('g_raw', 0.5 - _rand(_gen(n * 5 + s), n, s, 2))
    nbytes = int(_lib().sunerf_simple_star_bwd_workspace_bytes())
    ws = c.WS('workspace', nbytes)
    g_params = c.INOUT('g_params', torch.tensor([0.5, -1.0, 2.0, 4.0])) if acc else c.OUT('g_params', F32, 4)

    def expected():
        from sunerf_hip import ops
        out = torch.tensor([0.5, -1.0, 2.0, 4.0], device=c.device) if acc else None
        return {'g_params': ops.simple_star_bwd(o.t.view(n, 3), d.t.view(n, 3), z.t.view(n, s), params.t, STAR['t_photosphere'],
                                                g_raw.t.view(n, s, 2), out=out)}
    return Case('sunerf_simple_star_bwd', shape, c.arena,
                [o, d, z, n, s, params, STAR['t_photosphere'], g_raw, ws, nbytes, g_params, acc, STREAM], expected, ws_index=9,
                empty={3: 0}, empty_effect=lambda: {} if acc else {'g_params': torch.zeros(4)})      # header: no rays, a zero gradient


# ---- rays, grids and element-wise volumes ---------------------------------------------------------------------------------------
def _pose():
    from sunerf_hip.rays import pose_spherical
    return pose_spherical(-0.3, 0.1, 215.032)


def _c2w_host(c2w):
    return HostValue((ctypes.c_float * 12)(*[float(v) for v in c2w[:3, :4].reshape(-1).tolist()]))


@case('sunerf_observer_rays', [(n, pp, t) for n in (1, 255, 257, 769 + 5) for pp, t in ((0, 1), (1, 0))],
      'rays.hip: 256-thread blocks, one pixel per thread')
def observer_rays(shape, device):
    n_pix, per_pixel, with_times = shape
    c = Ctx(device)
    width, height, begin = 37, 23, 3                      # a frame of 851 pixels; the tile starts inside its first row
    assert begin + n_pix <= width * height
    ax, ay = torch.linspace(-5e-3, 5e-3, width, dtype=F64), torch.linspace(-4e-3, 4e-3, height, dtype=F64)
    if per_pixel:
        tx_t, ty_t = ax[None, :].expand(height, width).contiguous(), ay[:, None].expand(height, width).contiguous()
    else:
        tx_t, ty_t = ax, ay
    tx, ty = c.IN('tx', tx_t), c.IN('ty', ty_t)
    c2w = _pose()
    ro, rd = c.OUT('rays_o', F32, n_pix * 3), c.OUT('rays_d', F32, n_pix * 3)
    times = c.OUT('times', F32, n_pix) if with_times else c.NULL('times', OUT)

    def expected():
        from sunerf_hip import rays
        sh = (height, width) if per_pixel else (-1,)
        out = rays.grid_rays(tx.t.view(*sh), ty.t.view(*sh), c2w, begin, n_pix, time=0.25 if with_times else None)
        return dict(zip(('rays_o', 'rays_d', 'times'), out))
    return Case('sunerf_observer_rays', shape, c.arena,
                [tx, ty, per_pixel, width, begin, n_pix, _c2w_host(c2w), 0.25, ro, rd, times, STREAM], expected, empty={5: 0})


@case('sunerf_column_rays', [(n, pc, t) for n in (1, 255, 257, 769 + 5) for pc, t in ((0, 1), (1, 0))],
      'columns.hip: 256-thread blocks, one column per thread')
def column_rays(shape, device):
    n_cols, per_column, with_times = shape
    c = Ctx(device)
    n_lat, n_lon, begin = 23, 37, 3
    assert begin + n_cols <= n_lat * n_lon
    lat_t, lon_t = torch.linspace(-1.4, 1.4, n_lat, dtype=F64), torch.linspace(-math.pi, math.pi, n_lon, dtype=F64)
    if per_column:
        lat_t, lon_t = lat_t[:, None].expand(n_lat, n_lon).reshape(-1).contiguous(), lon_t[None, :].expand(n_lat, n_lon).reshape(-1).contiguous()
    lat, lon = c.IN('lat', lat_t), c.IN('lon', lon_t)
    ro, rd = c.OUT('rays_o', F32, n_cols * 3), c.OUT('rays_d', F32, n_cols * 3)
    times = c.OUT('times', F32, n_cols) if with_times else c.NULL('times', OUT)

    def expected():
        from sunerf_hip import maps
        out = maps.column_rays(lat.t, lon.t, grid=not per_column, col_begin=begin, n_cols=n_cols, time=0.25 if with_times else None)
        return dict(zip(('rays_o', 'rays_d', 'times'), out))
    return Case('sunerf_column_rays', shape, c.arena,
                [lat, lon, per_column, 1 if per_column else n_lon, begin, n_cols, 0.25, ro, rd, times, STREAM], expected, empty={5: 0})


def _volume_grid(kind):
    from sunerf_hip.volume import CartesianGrid, SphericalGrid
    if kind == 'affine':
        return CartesianGrid(np.linspace(-1.3, 1.3, 9), np.linspace(-1.2, 1.2, 11), np.linspace(-1.1, 1.4, 13), origin=(0.1, -0.2, 0.05),
                             basis=[[1.0, 0.1, 0.0], [0.0, 0.9, 0.2], [0.1, 0.0, 1.1]])
    return SphericalGrid(np.linspace(-1.2, 1.2, 9), np.linspace(-3.0, 3.0, 11), np.linspace(1.0, 2.0, 13))


@case('sunerf_grid_points', [(count, kind, off) for count in (1, 255, 257, 769 + 5) for kind, off in (('affine', 0), ('spherical', 1))],
      'volume.hip: 256-thread blocks, one voxel per thread; `radius` offset by one element (4-byte aligned only)')
def grid_points(shape, device):
    from sunerf_hip import volume
    count, kind, off = shape
    c = Ctx(device)
    grid = _volume_grid(kind)
    first = 7                                              # an odd first voxel
    assert first + count <= grid.n_voxels
    axes = [c.IN(f'a{k}', a) for k, a in enumerate(grid._kernel_axes())]
    # points are 16-byte aligned by the header; radius is a plain fp32 vector: offset by one element
    points, radius = c.OUT('points', F32, count * 4), c.OUT('radius', F32, count, offset=off)
    n0, n1, n2 = grid._shape3

    def expected():
        p, r = volume.grid_points(grid, Rs_per_ds=1.5, time=0.25, first=first, count=count, device=c.device)
        return {'points': p, 'radius': r}
    return Case('sunerf_grid_points', shape, c.arena,
                [0 if kind == 'affine' else 1, *axes, n0, n1, n2, HostValue(volume._frame(grid)), 1.5, 0.25, first, count, points, radius, STREAM],
                expected, empty={11: 0})


FQ_SHAPES = [(m, kind, w, off) for m in (1, 511, 513, 1025) for kind, w in (('emission', 0), ('dt', 1), ('dt', 7), ('white_light', 0))
             for off in (0, 1)]


@case('sunerf_field_quantities', FQ_SHAPES,
      'volume.hip FQ_CHUNK 512 = 2 x FQ_THREADS 256: two voxels per thread, 16-byte I/O; offset 1: every payload starts one voxel '
      'late, so that the scalar path (vec_io / vec_w false) runs')
def field_quantities(shape, device):
    from sunerf_hip import volume
    from test_gpu_volume import _radii
    m, kind, w, off = shape
    c = Ctx(device)
    gen = _gen(21 + m)
    ch = 1 if kind == 'white_light' else 2
    inf_t = torch.stack([_rand(gen, m) * 30 - 20, _rand(gen, m) * 6 - 3], -1)[:, :ch].float().contiguous()
    if kind == 'dt':
        inf_t = torch.stack([_rand(gen, m) * 3, 5.5 + 2 * _rand(gen, m)], -1).float().contiguous()
    rad_t = _radii(max(m, 6), gen)[:m]
    rad_t = torch.nan_to_num(rad_t, nan=0.5)
    inf, rad = c.IN('inferences', inf_t, offset=off * ch), c.IN('radius', rad_t, offset=off)
    lt, resp = _dt_tables()
    if w:
        wl = c.IN('wavelengths', torch.tensor([94., 131., 171., 193., 211., 304., 1600.])[:w] if w > 1 else torch.tensor([171.]))
        tl, tr, la = c.IN('table_logt', lt), c.IN('table_resp', resp), c.IN('log_abs', torch.linspace(-0.1, 0.5, 7))
        emis, absw = c.OUT('emissivity', F32, m * w, offset=off * w), c.OUT('absorption_w', F32, m * w, offset=off * w)
    else:
        wl, tl, tr, la = (c.NULL(k, IN) for k in ('wavelengths', 'table_logt', 'table_resp', 'log_abs'))
        emis, absw = c.NULL('emissivity', OUT), c.NULL('absorption_w', OUT)
    out0 = c.OUT('out0', F32, m, offset=off)
    out1 = c.NULL('out1', OUT) if kind == 'white_light' else c.OUT('out1', F32, m, offset=off)
    names = {'emission': ('emission', 'absorption'), 'dt': ('density', 'log_temperature'), 'white_light': ('electron_density',)}[kind]

    def expected():
        q = names + (('emissivity', 'absorption') if w else ())
        r = volume.field_quantities(inf.t.view(m, ch), rad.t, kind, quantities=q, r_range=(1.0, 1.3), fill=-1.0, kappa=2.0,
                                    wavelengths=wl.t if w else None, response_table=(tl.t.view(7, 101), tr.t.view(7, 101)) if w else None,
                                    log_abs=la.t if w else None)
        out = {'out0': r[names[0]]}
        if len(names) > 1:
            out['out1'] = r[names[1]]
        if w:
            out.update(emissivity=r['emissivity'], absorption_w=r['absorption'])
        return out
    return Case('sunerf_field_quantities', shape, c.arena,
                [volume._MODES[kind], inf, ch, rad, m, 1.0, 1.3, -1.0, 2.0, wl, w, tl, tr, la, out0, out1, emis, absw, STREAM], expected,
                empty={4: 0})


@case('sunerf_volume_metrics', [(1, 1, 1), (3, 5, 17), (7, 73, 1), (5, 7, 37), (9, 11, 13)],
      'volume.hip VM_THREADS 256: per-workgroup fp64 partial sums in the workspace, a second launch adds them (255, 511, 1295, 1287 voxels)')
def volume_metrics(shape, device):
    from sunerf_hip import volume
    n0, n1, n2 = shape
    c = Ctx(device)
    gen = _gen(31 + n0 * n1 * n2)
    m = n0 * n1 * n2
    a, b = c.IN('a', torch.randn(m, generator=gen)), c.IN('b', torch.randn(m, generator=gen))
    ws3 = [c.IN(f'w{k}', 0.5 + _rand(gen, n).double()) for k, n in enumerate(shape)]
    out = c.OUT('out', F64, 11)
    nbytes = int(_lib().sunerf_volume_metrics_workspace_bytes(m))
    ws = c.WS('workspace', nbytes)

    def expected():
        r = volume.volume_metrics(a.t.view(n0, n1, n2), b.t.view(n0, n1, n2), weights=[w.t for w in ws3])
        return {'out': torch.tensor([r[f'sum_{k}'] for k in volume.SUM_NAMES[:9]] + [r['max_abs'], float(r['count'])], dtype=F64)}
    return Case('sunerf_volume_metrics', shape, c.arena, [a, b, n0, n1, n2, *ws3, out, ws, nbytes, STREAM], expected, ws_index=10,
                rejections=[({2: 0}, -1)])          # header: an axis without nodes is SUNERF_E_BADARG


# ---- scoring and inversion ------------------------------------------------------------------------------------------------------
@case('sunerf_image_metrics', [(n, h, w) for n in (1, 3) for h in (7, 15, 17) for w in (7, 63, 65)] + [(1, 37, 133), (3, 37, 133)],
      'metrics.hip MT_THREADS 256: tiles of 64 x 16 pixels, window 7; one fp64 partial row per tile in the workspace')
def image_metrics(shape, device):
    from test_gpu_metrics import _inputs
    n, h, w = shape
    c = Ctx(device)
    pred_t, target_t = _inputs('noise', shape, 255, 7 * h + w)
    pred, target = c.IN('pred', pred_t), c.IN('target', target_t)
    out = c.OUT('out', F64, n * 4)
    nbytes = int(_lib().sunerf_image_metrics_workspace_bytes(n, h, w))
    ws = c.WS('workspace', nbytes)

    def expected():
        from sunerf_hip import metrics
        r = metrics.image_metrics(pred.t.view(n, h, w), target.t.view(n, h, w), 255.0)
        return {'out': torch.stack([r['ssim'], r['mse'], r['mae'], r['me']], -1)}
    return Case('sunerf_image_metrics', shape, c.arena, [pred, target, n, h, w, 255.0, out, ws, nbytes, STREAM], expected, ws_index=8,
                empty={2: 0})


# every (N, K, M) of the tiles' neighbours, the three modes taken in turn, and three blocks with a ragged end in every mode
INVERT_SHAPES = [(n, k, m, (i + j + l) % 3) for i, n in enumerate((1, 63, 65, 257)) for j, k in enumerate((2, 31, 33, 128))
                 for l, m in enumerate((1, 6, 8))] + [(517, 33, 8, mode) for mode in (0, 1, 2)]


@functools.lru_cache(maxsize=None)
def _invert_case(n, k, m):
    import dem_inversion_reference as ref
    from conftest import load_golden
    return ref.make_cases(load_golden('g6_dt_e2e'), n, n_channels=m, n_nodes=k, seed=n + k)


@case('sunerf_dem_invert', INVERT_SHAPES,
      'dem_inversion.hip INV_THREADS 256: one pixel per lane, 64-pixel waves stage 64 x 32 nodes in LDS per flush; mode 0: fixed '
      'lam [1], every output; 1: lam per pixel, dem NULL; 2: discrepancy')
def dem_invert(shape, device):
    n, k, m, mode = shape
    c = Ctx(device)
    e = _invert_case(n, k, m)
    y, sigma = c.IN('y', torch.from_numpy(e['y']).float()), c.IN('sigma', torch.from_numpy(e['sigma']).float())
    G, prior = c.IN('response', torch.from_numpy(e['G'])), c.IN('prior', torch.from_numpy(e['prior']))
    nodes = c.IN('logt_nodes', torch.from_numpy(e['nodes']).float())
    gen = _gen(n + k + m)
    if mode == 0:
        lam = c.IN('lam', torch.tensor([1.0]))
    elif mode == 1:
        lam = c.IN('lam', 10.0 ** (2 * _rand(gen, n) - 1))
    else:
        lam = c.NULL('lam', IN)
    dem = c.NULL('dem', OUT) if mode == 1 else c.OUT('dem', F32, n * k)
    em, mean, chi2, lam_out = (c.OUT(name, F32, n) for name in ('em', 'logt_mean', 'chi2', 'lam_out'))
    status = c.OUT('status', I32, n)
    n_bisect, tol, max_iter = 6, 1e-10, 64

    def expected():
        from sunerf_hip import dem_inversion as inv
        want = tuple(q for q in inv.OUTPUTS if not (mode == 1 and q == 'dem'))
        r = inv.invert_dem(y.t.view(n, m), G.t.view(m, k), nodes.t, errors=sigma.t.view(n, m), prior=prior.t,
                           lam=None if mode == 2 else (1.0 if mode == 0 else lam.t), n_bisect=n_bisect, tol=tol, max_iter=max_iter, want=want)
        out = {'em': r['em'], 'logt_mean': r['logt_mean'], 'chi2': r['chi2'], 'lam_out': r['lam'], 'status': r['status']}
        if mode != 1:
            out['dem'] = r['dem']
        return out
    return Case('sunerf_dem_invert', shape, c.arena,
                [y, sigma, G, prior, nodes, lam, int(mode == 1), int(mode == 2), -1.0, 1e-4, 1e4, n_bisect, tol, max_iter, n, m, k,
                 dem, em, mean, chi2, lam_out, status, STREAM], expected, empty={14: 0})


@case('sunerf_map_fill', [(ch, n, mode) for ch, n in ((1, 1), (1, 255), (3, 257), (2, 769 + 5)) for mode in (0, 1, 2)],
      'reprojection.hip: 256-thread workgroups, per-workgroup fp64 partial sums in the workspace')
def map_fill(shape, device):
    ch, n, mode = shape
    c = Ctx(device)
    gen = _gen(ch * 1000 + n)
    data = torch.randn(ch, 1, n, generator=gen)
    data[_rand(gen, ch, 1, n) < 0.3] = float('nan')
    image = c.INOUT('map', data)
    stats = c.OUT('stats', F64, ch * 2)
    nbytes = int(_lib().sunerf_map_fill_workspace_bytes(ch))
    ws = c.WS('workspace', nbytes)

    def expected():
        from sunerf_hip import reprojection
        img = data.to(c.device)
        st = reprojection.fill_map(img, {0: None, 1: 'mean', 2: 0.75}[mode])
        return {'map': img, 'stats': st}
    return Case('sunerf_map_fill', shape, c.arena, [image, ch, n, mode, 0.75 if mode == 2 else 0.0, stats, ws, nbytes, STREAM], expected,
                ws_index=7, rejections=[({2: 0}, -1)])          # header: non-positive shapes are SUNERF_E_BADARG


# ---- the training step ----------------------------------------------------------------------------------------------------------
def _train_ws(c):
    # header: ZERO-INITIALISED once by the caller, the kernels leave it zeroed -> init='zero' (never given a pattern)
    nbytes = int(_lib().sunerf_train_workspace_bytes())
    return c.WS('workspace', nbytes, init='zero'), nbytes


@case('sunerf_training_loss', [(n, w, reg, sc) for n, w in ((1, 1), (255, 1), (257, 1), (37, 7), (3 * 128 * 256 // 7 + 1, 7)) for reg, sc in ((0, 0), (1, 1))],
      'train_step.hip TS_THREADS 256 x TS_BLOCKS 128: grid-stride partial sums in the workspace')
def training_loss(shape, device):
    n_rays, w, with_reg, scaling = shape
    c = Ctx(device)
    gen = _gen(n_rays * 3 + w)
    n = n_rays * w
    coarse, fine, target = (c.IN(k, _rand(gen, n)) for k in ('coarse_image', 'fine_image', 'target_image'))
    n_reg = n_rays * 5 if with_reg else 0
    reg = c.IN('regularization', _rand(gen, n_reg)) if with_reg else c.NULL('regularization', IN)
    extra = [c.IN('finite_check0', _rand(gen, n_rays * 5)), c.IN('finite_check1', _rand(gen, 3))] if with_reg else []
    sizes = HostValue((ctypes.c_int64 * max(1, len(extra)))(*[b.numel for b in extra]))
    g_coarse, g_fine, stats = c.OUT('g_coarse', F32, n), c.OUT('g_fine', F32, n), c.OUT('stats', F32, 8)
    ws, nbytes = _train_ws(c)

    def expected():
        from sunerf_hip import train
        co, fi = coarse.plain(n_rays, w).requires_grad_(True), fine.plain(n_rays, w).requires_grad_(True)
        loss, st = train.training_loss(co, fi, target.t.view(n_rays, w), reg.t if with_reg else None, 1.0, 0.5,
                                       asinh_scaling=(1.0, 0.005) if scaling else None, finite_check=[b.t for b in extra])
        loss.backward()
        return {'g_coarse': co.grad, 'g_fine': fi.grad, 'stats': st.detach()}
    return Case('sunerf_training_loss', shape, c.arena,
                [coarse, fine, target, n, reg, n_reg, HostPtrs(extra), sizes, len(extra), scaling, 1.0, 0.005, 1.0, 0.5, g_coarse, g_fine, stats,
                 ws, nbytes, STREAM], expected, ws_index=18, rejections=[({3: 0}, -1)])          # header: n >= 1


@case('sunerf_clip_adam_step', [(n, clip) for n in (1, 255, 257, 128 * 256 + 1, 3 * 128 * 256 + 5) for clip in (0, 1)],
      'train_step.hip TS_THREADS 256 x TS_BLOCKS 128: the norm pass leaves partial sums in the workspace, the update is grid-stride')
def clip_adam_step(shape, device):
    n, clip = shape
    c = Ctx(device)
    gen = _gen(n)
    p0, g0 = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    m0, v0 = 0.1 * torch.randn(n, generator=gen), 0.01 * _rand(gen, n)
    params, grads, m, v = c.INOUT('params', p0), c.INOUT('grads', g0), c.INOUT('exp_avg', m0), c.INOUT('exp_avg_sq', v0)
    skip = c.IN('skip_if_positive', torch.zeros(1))
    norm = c.OUT('norm_out', F32, 4)
    counter = c.INOUT('step_counter', torch.tensor([3], dtype=I64))
    ws, nbytes = _train_ws(c)
    max_norm = 0.5 if clip else 0.0

    def expected():
        from sunerf_hip import train
        p = torch.nn.Parameter(p0.to(c.device))
        opt = train.ClipAdam([p], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_norm=max_norm if clip else None)
        opt.flat_grads.copy_(g0)
        opt.exp_avg.copy_(m0)
        opt.exp_avg_sq.copy_(v0)
        opt.applied_steps.fill_(3)
        opt.step()
        return {'params': opt.flat_params, 'grads': opt.flat_grads, 'exp_avg': opt.exp_avg, 'exp_avg_sq': opt.exp_avg_sq,
                'norm_out': opt.norm, 'step_counter': opt.applied_steps}
    return Case('sunerf_clip_adam_step', shape, c.arena,
                [params, grads, m, v, n, 1e-3, 0.9, 0.999, 1e-8, max_norm, 1.0, 0, skip, norm, ws, nbytes, counter, STREAM], expected,
                ws_index=15, empty={4: 0})


# ---- fields on grids and tables (descriptors) -----------------------------------------------------------------------------------
def _grid_descriptor(c, name, ch):
    """``SunerfGridFieldDesc`` of the grid ``name`` of tests/test_gpu_grid_field.py whose axis arrays are arena buffers."""
    from sunerf_hip import grid_field as gf
    from test_gpu_grid_field import FILL, make_grid
    grid = make_grid(name)
    desc = gf.GridDescriptor(grid, ch, 1.0, FILL[:ch], gf.longitude_mode(grid), 'cpu')
    axes = [c.IN(f'axis{k}', grid.axes[k]) for k in range(3)]
    for k in range(3):
        desc.record.axis[k] = axes[k].ptr.value
    desc.axes = tuple(a.t for a in axes)
    desc.device = c.device
    return grid, desc


def _grid_rays(name, n, s):
    from test_gpu_grid_field import GRIDS, make_rays
    o, d, z = make_rays(name, seed=100 + GRIDS.index(name), inside_only=name == 'cell')
    return o[:n].contiguous(), d[:n].contiguous(), z[:n, :s].contiguous()


GF_FWD_SHAPES = [(n, s, ch, mode, idx) for (n, s), ch in zip(((1, 1), (5, 51), (257, 1), (12, 67)), (1, 3, 4, 2))
                 for mode in ('rays', 'points3', 'points4') for idx in (0, 1)]


@case('sunerf_grid_field_fwd', GF_FWD_SHAPES, 'grid_field.hip GF_THREADS 256 (grid_gather.h): one sample per thread (1, 255, 257 and 804 samples)')
def grid_field_fwd(shape, device):
    n, s, ch, mode, want_index = shape
    c = Ctx(device)
    name = {1: 'nonuniform', 2: 'rotated', 3: 'sph_open', 4: 'sph_closed'}[ch]
    grid, desc = _grid_descriptor(c, name, ch)
    values = c.IN('values', torch.randn(*grid.shape, ch, generator=_gen(7 + ch)))
    o_t, d_t, z_t = _grid_rays(name, n, s)
    total = n * s
    if mode == 'rays':
        o, d, z = c.IN('rays_o', o_t), c.IN('rays_d', d_t), c.IN('z_vals', z_t)
        points, stride, n_rays, n_samples = c.NULL('points', IN), 0, n, s
    else:
        stride = int(mode[-1])
        p = (o_t[:, None, :] + d_t[:, None, :] * z_t[:, :, None]).reshape(-1, 3)
        p = torch.cat([p, torch.full((total, 1), 0.25)], 1)[:, :stride].contiguous()
        o, d, z = (c.NULL(k, IN) for k in ('rays_o', 'rays_d', 'z_vals'))
        points, n_rays, n_samples = c.IN('points', p), total, 1
    raw = c.OUT('raw', F32, total * ch)
    cells, weights = (c.OUT('cells', I32, total), c.OUT('weights', F32, total * 6)) if want_index else (c.NULL('cells', OUT), c.NULL('weights', OUT))

    def expected():
        from sunerf_hip import grid_field as gf
        v = values.t.view(*grid.shape, ch)
        if mode == 'rays':
            r = gf.grid_field_rays(desc, v, o.t.view(n, 3), d.t.view(n, 3), z.t.view(n, s), want_index=bool(want_index))
        else:
            r = gf.grid_field_points(desc, v, points.t.view(total, stride), want_index=bool(want_index))
        return {'raw': r[0], 'cells': r[1][0], 'weights': r[1][1]} if want_index else {'raw': r}
    return Case('sunerf_grid_field_fwd', shape, c.arena,
                [HostValue(desc.ref(), keep=desc), values, o, d, z, n_rays, n_samples, points, stride, raw, cells, weights, STREAM], expected,
                empty={5: 0})


@case('sunerf_grid_field_bwd', [(total, ch, acc) for total, ch in ((63, 1), (64, 3), (65, 4), (129, 2), (804, 3)) for acc in (0, 1)],
      'grid_gather.h GF_CHUNK 64: sorted positions per piece of a long segment; totals up to 129: every sample in the one cell of a '
      '2 x 2 x 2 grid (8 nodes: less than one block), so that the long-segment path and its `part` workspace run')
def grid_field_bwd(shape, device):
    total, ch, acc = shape
    c = Ctx(device)
    name = 'cell' if total <= 129 else 'sph_open'
    grid, desc = _grid_descriptor(c, name, ch)
    n, s = (-(-total // 67), 67) if name == 'cell' else (12, 67)
    o_t, d_t, z_t = _grid_rays(name, n, s)
    p = (o_t[:, None, :] + d_t[:, None, :] * z_t[:, :, None]).reshape(-1, 3)[:total].contiguous()
    gen = _gen(total + ch)
    n_nodes = grid.n_voxels
    g_raw = c.IN('g_raw', torch.randn(total, ch, generator=gen))
    if c.gpu:
        from sunerf_hip import grid_field as gf
        values = torch.zeros(*grid.shape, ch, device=c.device)
        _, (cells_t, weights_t) = gf.grid_field_points(desc, values, p.to(c.device), want_index=True)
        ids, perm_t = torch.sort(cells_t, stable=True)
        seg_t = torch.searchsorted(ids, torch.arange(desc.n_cells + 1, dtype=I32, device=c.device))
    else:
        cells_t, weights_t = torch.zeros(total, dtype=I32), torch.zeros(total, 6)
        perm_t, seg_t = torch.arange(total), torch.zeros(desc.n_cells + 1, dtype=I64)
    cells, weights = c.IN('cells', cells_t), c.IN('weights', weights_t)
    perm, seg = c.IN('perm', perm_t), c.IN('seg_start', seg_t)
    nbytes = int(_lib().sunerf_grid_field_bwd_workspace_bytes(total, ch))
    ws = c.WS('workspace', nbytes)
    g0 = torch.randn(n_nodes * ch, generator=gen)
    g_values = c.INOUT('g_values', g0) if acc else c.OUT('g_values', F32, n_nodes * ch)

    def expected():
        from sunerf_hip import grid_field as gf
        out = g0.to(c.device).view(*grid.shape, ch).clone() if acc else None
        return {'g_values': gf.grid_field_bwd(desc, g_raw.t.view(total, ch), (cells.t, weights.t.view(total, 6)), out=out, accumulate=bool(acc))}

    def empty_effect():          # header: n_total == 0 zeroes g_values unless accumulate
        return {} if acc else {'g_values': torch.zeros(n_nodes * ch)}
    return Case('sunerf_grid_field_bwd', shape, c.arena,
                [HostValue(desc.ref(), keep=desc), g_raw, cells, weights, perm, seg, total, ws, nbytes, g_values, acc, STREAM], expected,
                ws_index=8, empty={6: 0}, empty_effect=empty_effect)


def _mhd_tables(c):
    """Three resident frames (tests/test_gpu_mhd.py's) as a device table of ``SunerfMhdFrame`` whose node, axis and bucket arrays
    are arena buffers; ``slot`` maps frames 10..12 to them."""
    import mhd_reference as ref
    from sunerf_hip import ops
    frames = [ref.synthetic_frame(1), ref.synthetic_frame(2, n_phi=19, n_theta=21, n_r=33, r_range=(1.03, 1.35), phi_end=0.93 * 2 * np.pi),
              ref.synthetic_frame(3)]
    table = (ops.MhdFrame * len(frames))()
    for i, (r, th, phi, rho, temp) in enumerate(frames):
        data = torch.from_numpy(np.stack([rho, temp], -1)).float().clamp_min(1e-10)
        rec = table[i]
        rec.data = c.IN(f'frame{i}_data', data).ptr.value
        for k, ax in enumerate((phi, th, r)):
            ax = torch.from_numpy(np.asarray(ax)).float()
            bucket, inv_width = ops.mhd_bucket_table(ax)
            rec.axis[k] = c.IN(f'frame{i}_axis{k}', ax).ptr.value
            rec.bucket[k] = c.IN(f'frame{i}_bucket{k}', bucket).ptr.value
            rec.n[k], rec.nb[k] = ax.numel(), bucket.numel()
            rec.lo[k], rec.hi[k], rec.inv_width[k] = float(ax[0]), float(ax[-1]), inv_width
    raw_bytes = torch.frombuffer(bytearray(bytes(table)), dtype=U8).clone()
    return c.IN('frames', raw_bytes), c.IN('slot', torch.tensor([0, 1, 2], dtype=I32)), 10, 12


def _mhd_points(m):
    from test_gpu_mhd import _points
    return _points(m, 11 + m, (0.0, 0.25, 0.5, 0.8, 1.0))


@case('sunerf_mhd_field_points', [1, 255, 257, 769 + 5], 'mhd.hip MHD_THREADS 256: one point per thread, a point read as one 16-byte load')
def mhd_field_points(shape, device):
    m = shape
    c = Ctx(device)
    frames, slot, ffirst, flast = _mhd_tables(c)
    points = c.IN('points', _mhd_points(m))
    raw = c.OUT('raw', F32, m * 2)
    status = c.INOUT('status', torch.zeros(1, dtype=I32))          # header: only ever written 1; the caller zeroes it

    def expected():
        from sunerf_hip import ops
        return {'raw': ops.mhd_field_points(points.t.view(m, 4), frames.t, slot.t, ffirst, flast), 'status': torch.zeros(1, dtype=I32)}
    return Case('sunerf_mhd_field_points', shape, c.arena, [points, m, frames, slot, ffirst, flast, raw, status, STREAM], expected, empty={1: 0})


@case('sunerf_mhd_field', RAY_SHAPES, 'mhd.hip MHD_THREADS 256: one sample per thread')
def mhd_field(shape, device):
    n, s = shape
    c = Ctx(device)
    frames, slot, ffirst, flast = _mhd_tables(c)
    p = _mhd_points(n)
    gen = _gen(n + s)
    o, d = c.IN('rays_o', p[:, :3]), c.IN('rays_d', 0.05 * torch.randn(n, 3, generator=gen))
    z, times = c.IN('z_vals', _rand(gen, n, s).sort(1).values), c.IN('times', p[:, 3])
    raw = c.OUT('raw', F32, n * s * 2)
    status = c.INOUT('status', torch.zeros(1, dtype=I32))

    def expected():
        from sunerf_hip import ops
        return {'raw': ops.mhd_field(o.t.view(n, 3), d.t.view(n, 3), z.t.view(n, s), times.t.view(n, 1), frames.t, slot.t, ffirst, flast),
                'status': torch.zeros(1, dtype=I32)}
    return Case('sunerf_mhd_field', shape, c.arena, [o, d, z, times, n, s, frames, slot, ffirst, flast, raw, status, STREAM], expected,
                empty={4: 0})


# ---- observations and the reprojection baseline ---------------------------------------------------------------------------------
WL7 = [94., 131., 171., 193., 211., 304., 335.]


def _views(c, n_channels, shapes):
    """Views on the disk centre whose images and axes are arena buffers: ``shapes`` = [(height, width, downscale, absent)],
    ``absent`` channels of the ``n_channels`` missing from that view."""
    from sunerf_hip import observations as obs
    from sunerf_hip.rays import pose_spherical
    rng = np.random.default_rng(5 + n_channels)
    views = []
    for i, (h, w, f, absent) in enumerate(shapes):
        wl = np.array((WL7 * 3)[:n_channels], dtype=np.float32)
        wl[list(absent)] = 0.0
        n_planes = int((wl != 0).sum())
        planes = (rng.uniform(0.0, 2.0, size=(n_planes, h * f, w * f)) * 10.0 ** rng.integers(-3, 4, size=(n_planes, h * f, w * f))).astype(np.float32)
        lat, lon, dist = 0.1 - 0.2 * i, 0.3 + 0.4 * i, 215.0 - 10 * i
        tx = c.IN(f'view{i}_tx', torch.linspace(-6e-3, 6e-3, w, dtype=F64) if w > 1 else torch.zeros(1, dtype=F64))
        ty = c.IN(f'view{i}_ty', torch.linspace(-5e-3, 5e-3, h, dtype=F64) if h > 1 else torch.zeros(1, dtype=F64))
        image = c.IN(f'view{i}_image', planes)
        plane, wavelength = obs.channel_map(wl, n_planes)
        views.append(obs.View(image.t.view(n_planes, h * f, w * f), tx.t, ty.t, pose_spherical(-lon, lat, dist), 0.25 * i, plane, wavelength,
                              f, None, f'view{i}', lat, lon, dist, 0.25 * i))
    return views


def _view_table(c, views):
    from sunerf_hip import observations as obs
    rows, n_pixels = obs.view_descriptors(views)
    return c.IN('views', torch.from_numpy(rows.view(np.uint8).reshape(-1).copy())), n_pixels


POOL_SHAPES = [(n_slots, ch, extras, valid) for n_slots in (1, 255, 257, 517) for ch, extras, valid in ((1, 0, 0), (7, 1, 1), (7, 0, 1), (1, 1, 0))]


def _ray_pool(shape, device, misaligned):
    n_slots, ch, extras, with_valid = shape
    c = Ctx(device)
    views = _views(c, ch, [(29, 19, 1, ()), (5, 7, 2, (1, 4) if ch > 4 else ())])
    table, n_pixels = _view_table(c, views)
    assert n_pixels == 29 * 19 + 35
    if with_valid:
        keep = np.ones(n_pixels, dtype=bool)
        keep[[0, 17, 200, 551, 585]] = False          # the first and last pixel of both views among them
        valid = c.IN('valid_index', torch.from_numpy(np.nonzero(keep)[0]))
        n_valid = int(keep.sum())
    else:
        valid, n_valid = c.NULL('valid_index', IN), n_pixels
    slot_begin, seed, epoch = 3, 1234567891011, 5
    assert slot_begin + n_slots <= n_valid
    rays = c.OUT('rays', F32, n_slots * 6, offset=1 if misaligned else 0)
    time = c.OUT('time', F32, n_slots)
    target, wavelength = (c.OUT('target_image', F32, n_slots * ch), c.OUT('wavelength', F32, n_slots * ch)) if extras else \
        (c.NULL('target_image', OUT), c.NULL('wavelength', OUT))

    def expected():
        from sunerf_hip import observations as obs
        t = obs._Table.__new__(obs._Table)
        t.views, t.n_pixels, t.n_channels, t.desc, t.device = views, n_pixels, ch, table.t, c.device
        t.valid_index, t.n_valid = (valid.t if with_valid else None), n_valid
        out = t.empty(n_slots, bool(extras))
        if not extras:
            del out['target_image']
        t.build(out, slot_begin, n_slots, True, seed, epoch)
        return {k: v for k, v in out.items()}
    return Case('sunerf_build_ray_pool', shape, c.arena,
                [table, len(views), n_pixels, valid, n_valid, ch, 1, seed, epoch, slot_begin, n_slots, rays, time, target, wavelength, STREAM],
                expected, empty={10: 0})


@case('sunerf_build_ray_pool', POOL_SHAPES + [(257, 7, 1, 1, 'misaligned')],
      'observations.hip: 256 records per block staged in LDS and flushed with 16-byte stores; the misaligned case offsets `rays` by one '
      'float and must be refused with SUNERF_E_BADARG')
def build_ray_pool(shape, device):
    if len(shape) == 5:
        cs = _ray_pool(shape[:4], device, True)
        cs.shape, cs.expect_status = shape, -1
        return cs
    return _ray_pool(shape, device, False)


@case('sunerf_synchronic_map', [(n_rows, n_lon, ch, n_views) for n_rows, n_lon in ((1, 1), (3, 63), (2, 65), (3, 257)) for ch, n_views in ((1, 1), (7, 2))],
      'reprojection.hip: 256-thread blocks over the pixels of a slab of rows; coords only with one view')
def synchronic_map(shape, device):
    n_rows, n_lon, ch, n_views = shape
    c = Ctx(device)
    views = _views(c, ch, [(17, 19, 1, ()), (5, 7, 2, (1, 4) if ch > 4 else ())][:n_views])
    table, _ = _view_table(c, views)
    n_lat, row_begin = n_rows + 3, 2
    lat = c.IN('lat', torch.linspace(-1.2, 1.2, n_lat, dtype=F64))
    lon = c.IN('lon', torch.linspace(-1.5, 1.5, n_lon, dtype=F64) if n_lon > 1 else torch.tensor([0.3], dtype=F64))
    m = n_rows * n_lon
    image, footprint = c.OUT('map', F32, ch * m), c.OUT('footprint', I32, ch * m)
    coords = c.OUT('coords', F64, 3 * m) if n_views == 1 else c.NULL('coords', OUT)

    def expected():
        from sunerf_hip import reprojection
        r = reprojection.map_rows(views, lat.t, lon.t, 1.0, row_begin, n_rows, want_coords=n_views == 1)
        return dict(zip(('map', 'footprint', 'coords'), r))
    return Case('sunerf_synchronic_map', shape, c.arena,
                [table, n_views, ch, lat, n_lat, lon, n_lon, row_begin, n_rows, 1.0, image, footprint, coords, STREAM], expected, empty={8: 0})


@case('sunerf_reproject_views', [(obs, ch, co) for obs in (((1, 1),), ((15, 17),), ((1, 257),), ((16, 16), (1, 1)), ((23, 31), (5, 13)))
                                 for ch, co in ((1, 1), (3, 0), (7, 0))],
      'reprojection.hip: 256 pixels per block, rows of n_channels staged in LDS (s_out) and flushed with 16-byte stores '
      '(1, 255, 257, 257 and 778 pixels; odd channel counts)')
def reproject_views(shape, device):
    from sunerf_hip import reprojection
    from sunerf_hip.rays import pose_spherical
    observers, ch, want_coords = shape
    c = Ctx(device)
    n_lat, n_lon = 19, 37
    gen = _gen(ch + len(observers))
    image = c.IN('map', _rand(gen, ch, n_lat, n_lon))
    lat, lon = c.IN('lat', torch.linspace(-1.5, 1.5, n_lat, dtype=F64)), c.IN('lon', torch.linspace(-math.pi, math.pi, n_lon, dtype=F64))
    rows = np.zeros(len(observers), dtype=reprojection.OBSERVER_DESC)
    specs, offset = [], 0
    for i, (h, w) in enumerate(observers):
        tx = c.IN(f'observer{i}_tx', torch.linspace(-6e-3, 6e-3, w, dtype=F64) if w > 1 else torch.zeros(1, dtype=F64))
        ty = c.IN(f'observer{i}_ty', torch.linspace(-5e-3, 5e-3, h, dtype=F64) if h > 1 else torch.zeros(1, dtype=F64))
        o_lat, o_lon, dist = 0.2 - 0.3 * i, -0.5 + 1.1 * i, 215.0
        c2w = pose_spherical(-o_lon, o_lat, dist)
        rows[i]['pix_offset'], rows[i]['tx'], rows[i]['ty'] = offset, tx.ptr.value, ty.ptr.value
        rows[i]['height'], rows[i]['width'] = h, w
        rows[i]['c2w'] = np.asarray(c2w[:3, :4].reshape(-1).tolist(), dtype=np.float32)
        specs.append(dict(lat=o_lat, lon=o_lon, distance=dist, tx=tx.t, ty=ty.t))
        offset += h * w
    table = c.IN('observers', torch.from_numpy(rows.view(np.uint8).reshape(-1).copy()))
    out = c.OUT('out', F32, offset * ch)
    coords = c.OUT('coords', F64, 3 * offset) if want_coords else c.NULL('coords', OUT)

    def expected():
        smap = reprojection.SynchronicMap(image.t.view(ch, n_lat, n_lon), None, lat.t, lon.t, 1.0, None, None, None)
        r = smap.reproject_many([reprojection.Observer(**s) for s in specs], off_disk=-2.0, want_coords=bool(want_coords))
        images = r[0] if want_coords else r
        res = {'out': torch.cat([im.reshape(-1, ch) for im in images])}
        if want_coords:
            res['coords'] = r[1]
        return res
    return Case('sunerf_reproject_views', shape, c.arena,
                [image, ch, lat, n_lat, lon, n_lon, 1.0, table, len(observers), offset, -2.0, out, coords, STREAM], expected,
                rejections=[({9: 0}, -1)])          # header: non-positive shapes are SUNERF_E_BADARG


# ---- the MLP: packing, the fused forward, the backward routes -------------------------------------------------------------------
N_LINEAR, D_OUT = 3, 2               # in_layer (84 -> d), one hidden layer, out_layer (d -> 2)
FAST, EXACT = 0, 1                   # SUNERF_PRECISION_*
STASH_FP16, STASH_PHASE = 0, 1       # SUNERF_STASH_*


@functools.lru_cache(maxsize=None)
def _mlp_params(d):
    """nn.Linear's default initialisation (uniform +- 1 / sqrt(fan_in)) of the three layers, seeded."""
    gen = _gen(d)
    shapes = [(d, 84), (d, d), (D_OUT, d)]
    ws = [((2 * _rand(gen, *sh) - 1) / math.sqrt(sh[1])).contiguous() for sh in shapes]
    bs = [((2 * _rand(gen, sh[0]) - 1) / math.sqrt(sh[1])).contiguous() for sh in shapes]
    return ws, bs


_PACKED = {}


def _packed(d, device):
    """One ``PackedMLP`` per width (EXACT arithmetic), built once."""
    from sunerf_hip import ops
    if d not in _PACKED:
        ws, bs = _mlp_params(d)
        _PACKED[d] = ops.PackedMLP([w.to(device) for w in ws], [b.to(device) for b in bs], precision=ops.PRECISION_EXACT)
    return _PACKED[d]


def _mlp_rays(n, s):
    e = _emission_case(n, s)
    gen = _gen(1000 * n + s + 1)
    return e['o'], e['d'], _rand(gen, n), e['z'], (0.5 - _rand(gen, n, s, D_OUT)) * 1e-2


def _absmax(g_raw):
    return g_raw.abs().max().reshape(1).view(I32)


class _env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _stash_guard(d, s, fmt):
    """One forward workgroup's share of the activation stash: FWD_RAYS_PER_WG rays (a ray per wave) x the chunks of a ray."""
    import mlp_seams as ms
    return ms.FWD_RAYS_PER_WG * ms.chunks_per_ray(s) * ms.act_chunk_bytes(d, N_LINEAR, fmt)


def _dz_guard(d, s):
    import mlp_seams as ms
    return ms.FWD_RAYS_PER_WG * ms.chunks_per_ray(s) * ms.dz_chunk_bytes(d, N_LINEAR)


def _pipe_guard():
    """One workgroup's share of the pipelined backward's workspace: a hand-off ring of RING (bwd_pipe.hip:53) chunk slots."""
    import mlp_seams as ms
    return ms.PIPE_RING * ms.PIPE_SLOT


def _param_buffers(c, d, tag_prefix=''):
    ws, bs = _mlp_params(d)
    return [c.IN(f'{tag_prefix}weight{i}', w) for i, w in enumerate(ws)], [c.IN(f'{tag_prefix}bias{i}', b) for i, b in enumerate(bs)]


def _grad_buffers(c, d, acc):
    ws, bs = _mlp_params(d)
    gen = _gen(d + 99)
    init_w, init_b = [torch.randn(w.shape, generator=gen) for w in ws], [torch.randn(b.shape, generator=gen) for b in bs]
    if acc:
        gw = [c.INOUT(f'grad_weight{i}', t) for i, t in enumerate(init_w)]
        gb = [c.INOUT(f'grad_bias{i}', t) for i, t in enumerate(init_b)]
    else:
        gw = [c.OUT(f'grad_weight{i}', F32, t.numel()) for i, t in enumerate(init_w)]
        gb = [c.OUT(f'grad_bias{i}', F32, t.numel()) for i, t in enumerate(init_b)]

    def plain():          # the wrapper's own gradient tensors, holding the same initial values
        return [t.to(c.device).clone() for t in init_w], [t.to(c.device).clone() for t in init_b]

    def named(w, b):
        return {**{f'grad_weight{i}': t for i, t in enumerate(w)}, **{f'grad_bias{i}': t for i, t in enumerate(b)}}
    return gw, gb, plain, named


@case('sunerf_pack_mlp', [(d, p) for d in (64, 256) for p in (FAST, EXACT)], 'pack.hip: one fragment per thread, tail blocks per layer')
def pack_mlp(shape, device):
    d, precision = shape
    c = Ctx(device)
    wb, bb = _param_buffers(c, d)
    nbytes = int(_lib().sunerf_packed_mlp_bytes(d, N_LINEAR))
    packed = c.OUT('packed', U8, nbytes)

    def expected():
        from sunerf_hip import ops
        return {'packed': ops.PackedMLP([b.t.view(w.shape) for b, w in zip(wb, _mlp_params(d)[0])], [b.t for b in bb], precision=precision).buffer}
    return Case('sunerf_pack_mlp', shape, c.arena, [HostPtrs(wb), HostPtrs(bb), N_LINEAR, d, D_OUT, precision, packed, STREAM], expected)


@case('sunerf_pack_mlp_t', [64, 256], 'pack.hip: one fragment per thread, tail blocks per layer')
def pack_mlp_t(shape, device):
    d = shape
    c = Ctx(device)
    wb, _ = _param_buffers(c, d)
    packed_t = c.OUT('packedT', U8, int(_lib().sunerf_packed_mlp_t_bytes(d, N_LINEAR)))

    def expected():
        return {'packedT': _packed(d, c.device).transposed()}
    return Case('sunerf_pack_mlp_t', shape, c.arena, [HostPtrs(wb), N_LINEAR, d, D_OUT, packed_t, STREAM], expected)


def _forward(c, d, n, s, fmt):
    """(stash bytes, raw) of the wrapper's training forward in stash format ``fmt`` (GPU), zeros on the CPU."""
    nbytes = int(_lib().sunerf_act_stash_bytes(n, s, d, N_LINEAR, fmt))
    if not c.gpu:
        return torch.zeros(nbytes, dtype=U8), nbytes
    from sunerf_hip import ops
    o, dd, t, z, _ = _mlp_rays(n, s)
    packed = _packed(d, c.device)
    with _env(SUNERF_STASH='fp16' if fmt == STASH_FP16 else '', SUNERF_BACKWARD='classic' if fmt == STASH_FP16 else 'pipe'):
        out = ops._emission_render(packed, packed.buffer, EXACT, o.to(c.device), dd.to(c.device), t.to(c.device), z.to(c.device), 1.2, training=True)
    assert out['stash'].numel() == nbytes, (out['stash'].numel(), nbytes)
    return out['stash'], nbytes


RENDER_SHAPES = [(d, n, s, mode) for d, n, s in MLP_SHAPES for mode in ('inference', 'fp16', 'phase') if not (mode == 'phase' and d != 256)]


@case('sunerf_emission_render_fwd', RENDER_SHAPES,
      'render_fwd.hip / weight_ring.h WAVES 4: a ray per wave, 32-sample chunks; the stash is one chunk record per 32 samples of a ray '
      '+ one spare (guard: one workgroup\'s share, _stash_guard)')
def emission_render_fwd(shape, device):
    d, n, s, mode = shape
    c = Ctx(device)
    o_t, d_t, t_t, z_t, _ = _mlp_rays(n, s)
    nbytes = int(_lib().sunerf_packed_mlp_bytes(d, N_LINEAR))
    packed = c.IN('packed', _packed(d, c.device).buffer if c.gpu else torch.zeros(nbytes, dtype=U8))
    o, dd, t, z = c.IN('rays_o', o_t), c.IN('rays_d', d_t), c.IN('times', t_t), c.IN('z_vals', z_t)
    image, weights, absorption = c.OUT('image', F32, n), c.OUT('weights', F32, n * s), c.OUT('absorption', F32, n * s)
    training = mode != 'inference'
    fmt = STASH_PHASE if mode == 'phase' else STASH_FP16
    if training:
        raw = c.OUT('raw', F32, n * s * 2)
        hm, am, reg = (c.NULL(k, OUT) for k in ('height_map', 'absorption_map', 'regularization'))
        stash = c.OUT('act_stash', U8, int(_lib().sunerf_act_stash_bytes(n, s, d, N_LINEAR, fmt)), guard_bytes=_stash_guard(d, s, fmt))
    else:
        raw = c.OUT('raw', F32, n * s * 2) if n > 1 else c.NULL('raw', OUT)
        hm, am, reg = c.OUT('height_map', F32, n), c.OUT('absorption_map', F32, n), c.OUT('regularization', F32, n * s)
        stash = c.NULL('act_stash', OUT)
    ws_bytes = int(_lib().sunerf_render_workspace_bytes(d))
    assert ws_bytes == 0              # only d_filter 512 takes scratch
    ws = c.NULL('workspace', WORKSPACE)

    def expected():
        from sunerf_hip import ops
        p = _packed(d, c.device)
        with _env(SUNERF_STASH='fp16' if fmt == STASH_FP16 else '', SUNERF_BACKWARD='classic' if fmt == STASH_FP16 else 'pipe'):
            out = ops._emission_render(p, packed.t, EXACT, o.t.view(n, 3), dd.t.view(n, 3), t.t, z.t.view(n, s), 1.2,
                                       want_raw=training or n > 1, want_epilogues=not training, training=training)
        if training:
            assert ops.stash_format_of(out['stash'], n, s, p) == fmt
        if training:
            out['act_stash'] = out.pop('stash')          # opaque: compared on the bytes the direct call wrote
        return out
    return Case('sunerf_emission_render_fwd', shape, c.arena,
                [packed, d, N_LINEAR, EXACT, o, dd, t, z, n, s, image, weights, absorption, raw, hm, am, reg, 1.2, stash, fmt, ws, ws_bytes, STREAM],
                expected, empty={8: 0}, opaque=('act_stash',))


@case('sunerf_mlp_points_fwd', [(d, m, tr) for d in (64, 256) for m, tr in ((32, 0), (128, 1), (352, 0))],
      'render_fwd.hip: 32 points per chunk, a chunk per wave, WAVES 4 per workgroup; the header takes multiples of 32 only, so the '
      'rays x samples of the MLP shapes, 1, 99 and 325 points, are padded to 32, 128 and 352 as its callers do')
def mlp_points_fwd(shape, device):
    d, m, training = shape
    c = Ctx(device)
    gen = _gen(d + m)
    pts = torch.cat([torch.randn(m, 3, generator=gen) * 0.8, _rand(gen, m, 1)], 1)
    nbytes = int(_lib().sunerf_packed_mlp_bytes(d, N_LINEAR))
    packed = c.IN('packed', _packed(d, c.device).buffer if c.gpu else torch.zeros(nbytes, dtype=U8))
    points, raw = c.IN('points', pts), c.OUT('raw', F32, m * 2)
    if training:
        stash = c.OUT('act_stash', U8, int(_lib().sunerf_act_stash_bytes(m // 32, 32, d, N_LINEAR, STASH_FP16)),
                      guard_bytes=_stash_guard(d, 32, STASH_FP16))
    else:
        stash = c.NULL('act_stash', OUT)
    ws = c.NULL('workspace', WORKSPACE)

    def expected():
        from sunerf_hip import ops
        with _env(SUNERF_STASH='fp16', SUNERF_BACKWARD='classic'):
            out = ops.mlp_points_fwd(_packed(d, c.device), points.t.view(m, 4), training=bool(training))
        return {'raw': out['raw'], 'act_stash': out['stash']} if training else {'raw': out['raw']}
    return Case('sunerf_mlp_points_fwd', shape, c.arena, [packed, d, N_LINEAR, EXACT, points, m, raw, stash, STASH_FP16, ws, 0, STREAM], expected,
                empty={5: 0}, opaque=('act_stash',))


def _backward_inputs(c, d, n, s, fmt):
    stash_t, _ = _forward(c, d, n, s, fmt)
    g_t = _mlp_rays(n, s)[4]
    nbytes_t = int(_lib().sunerf_packed_mlp_t_bytes(d, N_LINEAR))
    packed_t = c.IN('packedT', _packed(d, c.device).transposed() if c.gpu else torch.zeros(nbytes_t, dtype=U8))
    stash = c.IN('act_stash', stash_t, guard_bytes=_stash_guard(d, s, fmt))
    g_raw, absmax = c.IN('g_raw', g_t), c.IN('g_absmax', _absmax(g_t))
    return packed_t, stash, g_raw, absmax


@case('sunerf_mlp_dgrad', MLP_SHAPES, 'render_bwd.hip DG_WAVES 4: a ray per wave, 32-sample chunks; dz_stash: a chunk record per 32 samples + a spare')
def mlp_dgrad(shape, device):
    d, n, s = shape
    c = Ctx(device)
    packed_t, stash, g_raw, absmax = _backward_inputs(c, d, n, s, STASH_FP16)
    dz = c.OUT('dz_stash', U8, int(_lib().sunerf_dz_stash_bytes(n, s, d, N_LINEAR)), guard_bytes=_dz_guard(d, s))
    return Case('sunerf_mlp_dgrad', shape, c.arena, [packed_t, d, N_LINEAR, g_raw, absmax, stash, dz, n, s, STREAM], lambda: {},
                empty={7: 0}, opaque=('dz_stash',))


def _wgrad_split(c, d):
    from sunerf_hip import ops
    cus = torch.cuda.get_device_properties(c.device).multi_processor_count if c.gpu else 256
    return ops.wgrad_split(N_LINEAR, cus, d)


@case('sunerf_mlp_wgrad', [(d, n, s, acc) for d, n, s in MLP_SHAPES for acc in (0, 1)],
      'wgrad.hip WG_THREADS 256: `split` partial sums per layer over the chunks (fewer chunks than partial sums at these sizes)')
def mlp_wgrad(shape, device):
    d, n, s, acc = shape
    c = Ctx(device)
    packed_t, stash, g_raw, absmax = _backward_inputs(c, d, n, s, STASH_FP16)
    dz_bytes = int(_lib().sunerf_dz_stash_bytes(n, s, d, N_LINEAR))
    dz_t = torch.zeros(dz_bytes, dtype=U8, device=c.device)
    if c.gpu:
        from sunerf_hip import lib, ops
        lib.call(c.device, 'sunerf_mlp_dgrad', packed_t.ptr, d, N_LINEAR, g_raw.ptr, absmax.ptr, stash.ptr, ops._ptr(dz_t), n, s, ops._stream(c.device))
    dz = c.IN('dz_stash', dz_t, guard_bytes=_dz_guard(d, s))
    split = _wgrad_split(c, d)
    ws = c.WS('workspace', int(_lib().sunerf_wgrad_workspace_bytes(d, N_LINEAR, split)))
    gw, gb, plain, named = _grad_buffers(c, d, acc)

    def expected():
        from sunerf_hip import ops
        w, b = plain()
        ops._mlp_backward_classic(_packed(d, c.device), g_raw.t.view(n, s, D_OUT), absmax.t, stash.t, w, b, bool(acc))
        return named(w, b)
    return Case('sunerf_mlp_wgrad', shape, c.arena,
                [d, N_LINEAR, D_OUT, packed_t, stash, dz, g_raw, absmax, n, s, ws, split, HostPtrs(gw), HostPtrs(gb), acc, STREAM], expected,
                empty={8: 0},          # header: no rays, zero gradients (accumulate: nothing)
                empty_effect=lambda: {} if acc else {b.name: torch.zeros(b.numel) for b in (*gw, *gb)})


@case('sunerf_mlp_backward_pipe', [(256, n, s, acc) for d, n, s in MLP_SHAPES if d == 256 for acc in (0, 1)],
      'bwd_pipe.hip: persistent launch of 256 workgroups, pairs own a layer; fewer chunks than pipelines at these sizes; workspace: '
      'sticky block (zeroed by the caller), control block, hand-off rings of RING 16 slots (guard: _pipe_guard)')
def mlp_backward_pipe(shape, device):
    d, n, s, acc = shape
    c = Ctx(device)
    packed_t, stash, g_raw, absmax = _backward_inputs(c, d, n, s, STASH_PHASE)
    nbytes = 0
    if c.gpu:
        with torch.cuda.device(c.device):
            nbytes = int(_lib().sunerf_bwd_pipe_workspace_bytes(n, s, d, N_LINEAR))
        assert nbytes > 0, 'the pipelined backward does not support this device'
    else:
        import mlp_seams as ms
        nbytes = ms.pipe_workspace_bytes(n, s, N_LINEAR)
    ws = c.WS('workspace', nbytes, guard_bytes=_pipe_guard(), init='zero_head:256')
    gw, gb, plain, named = _grad_buffers(c, d, acc)

    def expected():
        from sunerf_hip import ops
        w, b = plain()
        with _env(SUNERF_PIPE_HI_ONLY='0', SUNERF_PIPE_DEBUG='0'):
            ops._mlp_backward_pipe(_packed(d, c.device), g_raw.t.view(n, s, D_OUT), absmax.t, stash.t, nbytes, w, b, bool(acc))
        assert ops.pipe_status(raise_on_failure=True) == 0
        return named(w, b)
    return Case('sunerf_mlp_backward_pipe', shape, c.arena,
                [d, N_LINEAR, D_OUT, packed_t, stash, g_raw, absmax, n, s, ws, nbytes, HostPtrs(gw), HostPtrs(gb), acc, 0, STREAM], expected,
                ws_index=10, rejections=[({7: 0}, -1)])          # header: n_rays >= 1


def _query(c, n, s, mode):
    o_t, d_t, t_t, z_t, g_t = _mlp_rays(n, s)
    if mode == 'rays':
        bufs = [c.IN('rays_o', o_t), c.IN('rays_d', d_t), c.IN('times', t_t), c.IN('z_vals', z_t), c.NULL('points', IN)]
    else:
        p = torch.cat([(o_t[:, None, :] + d_t[:, None, :] * z_t[:, :, None]), t_t[:, None, None].expand(n, s, 1)], -1).reshape(-1, 4)
        bufs = [c.NULL(k, IN) for k in ('rays_o', 'rays_d', 'times', 'z_vals')] + [c.IN('points', p.contiguous())]
    return bufs, c.IN('g_raw', g_t)


def _query_of(bufs, n, s, mode):
    o, d, t, z, p = bufs
    return ('rays', o.t.view(n, 3), d.t.view(n, 3), t.t, z.t.view(n, s)) if mode == 'rays' else ('points', p.t.view(n * s, 4))


# the fp32 routes take a single sample: (1, 1) as well
EXACT_MLP_SHAPES = tuple((d, n, s) for d in (64, 256) for n, s in ((1, 1), (1, 2), (3, 33), (5, 65)))
EXACT_SHAPES = [(d, n, s, mode, acc) for d, n, s in EXACT_MLP_SHAPES for mode, acc in (('rays', 0), ('points', 1))]


def _backward_exact(name, chunked, shape, device):
    d, n, s, mode, acc = shape
    c = Ctx(device)
    wb, bb = _param_buffers(c, d)
    bufs, g_raw = _query(c, n, s, mode)
    lib = _lib()
    nbytes = int(lib.sunerf_mlp_backward_exact_chunked_workspace_bytes(d, N_LINEAR) if chunked else
                 lib.sunerf_mlp_backward_exact_workspace_bytes(n * s, d, N_LINEAR))
    ws = c.WS('workspace', nbytes)
    gw, gb, plain, named = _grad_buffers(c, d, acc)

    def expected():
        from sunerf_hip import ops
        w, b = plain()
        ops._mlp_backward_exact(_packed(d, c.device), g_raw.t.view(n, s, D_OUT), _query_of(bufs, n, s, mode), w, b, bool(acc), chunked=chunked)
        return named(w, b)
    return Case(name, shape, c.arena,
                [HostPtrs(wb), HostPtrs(bb), N_LINEAR, d, D_OUT, *bufs, n, s, g_raw, ws, nbytes, HostPtrs(gw), HostPtrs(gb), acc, STREAM], expected,
                ws_index=14, rejections=[({10: 0}, -1)])          # header: n_rays >= 1


@case('sunerf_mlp_backward_exact', EXACT_SHAPES, 'bwd_exact.hip: LDS-tiled fp32 MFMA GEMMs over all samples at once, COLSUM_ROWS 256 rows per bias block')
def mlp_backward_exact(shape, device):
    return _backward_exact('sunerf_mlp_backward_exact', False, shape, device)


@case('sunerf_mlp_backward_exact_chunked', EXACT_SHAPES,
      'bwd_exact.hip: chunks of 32768 samples, WGRAD_BLOCKS 512 split-K blocks, fp64 accumulators in the workspace')
def mlp_backward_exact_chunked(shape, device):
    return _backward_exact('sunerf_mlp_backward_exact_chunked', True, shape, device)


@case('sunerf_mlp_input_grad_exact', [(d, n, s, mode, params) for d, n, s in EXACT_MLP_SHAPES for mode, params in (('rays', 0), ('points', 1), ('rays', 1))],
      'bwd_exact.hip: the chunked kernel + an 84-column GEMM per chunk, per-ray fp64 sums')
def mlp_input_grad_exact(shape, device):
    d, n, s, mode, with_params = shape
    c = Ctx(device)
    wb, bb = _param_buffers(c, d)
    bufs, g_raw = _query(c, n, s, mode)
    nbytes = int(_lib().sunerf_mlp_input_grad_exact_workspace_bytes(d, N_LINEAR))
    ws = c.WS('workspace', nbytes)
    if with_params:
        gw, gb, plain, named = _grad_buffers(c, d, 0)
        gw_arg, gb_arg = HostPtrs(gw), HostPtrs(gb)
    else:
        gw_arg = gb_arg = None
    if mode == 'points':
        outs = [c.OUT('grad_points', F32, n * s * 4)] + [c.NULL(k, OUT) for k in ('grad_rays_o', 'grad_rays_d', 'grad_times', 'grad_z')]
    else:
        # with parameter gradients: only grad_z of the ray gradients (any of them may be NULL)
        want = (False, False, False, True) if with_params else (True, True, True, True)
        sizes = (('grad_rays_o', n * 3), ('grad_rays_d', n * 3), ('grad_times', n), ('grad_z', n * s))
        outs = [c.NULL('grad_points', OUT)] + [c.OUT(k, F32, m) if w else c.NULL(k, OUT) for w, (k, m) in zip(want, sizes)]

    def expected():
        from sunerf_hip import ops
        w, b = plain() if with_params else (None, None)
        r = ops.mlp_input_backward(_packed(d, c.device), g_raw.t.view(n, s, D_OUT) if mode == 'rays' else g_raw.t.view(n * s, D_OUT),
                                   _query_of(bufs, n, s, mode), w, b, False, wanted=(True,) * 4 if mode == 'points' else want)
        res = {'grad_points': r} if mode == 'points' else {k: t for (k, _), t in zip(sizes, r) if t is not None}
        if with_params:
            res.update(named(w, b))
        return res
    return Case('sunerf_mlp_input_grad_exact', shape, c.arena,
                [HostPtrs(wb), HostPtrs(bb), N_LINEAR, d, D_OUT, *bufs, n, s, g_raw, ws, nbytes, gw_arg, gb_arg, 0, *outs, STREAM], expected,
                ws_index=14, rejections=[({10: 0}, -1)])          # header: n_rays >= 1
