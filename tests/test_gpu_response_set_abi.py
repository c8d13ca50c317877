"""The three launching entry points of include/sunerf_hip_response.h stay inside their buffers: the checks of
tests/test_gpu_abi_extents.py (runs A and B with sentinel and NaN fills, guards, inputs untouched, outputs equal to the wrapper
by bits and independent of what they held, the empty call) on cases built with ``abi_cases.Ctx`` / ``Case`` and the guarded arena
of tests/abi_arena.py, with the extents the response-set header states.

The cases live in this file's own table ``RESPONSE_CASES`` (tests/test_abi_tables_host.py holds it to the table's symbols)."""
import functools

import pytest
import torch

import abi_cases as ac
import response_set_cases as rc
from abi_arena import IN, OUT
from abi_cases import F32, I32, STREAM, Case, Ctx

pytestmark = pytest.mark.gpu

# (rays, samples, columns, epilogues / per-sample gradients): one ray, a partial group, a group and one ray, and a ragged
# three-group batch (8 + 8 + 5 rays) whose sample count is no multiple of the 32-sample chunk
SHAPES = [(1, 33, 1, 0), (7, 31, 3, 1), (9, 65, 8, 1), (21, 37, 8, 0)]
# the same on the ragged 64-channel, 4096-node set ``R64r`` of tests/response_set_cases.py (a fifth entry names the set): the
# extents the header gives at its limits -- offsets[65], codes[64], logt / resp[4096], log_abs[64], g_log_abs[64]
SET_SHAPES = [(9, 33, 8, 1, 'R64r'), (21, 37, 3, 0, 'R64r')]
TILES = 'dt_response_set.hip RS_THREADS 256: 8 rays per workgroup, 32 lanes per ray, 32 samples per chunk'
# the scalar gradients are added with float atomics per ray and per workgroup: from three terms on the order is free
ORDERED_RAYS = 2


@functools.lru_cache(maxsize=None)
def _case(n, s, w, set_name=None):
    return rc.make_case(n, s, w, 'nerf_dt', 1000 * n + s, channels=list(rc.set_channels(set_name)) if set_name else None)


def _inputs(c, n, s, w, set_name=None):
    """The input buffers of a call on the 11-channel set, or on the set ``set_name`` of ``response_set_cases.SET_NODES``."""
    e = _case(n, s, w, set_name)
    rset = rc.set_of(set_name) if set_name else rc.response_set()
    b = dict(raw=c.IN('raw', e['raw']), z=c.IN('z_vals', e['z']), o=c.IN('rays_o', e['o']), d=c.IN('rays_d', e['d']),
             wl=c.IN('wavelengths', e['wl']), off=c.IN('offsets', torch.from_numpy(rset.offsets)),
             codes=c.IN('codes', torch.tensor(rset.codes, dtype=F32)),
             lt=c.IN('logt', torch.cat([torch.as_tensor(rset.table(i)[0]) for i in range(len(rset))])),
             resp=c.IN('resp', torch.cat([torch.as_tensor(rset.table(i)[1]) for i in range(len(rset))])),
             la=c.IN('log_abs', e['log_abs'].float()), vc=c.IN('vol_c', e['vol_c'].float()))
    head = [b['raw'], b['z'], b['o'], b['d'], b['wl'], w, rset.n_channels, rset.n_nodes, b['off'], b['codes'], b['lt'], b['resp'],
            b['la'], b['vc'], 10.0, 5.0, float(e['pixel']), 1.25, n, s]
    return e, rset, b, head


def _wrapper_args(b, e, rset, n, s, w):
    return (b['raw'].t.view(n, s, 2), b['z'].t.view(n, s), b['o'].t.view(n, 3), b['d'].t.view(n, 3), b['wl'].t.view(n, w), rset,
            b['la'].t, b['vc'].t, 10.0, 5.0, float(e['pixel']), 1.25)


def response_fwd(shape, device):
    n, s, w, epi = shape[:4]
    c = Ctx(device)
    e, rset, b, head = _inputs(c, n, s, w, *shape[4:])
    image, weights, reg_q = c.OUT('image', F32, n * w), c.OUT('weights', F32, n * s), c.OUT('reg_q', F32, n * s)
    if epi:
        hm, am, reg = c.OUT('height_map', F32, n), c.OUT('absorption_map', F32, n), c.OUT('regularization', F32, n * s)
    else:
        hm, am, reg = (c.NULL(k, OUT) for k in ('height_map', 'absorption_map', 'regularization'))

    def expected():
        from sunerf_hip import ops
        out = ops.dt_response_fwd(*_wrapper_args(b, e, rset, n, s, w), want_epilogues=bool(epi))
        return {k: out[k] for k in ('image', 'weights', 'reg_q') + (('height_map', 'absorption_map', 'regularization') if epi else ())}
    return Case('sunerf_dt_response_fwd', shape, c.arena, head + [image, weights, reg_q, hm, am, reg, STREAM], expected,
                empty={18: 0})


def _response_bwd(name, shape, device, full):
    n, s, w, with_reg = shape[:4]
    c = Ctx(device)
    e, rset, b, head = _inputs(c, n, s, w, *shape[4:])
    m = rset.n_channels
    gen = ac._gen(n * 31 + s)
    g_image = c.IN('g_image', e['g_image'].float())
    names = ('g_reg', 'g_weights', 'g_reg_q') if full else ('g_reg',)
    per_sample = [c.IN(k, 0.5 - ac._rand(gen, n, s)) if with_reg else c.NULL(k, IN) for k in names]
    g_raw, g_la, g_vc, absmax = (c.OUT('g_raw', F32, n * s * 2), c.OUT('g_log_abs', F32, m), c.OUT('g_vol_c', F32, 1),
                                 c.OUT('g_absmax', I32, 1))

    def expected():
        from sunerf_hip import ops
        fn = ops.dt_response_bwd_full if full else ops.dt_response_bwd
        g, la, vc, am = fn(*_wrapper_args(b, e, rset, n, s, w), g_image.t.view(n, w),
                           *[p.t.view(n, s) if with_reg else None for p in per_sample])
        return {'g_raw': g, 'g_log_abs': la, 'g_vol_c': vc, 'g_absmax': am}

    def tolerance(key, got, want):
        """g_log_abs / g_vol_c are added with float atomics: the bound of the kernel's own test; everything else by bits."""
        import test_gpu_dt_integral as dt
        if key in ('g_log_abs', 'g_vol_c'):
            ref = want.detach().cpu().double()
            assert dt.scalar_rel(got, ref, ref.reshape(-1) == 0) <= dt.SCALAR_GRADIENT_REL, key
        else:
            assert torch.equal(got.reshape(-1).view(I32), want.reshape(-1).view(I32)), key

    # header: an empty batch clears the three scalar outputs
    effect = lambda: {'g_log_abs': torch.zeros(m), 'g_vol_c': torch.zeros(1), 'g_absmax': torch.zeros(1, dtype=I32)}    # noqa: E731
    return Case(name, shape, c.arena, head + [g_image, *per_sample, g_raw, g_la, g_vc, absmax, STREAM], expected, empty={18: 0},
                empty_effect=effect, reproducible=n <= ORDERED_RAYS, tolerance=tolerance)


def response_bwd(shape, device):
    return _response_bwd('sunerf_dt_response_bwd', shape, device, False)


def response_bwd_full(shape, device):
    return _response_bwd('sunerf_dt_response_bwd_full', shape, device, True)


RESPONSE_CASES = {'sunerf_dt_response_fwd': (response_fwd, tuple(SHAPES + SET_SHAPES)),
                  'sunerf_dt_response_bwd': (response_bwd, tuple(SHAPES + SET_SHAPES)),
                  'sunerf_dt_response_bwd_full': (response_bwd_full, tuple(SHAPES + SET_SHAPES))}
PAIRS = [(name, shape) for name, (_, shapes) in RESPONSE_CASES.items() for shape in shapes]


@pytest.mark.parametrize('name,shape', PAIRS, ids=[f'{n[7:]}-{ac.shape_id(s)}' for n, s in PAIRS])
def test_response_entry_point_stays_inside_its_buffers(name, shape):
    import test_gpu_abi_extents as extents
    extents.check_entry_point(RESPONSE_CASES[name][0], name, shape)
