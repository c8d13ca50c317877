"""The launching entry points of include/sunerf_hip_polarimetry.h check their arguments in the documented order and stay inside their
buffers: the checks of tests/test_gpu_abi_extents.py (runs A and B with sentinel and NaN fills, guards, inputs untouched, outputs
equal to the wrapper by bits and independent of what they held, the empty call, the header's rejections) on cases built with
``abi_cases.Ctx`` / ``Case`` and the guarded arena of tests/abi_arena.py, with the extents the header states: ``stokes`` at
``3 n_planes height width``, the planes and ``status`` at ``n_planes height width`` or NULL, ``counts`` at 4 int64 per plane or NULL;
the six per-ray outputs of the depth at ``n`` or NULL.  There is no workspace.

The cases live in this file's own table ``POLARIMETRY_CASES`` (tests/test_polarimetry_host.py holds it to the table's symbols)."""
import ctypes

import numpy as np
import pytest
import torch

import abi_cases as ac
from abi_arena import IN, OUT
from abi_cases import F32, I64, STREAM, U8, Case, Ctx, HostValue

pytestmark = pytest.mark.gpu

# (frames, planes, height, width, with bad, with the noise model, with the optional outputs): the shapes of tests/test_gpu_polarimetry.py
# -- one pixel, one pixel past a workgroup of 256, several planes, the most frames -- and one with every optional output absent
STOKES_SHAPES = [(3, 1, 1, 1, 0, 0, 1), (3, 1, 1, 257, 1, 1, 1), (4, 2, 3, 85, 1, 0, 1), (8, 1, 16, 16, 0, 1, 1), (5, 3, 7, 37, 1, 1, 1),
                 (5, 3, 7, 37, 0, 0, 0)]
# (rays, with the optional outputs)
DEPTH_SHAPES = [(1, 1), (255, 1), (256, 0), (257, 1)]
OPTIONAL = ('stokes', 'pb_cross', 'chi2', 'sigma_tb', 'sigma_pb', 'status', 'counts')


def _host(values):
    values = [float(v) for v in values]
    return HostValue((ctypes.c_double * len(values))(*values))


def stokes(shape, device):
    from sunerf_hip import polarimetry as pl
    from test_gpu_polarimetry import make_frames
    n, c_, h, w, with_bad, model, full = shape
    c = Ctx(device)
    planes, flagged, design, a, b = make_frames(n, c_, h, w)
    frames = c.IN('frames', torch.from_numpy(planes.copy()))
    bad = c.IN('bad', torch.from_numpy(flagged.copy())) if with_bad else c.NULL('bad', IN)
    va = c.IN('a', torch.from_numpy(a.astype(np.float64))) if model else c.NULL('a', IN)
    vb = c.IN('b', torch.from_numpy(b.astype(np.float64))) if model else c.NULL('b', IN)
    px = c_ * h * w
    outs = {'stokes': (F32, 3 * px), 'tb': (F32, px), 'pb': (F32, px), 'pb_cross': (F32, px), 'chi2': (F32, px), 'sigma_tb': (F32, px),
            'sigma_pb': (F32, px), 'status': (U8, px), 'counts': (I64, 4 * c_)}
    bufs = {k: (c.OUT(k, *v) if full or k not in OPTIONAL else c.NULL(k, OUT)) for k, v in outs.items()}
    centre = (0.5 * h - 0.5, float(w // 2))          # on a pixel of a plane with an odd number of rows

    def expected():
        names = tuple(k for k in pl.STOKES_OUTPUTS if full or k not in OPTIONAL)
        return pl.stokes_launch(frames.t.view(n, c_, h, w), bad.t.view(n, c_, h, w) if with_bad else None, *design,
                                va.t if model else None, vb.t if model else None, *centre, outputs=names)
    args = [frames, bad, *[_host(v) for v in design], va, vb, n, c_, h, w, *centre, *[bufs[k] for k in pl.STOKES_OUTPUTS], STREAM]
    zero_throughput = _host([1.0] * (n - 1) + [0.0])
    nan_cos = _host([float('nan')] + [0.5] * (n - 1))
    return Case('sunerf_polarimetry_stokes', shape, c.arena, args, expected, empty={9: 0},
                rejections=[({8: 9}, -2), ({8: 9, 9: 0}, -2), ({8: 2}, -1), ({8: 2, 10: 0}, -1), ({9: -1}, -1), ({12: float('nan')}, -1),
                            ({13: float('inf')}, -1), ({0: None}, -1), ({2: None}, -1), ({5: None}, -1), ({15: None}, -1), ({16: None}, -1),
                            ({4: zero_throughput}, -1), ({5: zero_throughput}, -1), ({2: nan_cos}, -1), ({15: frames}, -1), ({16: frames}, -1)]
                + ([({6: None}, -1), ({7: None}, -1)] if model else [({6: frames}, -1)])
                + ([({15: bad}, -1)] if with_bad else []) + ([({14: frames}, -1), ({21: frames}, -1)] if full else []))


def ratio_depth(shape, device):
    from sunerf_hip import polarimetry as pl
    from test_gpu_polarimetry import lattice_rays
    import polarimetry_reference as pr
    n, full = shape
    c = Ctx(device)
    R, u = 0.25, 0.63
    o, d, z = (np.concatenate([v] * 3)[:n] for v in lattice_rays(R, seed=5))
    # the ratio of one electron at the sample, and beside the ordinary rays one of every other status
    _, l, z0, b2, _ = pr.ray_geometry(o, d)
    f = pr.ratio(np.abs(z.astype(np.float64) - z0) * l, b2, np.float64(R), np.float64(np.float32(u)))
    tb_v = np.linspace(1.0, 3.0, n).astype(np.float32)
    pb_v = (f * tb_v).astype(np.float32)
    if n > 8:
        tb_v[1], pb_v[2], pb_v[3] = np.nan, -1.0, 4.0                    # INVALID, BELOW, ABOVE
        d[4] = 0.0                                                        # DEGENERATE
        o[5], d[5] = (0.1, 0.05, -50.0), (0.0, 0.0, 1.0)                  # CLOSE
    tb, pb, rays_o, rays_d = c.IN('tb', torch.from_numpy(tb_v)), c.IN('pb', torch.from_numpy(pb_v)), c.IN('rays_o', torch.from_numpy(o)), \
        c.IN('rays_d', torch.from_numpy(d))
    rs, ld = c.IN('solar_radius', torch.tensor([R], dtype=F32)), c.IN('limb_darkening_coeff', torch.tensor([u], dtype=F32))
    bufs = {k: (c.OUT(k, U8 if k == 'status' else F32, n) if full or k in ('depth', 'status') else c.NULL(k, OUT)) for k in pl.DEPTH_OUTPUTS}

    def expected():
        names = tuple(k for k in pl.DEPTH_OUTPUTS if full or k in ('depth', 'status'))
        return pl.ratio_depth_launch(tb.t, pb.t, rays_o.t.view(n, 3), rays_d.t.view(n, 3), rs.t, ld.t, 48.0, outputs=names)
    args = [tb, pb, rays_o, rays_d, rs, ld, n, 48.0, *[bufs[k] for k in pl.DEPTH_OUTPUTS], STREAM]
    return Case('sunerf_polarimetry_ratio_depth', shape, c.arena, args, expected, empty={6: 0},
                rejections=[({6: -1}, -1), ({7: 0.0}, -1), ({7: -1.0}, -1), ({7: float('nan')}, -1), ({7: float('inf')}, -1)]
                + [({i: None}, -1) for i in (0, 1, 2, 3, 4, 5, 8, 13)])


POLARIMETRY_CASES = {'sunerf_polarimetry_stokes': (stokes, tuple(STOKES_SHAPES)), 'sunerf_polarimetry_ratio_depth': (ratio_depth, tuple(DEPTH_SHAPES))}
PAIRS = [(name, shape) for name, (_, shapes) in POLARIMETRY_CASES.items() for shape in shapes]


def test_argument_checks_come_in_the_documented_order():
    """The checks of tests/test_polarimetry_host.py on the library the GPU tests run: no call reaches a launch."""
    from sunerf_hip import lib
    from test_polarimetry_host import check_argument_order
    check_argument_order(lib.load())


@pytest.mark.parametrize('name,shape', PAIRS, ids=[f'{n[7:]}-{ac.shape_id(s)}' for n, s in PAIRS])
def test_polarimetry_entry_point_stays_inside_its_buffers(name, shape):
    import test_gpu_abi_extents as extents
    extents.check_entry_point(POLARIMETRY_CASES[name][0], name, shape)
