"""The two launching entry points of include/sunerf_hip_patch.h check their arguments in the documented order and stay inside
their buffers: the checks of tests/test_gpu_abi_extents.py (runs A and B with sentinel and NaN fills, guards, inputs untouched,
outputs equal to the wrapper by bits and independent of what they held, the empty call, the header's rejections) on cases built
with ``abi_cases.Ctx`` / ``Case`` and the guarded arena of tests/abi_arena.py, with the extents the header states.

The cases live in this file's own table ``PATCH_CASES`` (tests/test_abi_tables_host.py holds it to the table's symbols)."""
import numpy as np
import pytest
import torch

import abi_cases as ac
from abi_arena import OUT
from abi_cases import F32, I32, STREAM, Case, Ctx

pytestmark = pytest.mark.gpu

TILES = ('patch.hip: adjoint tiles of 32 x 32 input pixels, 256 threads with four pixels each; records 256 rays, then 256 target '
         'elements, per workgroup')
# (planes, height, width, psf rows, psf columns, bin, per-plane kernels, boundary): a kernel larger than the image, a single pixel,
# one tile plus one / two tiles plus one, a ragged batch with per-plane kernels, exactly one tile, a binned ragged frame, the
# largest kernel
ADJOINT_SHAPES = [(1, 5, 7, 9, 9, 1, 0, 0), (1, 1, 1, 3, 3, 1, 0, 1), (1, 33, 65, 5, 5, 1, 0, 1), (3, 34, 67, 5, 5, 1, 1, 0),
                  (1, 32, 32, 3, 3, 2, 0, 1), (2, 37, 53, 7, 5, 3, 1, 1), (1, 40, 48, 89, 89, 8, 0, 1)]
# (patches, channels, patch, bin, psf rows, psf columns, with wavelength): one patch of one pixel, 256 rays plus a few, a batch
# with two channels and a view that lacks one, no wavelength output
RECORD_SHAPES = [(1, 1, 1, 1, 1, 1, 1), (3, 1, 4, 2, 3, 3, 1), (7, 2, 4, 2, 3, 5, 1), (5, 2, 3, 3, 4, 2, 0)]


def adjoint(shape, device):
    from sunerf_hip.instrument import Instrument, correlate_bin_adjoint
    c_, h, w, kh, kw, b, per_plane, boundary = shape
    c = Ctx(device)
    gen = ac._gen(100 * h + w + kh)
    g_out = c.IN('g_out', ac._rand(gen, c_, h // b, w // b) * 1000.0 - 100.0)
    psf = (ac._rand(gen, c_ if per_plane else 1, kh, kw).double() - 0.1).numpy()
    inst = Instrument(psf=psf if per_plane else psf[0], bin=b, boundary=('zero', 'nearest')[boundary])
    K, (ay, ax) = inst.effective_kernel()
    taps = c.IN('K', torch.from_numpy(K))
    g_in = c.OUT('g_in', F32, c_ * h * w)

    def expected():
        return {'g_in': correlate_bin_adjoint(g_out.t.view(c_, h // b, w // b), h, w, taps.t.view(K.shape), K.shape[0], K.shape[1],
                                              K.shape[2], b, ay, ax, inst.scale, boundary)}
    args = [g_out, c_, h, w, taps, K.shape[0], K.shape[1], K.shape[2], b, ay, ax, inst.scale, boundary, g_in, STREAM]
    return Case('sunerf_patch_correlate_bin_adjoint', shape, c.arena, args, expected, empty={1: 0},
                rejections=[({6: 97}, -2), ({7: 97}, -2), ({8: 9}, -2), ({12: 2}, -2)])          # header: the limits, the boundary


def records(shape, device):
    from sunerf_hip import observations as obs, patch
    from sunerf_hip.rays import pose_spherical
    n, ch, p, b, kh, kw, with_wl = shape
    keh, kew = kh + b - 1, kw + b - 1          # the effective kernel of a kh x kw PSF under bin b
    ay, ax = kh // 2, kw // 2
    c = Ctx(device)
    rng = np.random.default_rng(n * 100 + ch * 10 + p)
    views, axes = [], []
    for i, (h, w, n_planes, wl) in enumerate([(p + 5, p + 2, 1, [171.] + [0.] * (ch - 1)), (p + 1, p + 3, ch, [171., 193.][:ch])]):
        planes = (rng.uniform(0.0, 2.0, size=(n_planes, h, w)) * 10.0 ** rng.integers(-3, 4, size=(n_planes, h, w))).astype(np.float32)
        lat, lon, dist = 0.1 - 0.2 * i, 0.3 + 0.4 * i, 215.0 - 10 * i
        ext_x = patch.extended_axis(np.linspace(-6e-3, 6e-3, w), b, kew, ax)
        ext_y = patch.extended_axis(np.linspace(-5e-3, 5e-3, h), b, keh, ay)
        tx, ty = c.IN(f'view{i}_tx', torch.from_numpy(ext_x)), c.IN(f'view{i}_ty', torch.from_numpy(ext_y))
        image = c.IN(f'view{i}_image', planes)
        plane, wavelength = obs.channel_map(wl, n_planes)
        views.append(obs.View(image.t.view(n_planes, h, w), tx.t, ty.t, pose_spherical(-lon, lat, dist), 0.25 * i, plane, wavelength, 1,
                              None, f'view{i}', lat, lon, dist, 0.25 * i))          # (the extended axes only serve the descriptor)
        axes.append((tx.t, ty.t))
    rows = patch.patch_view_descriptors(views, axes)
    table = c.IN('views', torch.from_numpy(rows.view(np.uint8).reshape(-1).copy()))
    # every corner of both views' patch lattices in turn
    corners = [(v, r0, c0) for v, view in enumerate(views) for r0 in (0, view.height - p) for c0 in (0, view.width - p)]
    triples = c.IN('patches', torch.tensor([corners[k % len(corners)] for k in range(n)], dtype=I32))
    hw, ww = (p - 1) * b + keh, (p - 1) * b + kew
    rays, time = c.OUT('rays', F32, n * hw * ww * 6), c.OUT('time', F32, n * hw * ww)
    target = c.OUT('target_image', F32, n * ch * p * p)
    wavelength = c.OUT('wavelength', F32, n * hw * ww * ch) if with_wl else c.NULL('wavelength', OUT)

    def expected():
        return patch.records(table.t, len(views), triples.t.view(n, 3), ch, p, b, keh, kew, bool(with_wl))
    args = [table, len(views), triples, n, ch, p, b, keh, kew, rays, time, target, wavelength, STREAM]
    return Case('sunerf_patch_records', shape, c.arena, args, expected, empty={3: 0},
                rejections=[({7: 97}, -2), ({8: 97}, -2), ({6: 9}, -2), ({4: 17}, -1), ({1: 0}, -1)])


PATCH_CASES = {'sunerf_patch_correlate_bin_adjoint': (adjoint, tuple(ADJOINT_SHAPES)),
               'sunerf_patch_records': (records, tuple(RECORD_SHAPES))}
PAIRS = [(name, shape) for name, (_, shapes) in PATCH_CASES.items() for shape in shapes]


def test_argument_checks_come_in_the_documented_order():
    """The checks of tests/test_patch_host.py on the library the GPU tests run: no call reaches a launch."""
    from sunerf_hip import lib
    from test_patch_host import check_argument_order
    check_argument_order(lib.load())


@pytest.mark.parametrize('name,shape', PAIRS, ids=[f'{n[7:]}-{ac.shape_id(s)}' for n, s in PAIRS])
def test_patch_entry_point_stays_inside_its_buffers(name, shape):
    import test_gpu_abi_extents as extents
    extents.check_entry_point(PATCH_CASES[name][0], name, shape)
