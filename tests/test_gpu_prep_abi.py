"""The three launching entry points of include/sunerf_hip_prep.h stay inside their buffers: the checks of
tests/test_gpu_abi_extents.py (runs A and B with sentinel and NaN fills, guards, inputs untouched, outputs equal to the wrapper
by bits and independent of what they held, the workspace bound, the empty call) on cases built with ``abi_cases.Ctx`` / ``Case``
and the guarded arena of tests/abi_arena.py, with the extents the header states.

The cases live in this file's own table ``PREP_CASES`` (tests/test_abi_tables_host.py holds it to the table's symbols)."""
import numpy as np
import pytest
import torch

import abi_cases as ac
from abi_arena import IN, OUT
from abi_cases import F32, F64, I64, STREAM, U8, Case, Ctx

pytestmark = pytest.mark.gpu

TILES = ('prep.hip: prefilter tiles of 64 lines x 128 samples (PF_THREADS 256); resample 256 output pixels per workgroup; order '
         'statistics 4096 values per workgroup at least, 128 workgroups per plane at most')
# (planes, height, width, order, with mask): a single pixel, a partial tile, one tile plus one on both axes, a ragged
# multi-segment batch; a plane of one row (no pass along y, no workspace)
PREFILTER_SHAPES = [(1, 1, 1, 3, 1), (1, 37, 53, 3, 0), (1, 65, 129, 5, 1), (3, 70, 300, 4, 1), (2, 1, 131, 2, 0), (2, 9, 7, 1, 1)]
# (planes, height, width, order, out height, out width, flags): 1, 255, 257 and 3 x 713 output pixels
RESAMPLE_SHAPES = [(1, 1, 1, 0, 1, 1, 0), (1, 9, 11, 3, 15, 17, 1 | 8), (1, 12, 7, 5, 1, 257, 2 | 4), (3, 37, 53, 4, 23, 31, 31),
                   (2, 6, 5, 1, 9, 8, 16)]
# (planes, values, ranks): one value, a partial workgroup, one workgroup plus one value, ragged groups in a batch
SELECT_SHAPES = [(1, 1, 1), (1, 4095, 4), (1, 4097, 2), (3, 2 * 4096 + 77, 8)]


def _image(c, h, w, seed):
    gen = ac._gen(seed)
    img = ac._rand(gen, c, h, w) * 1000.0
    if h * w > 4:
        img.view(-1)[1::h * w // 3 + 1] = float('nan')
        img.view(-1)[2] = float('inf')
    return img


def prefilter(shape, device):
    c_, h, w, order, with_mask = shape
    c = Ctx(device)
    image = c.IN('image', _image(c_, h, w, 100 * h + w))
    coef = c.OUT('coefficients', F64, c_ * h * w)
    mask = c.OUT('nonfinite_mask', U8, c_ * h * w) if with_mask else c.NULL('nonfinite_mask', OUT)
    nbytes = int(ac._lib().sunerf_prep_workspace_bytes(0, c_, h, w, order))
    assert nbytes == (c_ * h * w * 8 if order >= 2 and h >= 2 else 0)              # the header's formula
    ws = c.WS('workspace', nbytes)

    def expected():
        from sunerf_hip import prep
        co, m = prep.spline_prefilter(image.t.view(c_, h, w), order, want_mask=bool(with_mask))
        return {'coefficients': co, **({'nonfinite_mask': m} if with_mask else {})}
    return Case('sunerf_prep_spline_prefilter', shape, c.arena, [image, c_, h, w, order, coef, mask, ws, nbytes, STREAM], expected,
                ws_index=8 if nbytes else None, empty={1: 0})


def resample(shape, device):
    c_, h, w, order, nh, nw, flags = shape
    c = Ctx(device)
    gen = ac._gen(h * 17 + w)
    coef = c.IN('coefficients', (ac._rand(gen, c_, h, w) * 100.0).double())
    bad = (ac._rand(gen, c_, h, w) < 0.05).to(U8)
    mask = c.IN('nonfinite_mask', bad) if flags & 16 else c.NULL('nonfinite_mask', IN)
    par = torch.tensor([[5.0 + k, 90.0, 0.5 + k, 2.0, 40.0 + k, 0.0] for k in range(c_)], dtype=F64)
    params = c.IN('params', par)
    out = c.OUT('out', F32, c_ * nh * nw)
    th = 0.3
    s = 0.9 * min(h / nh, w / nw) if h > 1 else 1.0
    m = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]) * s if h > 1 else np.eye(2)
    off = np.array([(h - 1) / 2.0, (w - 1) / 2.0]) - m @ np.array([(nh - 1) / 2.0, (nw - 1) / 2.0])

    def expected():
        from sunerf_hip import prep
        return {'out': prep.affine_resample(coef.t.view(c_, h, w), m, off, (nh, nw), order, -1.5, params.t.view(c_, 6), flags,
                                            mask.t.view(c_, h, w) if flags & 16 else None)}
    args = [coef, mask, c_, h, w, order, float(m[0, 0]), float(m[0, 1]), float(m[1, 0]), float(m[1, 1]), float(off[0]), float(off[1]),
            -1.5, params, flags, nh, nw, out, STREAM]
    return Case('sunerf_prep_affine_resample', shape, c.arena, args, expected, empty={2: 0},
                rejections=[({5: 6}, -2), ({14: 32}, -2)])          # header: an order above 5, an unknown flag


def order_statistics(shape, device):
    c_, n, r = shape
    c = Ctx(device)
    gen = ac._gen(n + r)
    data = (ac._rand(gen, c_, n) - 0.5) * 8.0
    data = torch.where(ac._rand(gen, c_, n) < 0.3, torch.round(data), data)          # ties, zeros
    if n > 4:
        data[:, 3] = float('nan')
        data[0, 4] = float('-inf')
    x = c.IN('x', data)
    rk = torch.randint(0, max(1, n - 1), (c_, r), generator=gen, dtype=I64)
    rk[0, 0] = 0
    if r > 1:
        rk[-1, -1] = n                                                               # outside the valid ranks: NaN
    ranks = c.IN('ranks', rk)
    values, nan_count = c.OUT('values', F32, c_ * r), c.OUT('nan_count', I64, c_)
    nbytes = int(ac._lib().sunerf_prep_workspace_bytes(1, c_, n, 1, r))
    groups = min(128, -(-n // 4096))
    assert nbytes == c_ * r * 16 + c_ * groups * (r * 256 + 1) * 4                   # the header's formula
    ws = c.WS('workspace', nbytes)

    def expected():
        from sunerf_hip import prep
        v, k = prep.order_statistics(x.t.view(c_, n), ranks.t.view(c_, r))
        return {'values': v, 'nan_count': k}
    return Case('sunerf_prep_order_statistics', shape, c.arena, [x, c_, n, ranks, r, values, nan_count, ws, nbytes, STREAM], expected,
                ws_index=8, empty={1: 0}, rejections=[({4: 9}, -2)])               # header: more than 8 ranks


PREP_CASES = {'sunerf_prep_spline_prefilter': (prefilter, tuple(PREFILTER_SHAPES)),
              'sunerf_prep_affine_resample': (resample, tuple(RESAMPLE_SHAPES)),
              'sunerf_prep_order_statistics': (order_statistics, tuple(SELECT_SHAPES))}
PAIRS = [(name, shape) for name, (_, shapes) in PREP_CASES.items() for shape in shapes]


@pytest.mark.parametrize('name,shape', PAIRS, ids=[f'{n[7:]}-{ac.shape_id(s)}' for n, s in PAIRS])
def test_prep_entry_point_stays_inside_its_buffers(name, shape):
    import test_gpu_abi_extents as extents
    extents.check_entry_point(PREP_CASES[name][0], name, shape)
