"""The two voxel-grid fields node by node at their chunk and sphere seams, on a real MI355X:
csrc/grid_field.hip and csrc/dynamic_grid.hip against the float64 restatements, with the cases of tests/grid_seams.py.

1. Every gradient is bounded per node and channel, |got - want| <= (n + 8) 2^-24 A (static), (n + 10) 2^-24 A (time axis),
   A = sum |w||g| over the node's n samples (grid_seams: the derivation), nodes without a sample exactly 0 -- for the cases the
   two existing GPU files build and for everything below.  One dropped, doubled or misattributed segment moves a node by a
   whole term, a thousand bounds; the tensor's relative L2 of the existing tests need not notice.
2. Constructed layouts of the sorted inverted index (segments of 63 / 64 / 65 samples, long segments that start inside a piece,
   end on a piece boundary, share a piece with each other, with a short one, with the sentinel; totals of 64 k and 256 k + 1;
   long segments in the wrap cell; two adjacent intervals) in an *exact* mode, where the gradient must equal the restatement bit
   for bit, and a *random* mode under the bound.
3. The seams of a sphere -- poles, the longitude seam, first and last shell, r = 0, NaN, the faces of a patch, both signs of
   zero -- at points where inside / outside, cell and weights are decided identically by construction, at Rs_per_ds 1 and 0.25,
   and the random rays of the existing tests at Rs_per_ds = 0.7.
"""
import pytest
import torch

import dynamic_grid_reference as dref
import grid_field_reference as sref
import grid_seams as gs
import test_gpu_dynamic_grid as dynamic
import test_gpu_grid_field as static
from conftest import gate_units

pytestmark = pytest.mark.gpu

FLOOR, FILL = static.FLOOR, static.FILL
CHANNELS = (1, 3, 4)


def _bits(x):
    return x.contiguous().view(torch.int32)


def _static_desc(cs, c, Rs_per_ds=1.0):
    from sunerf_hip import grid_field as gf
    mode = gf.longitude_mode(cs['grid'])
    assert gf.LON_NAMES[mode] == cs['lon']
    return gf.GridDescriptor(cs['grid'], c, Rs_per_ds, FILL[:c], mode, 'cuda')


def _dynamic_desc(cs, c, Rs_per_ds=1.0):
    from sunerf_hip import dynamic_grid as dg, grid_field as gf
    mode = gf.longitude_mode(cs['grid'])
    assert gf.LON_NAMES[mode] == cs['lon']
    return dg.DynamicGridDescriptor(cs['grid'], c, Rs_per_ds, FILL[:c], mode, cs['tau'], cs['time_mode'], 'cuda')


def run_points(cs, c, with_time, Rs_per_ds=1.0):
    """Forward with the index and backward of the first ``c`` channels of a points case of grid_seams: ``(raw, ids, weights,
    grad)`` on the CPU; the backward runs twice and must give the same bits."""
    from sunerf_hip import dynamic_grid as dg, grid_field as gf
    values = cs['values'][..., :c].contiguous().cuda()
    g_raw = cs['g_raw'][:, :c].contiguous().cuda()
    if with_time:
        desc = _dynamic_desc(cs, c, Rs_per_ds)
        raw, index = dg.dynamic_grid_points(desc, values, cs['points'].cuda(), want_index=True)
        grad, again = dg.dynamic_grid_bwd(desc, g_raw, index), dg.dynamic_grid_bwd(desc, g_raw, index)
    else:
        desc = _static_desc(cs, c, Rs_per_ds)
        raw, index = gf.grid_field_points(desc, values, cs['points'].cuda(), want_index=True)
        grad, again = gf.grid_field_bwd(desc, g_raw, index), gf.grid_field_bwd(desc, g_raw, index)
    torch.cuda.synchronize()
    assert torch.equal(_bits(grad), _bits(again))
    return raw.cpu(), index[0].cpu().long(), index[1].cpu(), grad.cpu()


def check_forward(cs, c, raw, ids, decided=None):
    """The fill exactly where the restatement says, the gate of the existing forward tests everywhere else, and the ids of
    the points in ``decided`` (default: all) equal to the restatement's."""
    outside = ~cs['inside']
    n_cells = 1
    for k in gs.cells_per_axis(cs['grid'], cs['lon']):
        n_cells *= k
    sentinel = n_cells * (cs['values'].shape[0] - 1 if cs['values'].dim() == 5 else 1)
    assert torch.equal(ids == sentinel, outside) and int(ids.min()) >= 0 and int(ids.max()) <= sentinel
    fill = torch.tensor(FILL[:c])
    assert torch.equal(_bits(raw[outside]), _bits(fill.expand(int(outside.sum()), c)))
    sel = slice(None) if decided is None else decided
    assert torch.equal(ids[sel], cs['ids'][sel])
    return gate_units(raw, cs['raw'][:, :c], floor=FLOOR * cs['abs_sum'][:, :c])


def check_backward(cs, c, grad, slack, exact=False):
    if exact:
        assert torch.equal(grad.double(), cs['grad'][..., :c]), 'exact mode: the gradient differs from the restatement'
    return gs.node_check(grad, cs['grad'][..., :c], cs['terms'][..., :c], cs['count'], slack)


# ---- 1. the cases of the two existing files, node by node -------------------------------------------------------------------
@pytest.mark.parametrize('c', [1, 2, 4])
@pytest.mark.parametrize('name', static.GRIDS)
def test_static_cases_node_by_node(name, c):
    from sunerf_hip import grid_field as gf
    cs = static.case(name, c)
    field = static.make_field(cs)
    _, index = static._index(field, cs)
    got = gf.grid_field_bwd(field.descriptor(), cs['g_raw'].cuda(), index)
    pts = sref.ray_points(cs['o'], cs['d'], cs['z']).reshape(-1, 3)
    terms, count = sref.node_terms(cs['grid'], pts, cs['g_raw'].reshape(-1, c), 1.0, cs['lon'])
    worst = gs.node_check(got, cs['grad'], terms, count, gs.STATIC_SLACK)
    print(f'grid field backward {name} C={c}: worst node at {worst:.3f} of its bound, most samples on a node {int(count.max())}')
    assert worst <= 1.0


@pytest.mark.parametrize('mode', dynamic.MODES)
@pytest.mark.parametrize('name,c,n_frames', dynamic.CASES)
def test_dynamic_cases_node_by_node(name, c, n_frames, mode):
    from sunerf_hip import dynamic_grid as dg
    cs = dynamic.case(name, c, n_frames, mode)
    field = dynamic.make_field(cs)
    _, index = dynamic._index(field, cs)
    got = dg.dynamic_grid_bwd(field.descriptor(), cs['g_raw'].cuda(), index)
    n, s = cs['z'].shape
    pts = torch.cat([sref.ray_points(cs['o'], cs['d'], cs['z']), cs['t'].reshape(n, 1, 1).expand(n, s, 1)], -1).reshape(-1, 4)
    terms, count = dref.node_terms(cs['grid'], cs['tau'], pts, cs['g_raw'].reshape(-1, c), 1.0, cs['lon'], mode)
    worst = gs.node_check(got, cs['grad'], terms, count, gs.DYNAMIC_SLACK)
    print(f'dynamic grid backward {name} C={c} T={n_frames} {mode}: worst node at {worst:.3f} of its bound, most samples on a '
          f'node {int(count.max())}')
    assert worst <= 1.0


@pytest.mark.parametrize('name', gs.SCALED_GRIDS)
def test_random_rays_off_the_default_scale(name):
    """The rays of the existing cases at Rs_per_ds = 0.7: forward gate, fill, and the backward node by node."""
    from sunerf_hip import grid_field as gf
    cs = gs.scaled_rays_case(name)
    c = cs['c']
    desc = _static_desc(cs, c, cs['Rs'])
    raw, index = gf.grid_field_rays(desc, cs['values'].cuda(), cs['o'].cuda(), cs['d'].cuda(), cs['z'].cuda(), want_index=True)
    got = gf.grid_field_bwd(desc, cs['g_raw'].cuda(), index)
    torch.cuda.synchronize()
    units = gate_units(raw, cs['raw'], floor=FLOOR * cs['abs_sum'])
    outside = ~cs['inside']
    assert torch.equal(raw.cpu()[outside], torch.tensor(FILL[:c]).expand(int(outside.sum()), c))
    worst = gs.node_check(got, cs['grad'], cs['terms'], cs['count'], gs.STATIC_SLACK)
    print(f'grid field {name} at Rs_per_ds = 0.7: forward {units:.3f} gate units, worst node at {worst:.3f} of its bound')
    assert units <= 1.0 and worst <= 1.0


# ---- 2. constructed layouts of the inverted index ---------------------------------------------------------------------------
@pytest.mark.parametrize('c', CHANNELS)
@pytest.mark.parametrize('mode', gs.MODES)
@pytest.mark.parametrize('name', list(gs.LAYOUTS))
def test_static_layout(name, mode, c):
    cs = gs.static_layout(name, mode)
    raw, ids, _, grad = run_points(cs, c, with_time=False)
    units = check_forward(cs, c, raw, ids)
    worst = check_backward(cs, c, grad, gs.STATIC_SLACK, exact=mode == 'exact')
    print(f'grid field layout {name} {mode} C={c}: forward {units:.3f} gate units, worst node at {worst:.3f} of its bound')
    assert units <= 1.0 and worst <= 1.0


@pytest.mark.parametrize('c', CHANNELS)
@pytest.mark.parametrize('mode', gs.MODES)
@pytest.mark.parametrize('name', gs.DYNAMIC_LAYOUTS)
def test_dynamic_layout(name, mode, c):
    cs = gs.dynamic_layout(name, mode)
    raw, ids, _, grad = run_points(cs, c, with_time=True)
    units = check_forward(cs, c, raw, ids)
    worst = check_backward(cs, c, grad, gs.DYNAMIC_SLACK, exact=mode == 'exact')
    print(f'dynamic grid layout {name} {mode} C={c}: forward {units:.3f} gate units, worst node at {worst:.3f} of its bound')
    assert units <= 1.0 and worst <= 1.0


@pytest.mark.parametrize('c', CHANNELS)
@pytest.mark.parametrize('with_time', [False, True])
def test_long_segments_in_the_wrap_cell(with_time, c):
    cs = gs.wrap_layout(with_time)
    raw, ids, _, grad = run_points(cs, c, with_time)
    units = check_forward(cs, c, raw, ids)
    counts = torch.bincount(ids)
    assert [int(counts[i]) for i in gs.wrap_cell_ids(cs['grid'], with_time)] == [65, 200]
    worst = check_backward(cs, c, grad, gs.DYNAMIC_SLACK if with_time else gs.STATIC_SLACK)
    # the wrap column: node 0 of the longitude receives from the wrap cells
    assert float(grad.select(-3, 0).abs().max()) > 0 and float(grad.select(-3, grad.shape[-3] - 1).abs().max()) > 0
    print(f'{"dynamic grid" if with_time else "grid field"} wrap cell C={c}: forward {units:.3f} gate units, worst node at '
          f'{worst:.3f} of its bound')
    assert units <= 1.0 and worst <= 1.0


# ---- 3. the seams of a sphere -----------------------------------------------------------------------------------------------
N_AXIS = 168


def _check_axis_points(name, raw, ids, weights, cs, n_space=None):
    """On the axis points the decisions are exact: the weights are the restatement's (0 or 1 in latitude and longitude), and
    the sign of a zero component changes no bit on a periodic grid -- except at a pole, where the longitude is
    atan2(-+0, +-0) = 0 or pi by the sign of y, as the restatement has it too (the ids are compared in check_forward)."""
    grid, lon = cs['grid'], cs['lon']
    pts = cs['points'][:N_AXIS, :3]
    _, _, t, inside = sref.locate(grid, sref.grid_coordinates(grid, pts, cs['Rs'], lon), lon)
    want = torch.stack([1 - t, t], -1).reshape(N_AXIS, 6).float()
    inside = inside & cs['inside'][:N_AXIS]
    assert torch.equal(weights[:N_AXIS, :6][inside], want[inside])
    if name in gs.PERIODIC:
        r = _bits(raw[:N_AXIS]).reshape(6, 7, 4, -1)
        assert torch.equal(r[:4], r[:4, :, :1].expand_as(r[:4]))
        assert torch.equal(r[4:, :, 0], r[4:, :, 2]) and torch.equal(r[4:, :, 1], r[4:, :, 3])


@pytest.mark.parametrize('c', [1, 3])
@pytest.mark.parametrize('Rs_per_ds', gs.SCALES)
@pytest.mark.parametrize('name', gs.SPHERES)
def test_sphere_seams(name, Rs_per_ds, c):
    cs = gs.sphere_case(name, Rs_per_ds)
    raw, ids, weights, grad = run_points(cs, c, with_time=False, Rs_per_ds=Rs_per_ds)
    n_decided = N_AXIS + gs.special_points().shape[0]
    units = check_forward(cs, c, raw, ids, decided=slice(0, n_decided))
    _check_axis_points(name, raw, ids, weights, cs)
    worst = check_backward(cs, c, grad, gs.STATIC_SLACK)
    print(f'grid field sphere {name} Rs_per_ds={Rs_per_ds} C={c}: {int(cs["inside"].sum())} of {cs["inside"].shape[0]} points '
          f'inside, forward {units:.3f} gate units, worst node at {worst:.3f} of its bound')
    assert units <= 1.0 and worst <= 1.0
    if Rs_per_ds != 1.0:                                  # a power of two: the same bits as at scale 1
        one = run_points(gs.sphere_case(name, 1.0), c, with_time=False)
        assert torch.equal(_bits(raw), _bits(one[0])) and torch.equal(ids, one[1]) and torch.equal(_bits(grad), _bits(one[3]))


@pytest.mark.parametrize('Rs_per_ds', gs.SCALES)
@pytest.mark.parametrize('time_mode', dynamic.MODES)
@pytest.mark.parametrize('name', gs.SPHERES)
def test_dynamic_sphere_seams(name, time_mode, Rs_per_ds):
    c = 3
    cs = gs.dynamic_sphere_case(name, time_mode, Rs_per_ds)
    raw, ids, weights, grad = run_points(cs, c, with_time=True, Rs_per_ds=Rs_per_ds)
    m = cs['n_space']
    n_decided = N_AXIS + gs.special_points().shape[0]
    decided = (torch.arange(cs['points'].shape[0]) % m) < n_decided
    units = check_forward(cs, c, raw, ids, decided=decided)
    for k, t in enumerate(gs.SPHERE_TIMES.tolist()):
        if time_mode == 'clamp' or t <= gs.SPHERE_TAU[-1]:
            part = dict(cs, points=cs['points'][k * m:(k + 1) * m], inside=cs['inside'][k * m:(k + 1) * m])
            _check_axis_points(name, raw[k * m:(k + 1) * m], ids[k * m:(k + 1) * m], weights[k * m:(k + 1) * m], part)
    # the temporal weights of the five times, on a point inside: (1, 0) on the first frame, fp32(0.1) just inside interval 1
    p = int(torch.nonzero(cs['inside'][:m])[0])
    wt = weights[p::m, 6:8].tolist()
    s01 = (float(gs.SPHERE_TIMES[1]) - 0.1) / (0.3 - 0.1)
    assert wt[0] == [1.0, 0.0] and wt[1] == [1.0, torch.tensor(s01).float().item()] and wt[2] == [0.5, 0.5]
    assert wt[4] == ([0.0, 1.0] if time_mode == 'clamp' else [0.0, 0.0])
    worst = check_backward(cs, c, grad, gs.DYNAMIC_SLACK)
    print(f'dynamic grid sphere {name} {time_mode} Rs_per_ds={Rs_per_ds}: {int(cs["inside"].sum())} of {cs["inside"].shape[0]} '
          f'points inside, forward {units:.3f} gate units, worst node at {worst:.3f} of its bound')
    assert units <= 1.0 and worst <= 1.0
