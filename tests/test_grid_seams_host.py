"""CPU-only checks of the case builders of tests/grid_seams.py (no GPU): every constructed layout of the inverted index has the
counts of its table and really holds the seam it is named for, the exact mode is exact (integer arithmetic reproduces the fp64
gradient), the points on the sphere's seams are decided as the IEEE rules say, and ``node_terms`` of the two reference modules
is what the bound per node needs."""
import math

import pytest
import torch

import dynamic_grid_reference as dref
import grid_field_reference as sref
import grid_seams as gs


# ---- layouts ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(gs.LAYOUTS))
def test_static_layout_has_its_counts_and_its_seams(name):
    counts, n_outside, named = gs.LAYOUTS[name]
    assert named and named <= gs.seams(counts, n_outside), (name, named - gs.seams(counts, n_outside))
    for mode in gs.MODES:
        cs = gs.static_layout(name, mode)
        m = sum(counts) + n_outside
        assert cs['points'].shape == (m, 3) and m < 1500
        table = list(counts) + [0] * (gs.N_CELLS - len(counts)) + [n_outside]
        assert torch.bincount(cs['ids'], minlength=gs.N_CELLS + 1).tolist() == table
        assert torch.equal(cs['inside'], cs['ids'] < gs.N_CELLS)
        # the input order is shuffled: the sort of the backward has work to do
        if m > 8 and len([c for c in counts if c]) + (n_outside > 0) > 1:
            assert not bool((cs['ids'][1:] >= cs['ids'][:-1]).all())


def test_the_probed_layout_has_its_917_samples():
    counts, n_outside, _ = gs.LAYOUTS['probe']
    assert len(counts) == 24 and sum(counts) == 917 and n_outside == 0
    assert counts[:12] == [63, 64, 65, 1, 130, 62, 66, 0, 129, 64, 200, 3] and counts[12:] == [0] * 11 + [70]
    for mode, build in (('static', gs.static_layout), ('dynamic', lambda n, m: gs.dynamic_layout(n + '@0', m))):
        cs = build('probe', 'exact')
        assert torch.equal(cs['points'].double(), cs['p64']), mode                          # the points are exact in fp32
        if mode == 'dynamic':
            s = dref.locate_time(cs['tau'], cs['points'][:, 3])[1]
            assert bool(((s * 4) % 1 == 0).all())                                           # every weight in time a multiple of 1/4


def test_every_seam_is_named_by_some_layout():
    named = set().union(*(s for _, _, s in gs.LAYOUTS.values()))
    assert named >= {'len63', 'len64', 'len65', 'long_starts_inside_a_piece', 'long_ends_on_a_boundary', 'two_long_ids_in_a_piece',
                     'short_between_two_longs', 'long_shares_its_last_piece_with_the_sentinel', 'total_64k', 'total_256k_plus_1',
                     'long_in_the_last_id', 'first_id_empty'}


@pytest.mark.parametrize('name', gs.DYNAMIC_LAYOUTS)
def test_dynamic_layout_has_its_counts(name):
    n_frames, counts, n_outside = gs.dynamic_table(name)
    n_ids = (n_frames - 1) * gs.N_CELLS
    assert len(counts) == n_ids
    base = name.split('@')[0]
    assert sum(counts) == sum(gs.LAYOUTS[base][0]) * (2 if name.endswith('@1+2') else 1)
    for mode in gs.MODES:
        cs = gs.dynamic_layout(name, mode)
        assert cs['points'].shape == (sum(counts) + n_outside, 4) and cs['points'].shape[0] < 1500
        assert torch.bincount(cs['ids'], minlength=n_ids + 1).tolist() == list(counts) + [n_outside]
        assert cs['values'].shape[0] == n_frames == len(cs['tau'])


@pytest.mark.parametrize('base', ['63_65', '1_200', '63_129', '10_118', '64_128'])
def test_two_interval_layouts_pair_a_long_with_a_short_segment_on_one_cell(base):
    _, counts, _ = gs.dynamic_table(base + '@1+2')
    lower, upper = counts[gs.N_CELLS:2 * gs.N_CELLS], counts[2 * gs.N_CELLS:3 * gs.N_CELLS]
    # frame 2 is the upper frame of interval 1 and the lower frame of interval 2
    assert any(a > gs.CHUNK >= b > 0 for a, b in zip(lower, upper)), 'no cell: long as the upper frame, short as the lower'
    assert any(b > gs.CHUNK >= a > 0 for a, b in zip(lower, upper)), 'no cell: short as the upper frame, long as the lower'


def _integer_gradient(cs, with_time):
    """The adjoint of an exact-mode layout in int64: weights as numerators over 4, g_raw as integers."""
    grid = cs['grid']
    pts = cs['points']
    i0, i1, t, inside = sref.locate(grid, sref.grid_coordinates(grid, pts), 'patch')
    q = (t * 4).round().long()
    assert torch.equal(q.double()[inside] / 4, t[inside]) and bool(((q[inside] >= 1) & (q[inside] <= 3)).all())
    g = cs['g_raw'].long()
    assert torch.equal(g.float(), cs['g_raw']) and int(g.abs().max()) <= 8
    n0, n1, n2 = grid.shape
    if with_time:
        j, s, inside_t = dref.locate_time(cs['tau'], pts[:, 3], 'clamp')
        qs = (s * 4).round().long()
        inside = inside & inside_t
        assert torch.equal(qs.double()[inside] / 4, s[inside])
        n_frames = len(cs['tau'])
    else:
        j, qs, n_frames = torch.zeros_like(q[:, 0]), None, 1
    out = torch.zeros(n_frames * n0 * n1 * n2, 4, dtype=torch.long)
    for dt in ((0, 1) if with_time else (0,)):
        for d0 in (0, 1):
            for d1 in (0, 1):
                for d2 in (0, 1):
                    w = torch.ones_like(q[:, 0])
                    for k, d in enumerate((d0, d1, d2)):
                        w = w * (q[:, k] if d else 4 - q[:, k])
                    if with_time:
                        w = w * (qs if dt else 4 - qs)
                    idx = [(i1 if d else i0)[:, k] for k, d in enumerate((d0, d1, d2))]
                    flat = ((((j + dt) * n0 + idx[0]) * n1 + idx[1]) * n2 + idx[2])[inside]
                    out.index_add_(0, flat, (w[:, None] * g)[inside])
    return out.reshape(cs['grad'].shape), 256 if with_time else 64


@pytest.mark.parametrize('name', list(gs.LAYOUTS))
def test_exact_mode_is_exact(name):
    """Integer arithmetic reproduces the fp64 gradient, every term and every possible partial sum is a multiple of 1 / 256
    below 2^24 / 256 (so fp32 adds them exactly in any order), and the fp32 points and times are the intended ones."""
    cases = [(gs.static_layout(name, 'exact'), False)]
    cases += [(gs.dynamic_layout(n, 'exact'), True) for n in gs.DYNAMIC_LAYOUTS if n.split('@')[0] == name]
    assert len(cases) >= 2
    for cs, with_time in cases:
        assert torch.equal(cs['points'].double()[cs['inside']], cs['p64'][cs['inside']])
        want, denominator = _integer_gradient(cs, with_time)
        assert torch.equal(cs['grad'] * denominator, want.double())
        assert float((cs['terms'] * denominator).max()) < 2 ** 24              # sum |w||g|: no partial sum can leave fp32's integers
        assert torch.equal(cs['grad'].float().double(), cs['grad'])


def test_random_mode_keeps_every_sample_in_its_cell_after_rounding():
    for name in ('probe', '70_5_70'):
        cs = gs.static_layout(name, 'random')
        assert torch.equal(gs.cell_ids(cs['grid'], cs['points']), gs.cell_ids(cs['grid'], cs['p64'].float()))
        u = sref.grid_coordinates(cs['grid'], cs['points'])
        _, _, t, inside = sref.locate(cs['grid'], u)
        assert bool(((t[inside] > 0.04) & (t[inside] < 0.96)).all())


@pytest.mark.parametrize('with_time', [False, True])
def test_wrap_layout_has_two_long_segments_in_wrap_cells(with_time):
    cs = gs.wrap_layout(with_time)
    grid = cs['grid']
    n1 = grid.shape[1]
    nc = gs.cells_per_axis(grid, 'open')
    assert nc[1] == n1                                                         # an open longitude: one cell per node
    ids = gs.wrap_cell_ids(grid, with_time)
    counts = torch.bincount(cs['ids'])
    assert [int(counts[i]) for i in ids] == [65, 200] and int(counts[-1]) == 20 and int(counts.sum()) == 285
    cells = torch.tensor(ids) % (nc[0] * nc[1] * nc[2])
    assert bool((((cells // nc[2]) % nc[1]) == n1 - 1).all())                  # i1 = n1 - 1
    u = sref.grid_coordinates(grid, cs['points'], 1.0, 'open')
    assert bool((u[cs['inside'], 1] > grid.axes[1][-1]).all())


# ---- node_terms -------------------------------------------------------------------------------------------------------------
def test_node_terms_bound_the_gradient_and_count_the_samples():
    cs = gs.static_layout('probe', 'random')
    assert bool((cs['grad'].abs() <= cs['terms'] * (1 + 1e-12)).all())
    assert int(cs['count'].sum()) == 8 * 917
    # with g = 1 and positive weights the terms are the gradient
    ones = torch.ones_like(cs['g_raw'])
    terms, count = sref.node_terms(cs['grid'], cs['points'], ones)
    leaf = torch.zeros(*cs['grid'].shape, 4, dtype=torch.float64, requires_grad=True)
    sref.field(cs['grid'], leaf, cs['points'], gs.FILL)[0].sum().backward()
    assert torch.allclose(terms, leaf.grad, rtol=1e-13, atol=0) and torch.equal(count, cs['count'])
    cd = gs.dynamic_layout('probe@0', 'random')
    assert bool((cd['grad'].abs() <= cd['terms'] * (1 + 1e-12)).all())
    assert int(cd['count'].sum()) == 16 * 917 and cd['count'].shape == (5, 5, 4, 3)
    assert int(cd['count'][2:].sum()) == 0                                     # interval 0 touches frames 0 and 1 only


def test_node_check_bites():
    cs = gs.static_layout('70_5_70', 'random')
    good = cs['grad'].float()
    assert gs.node_check(good, cs['grad'], cs['terms'], cs['count'], gs.STATIC_SLACK) <= 1.0
    touched = torch.nonzero(cs['count'] > 0)[0]
    bad = good.clone()
    bad[tuple(touched)] *= 1 + 1e-4                                            # one node off by 1e-4: invisible in the tensor's L2
    assert ((bad.double() - cs['grad']).norm() / cs['grad'].norm()).item() < 1e-3
    assert gs.node_check(bad, cs['grad'], cs['terms'], cs['count'], gs.STATIC_SLACK) > 1.0
    stray = good.clone()
    stray[tuple(torch.nonzero(cs['count'] == 0)[0])] = 1e-30
    with pytest.raises(AssertionError):
        gs.node_check(stray, cs['grad'], cs['terms'], cs['count'], gs.STATIC_SLACK)


# ---- the sphere -------------------------------------------------------------------------------------------------------------
def test_sphere_grids_are_read_as_closed_open_and_patch():
    from sunerf_hip.grid_field import LON_NAMES, longitude_mode
    for name in gs.SPHERES:
        grid = gs.sphere_grid(name)
        assert LON_NAMES[longitude_mode(grid)] == gs.SPHERE_LON[name]
        assert grid.axes[2].tolist() == [1.0, 1.25, 1.5, 2.0]
    assert gs.sphere_grid('full_open_to_zero').axes[1][-1].item() == 0.0 and gs.sphere_grid('full_open_to_zero').shape[1] == 8
    lat, lon, _ = gs.sphere_grid('full_open').axes
    assert lat[0].item() == -math.pi / 2 and lat[-1].item() == math.pi / 2 and lat[2].item() == 0.0
    assert lon[0].item() == -math.pi and lon[4].item() == 0.0 and lon[2].item() == -math.pi / 2


def test_axis_points_are_decided_exactly():
    pts = gs.axis_points()
    radii, shell = gs.axis_radii()
    assert pts.shape == (168, 3) and radii.shape == (7,)
    idx = torch.arange(168)
    direction, radius = idx // 28, (idx // 4) % 7
    assert torch.equal(pts.double().norm(dim=1), radii.double()[radius])       # the root is exact
    assert int((pts == 0).sum()) == 2 * 168 and int(torch.signbit(pts[pts == 0]).sum()) == 168
    positive_axes = (direction % 2) == 0                                       # +x, +y, +z: 84 of the 168 points
    for name, n_inside, n_positive in (('full_closed', 120, 60), ('full_open', 120, 60), ('patch', 70, 40),
                                         ('full_open_to_zero', 120, 60)):
        grid, lon = gs.sphere_grid(name), gs.SPHERE_LON[name]
        u = sref.grid_coordinates(grid, pts, 1.0, lon)
        i0, i1, t, inside = sref.locate(grid, u, lon)
        assert int(inside.sum()) == n_inside and int(inside[positive_axes].sum()) == n_positive, name
        assert torch.equal(u[:, 2], radii.double()[radius])
        if name != 'patch':
            assert torch.equal(inside, torch.tensor(shell)[radius])
            # latitude: 0 on the four equatorial directions, +-pi/2 at the poles (asin(+-1)); longitude: on a node, +pi folded
            # onto lon[0] = -pi exactly
            assert torch.equal(u[:, 0].abs(), (direction >= 4).double() * (math.pi / 2))
            lon0 = grid.axes[1][0].item()
            assert bool((u[:, 1] >= lon0).all()) and bool((u[:, 1] < lon0 + sref.TWO_PI).all())
            on_node = (u[:, 1:2] == grid.axes[1][None, :]).any(1)
            assert bool(on_node.all())
            assert bool(((t[inside][:, :2] == 0) | (t[inside][:, :2] == 1)).all())
            # both signs of a zero: the same cell and weights on the equatorial directions; at a pole the longitude is
            # atan2(-+0, +-0) = 0 or pi by the sign of y alone
            cells = gs.cell_ids(grid, pts, 1.0, lon).reshape(6, 7, 4)
            tt = t.reshape(6, 7, 4, 3)
            assert bool((cells[:4] == cells[:4, :, :1]).all()) and bool((tt[:4] == tt[:4, :, :1]).all())
            same_y = ((0, 2), (1, 3))                                          # ZERO_SIGNS: (x, y) = (+,+) (+,-) (-,+) (-,-)
            for a, b in same_y:
                assert torch.equal(cells[4:, :, a], cells[4:, :, b]) and torch.equal(tt[4:, :, a], tt[4:, :, b])
            assert not torch.equal(cells[4:, :, 0], cells[4:, :, 1])
            if name == 'full_open_to_zero':                                    # +y: u == lon[-1] exactly, the last ordinary cell
                plus_y = inside & (direction == 2)
                assert bool((u[plus_y, 1] == 0.0).all()) and bool((i0[plus_y, 1] == 6).all()) and bool((t[plus_y, 1] == 1).all())
        else:
            # the patch: -y is at lon = +-pi, +z at lat = -pi/2: outside; -z is inside where y = +0 (lon = -+0), outside where
            # y = -0 (lon = -+pi) -- the IEEE rule for atan2 of two zeros
            got = inside.reshape(6, 7, 4)[:, 0].tolist()
            assert got == [[True] * 4, [True] * 4, [True] * 4, [False] * 4, [False] * 4, [True, False, True, False]]


def test_special_and_continuity_points():
    sp = gs.special_points()
    assert sp[8, 2].item() > 0 and sp[9, 2].item() < 0                          # fp32 holds 1e-30
    for name in gs.SPHERES:
        cs = gs.sphere_case(name)
        n_axis = 168
        inside = cs['inside'][n_axis:n_axis + sp.shape[0]]
        assert not bool(inside[:gs.N_SPECIAL_OUTSIDE].any())                    # r = 0, NaN
        if name == 'patch':
            assert inside[gs.N_SPECIAL_OUTSIDE:].tolist() == [False, True, False, True]      # the lat = 0 face: by the sign of z
        else:
            assert bool(inside[gs.N_SPECIAL_OUTSIDE:].all())
            cont = cs['inside'][n_axis + sp.shape[0]:]
            assert cont.shape[0] == 18 * 4 + 40 and bool(cont.all())
            u = sref.grid_coordinates(cs['grid'], cs['points'][n_axis + sp.shape[0]:], 1.0, cs['lon'])
            lon0 = cs['grid'].axes[1][0].item()
            near = torch.minimum(u[:36, 1] - lon0, lon0 + sref.TWO_PI - u[:36, 1])
            assert bool((near > 0).all()) and bool((near < 1e-6).all())
            assert bool((u[:18, 1] - lon0 < 1e-6).all()) and bool((lon0 + sref.TWO_PI - u[18:36, 1] < 1e-6).all())
            pole = math.pi / 2 - u[36:72, 0].abs()
            assert bool((pole > 0).all()) and bool((pole < 1e-6).all())


def test_scaled_points_give_the_same_decisions_and_weights():
    for name in gs.SPHERES:
        one, quarter = gs.sphere_case(name, 1.0), gs.sphere_case(name, 0.25)
        finite = torch.isfinite(one['points'])
        assert torch.equal((quarter['points'] * 0.25)[finite], one['points'][finite])
        assert torch.equal(one['ids'], quarter['ids']) and torch.equal(one['grad'], quarter['grad'])
        assert torch.equal(one['raw'], quarter['raw'])


def test_dynamic_sphere_times_are_decided_exactly():
    t = gs.SPHERE_TIMES.double()
    assert t[1].item() > 0.1 and t[4].item() > 0.3                              # fp32(0.1) > 0.1, fp32(0.3) > 0.3
    for mode in ('clamp', 'fill'):
        j, s, inside = dref.locate_time(gs.SPHERE_TAU, gs.SPHERE_TIMES, mode)
        assert j.tolist() == ([0, 1, 0, 1, 1] if mode == 'clamp' else [0, 1, 0, 1, 0])
        assert inside.tolist() == [True, True, True, True, mode == 'clamp']
        assert s[0].item() == 0.0 and 0 < s[1].item() < 1e-7 and (s[4].item() == 1.0 if mode == 'clamp' else True)
        cs = gs.dynamic_sphere_case('full_open', mode)
        m = cs['n_space']
        space = gs.sphere_case('full_open')['inside']
        assert torch.equal(cs['inside'].reshape(5, m), space[None, :] & inside[:, None])


def test_scaled_rays_stay_clear_of_the_faces():
    for name in gs.SCALED_GRIDS:
        cs = gs.scaled_rays_case(name)
        assert cs['Rs'] == 0.7 and cs['count'].sum() > 0
