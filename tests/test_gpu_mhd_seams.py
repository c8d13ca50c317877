"""The MHD cube field on MI355X (csrc/mhd.hip: ``mhd_field_kernel``) where its decisions are discontinuous: points ON grid
nodes, on the first and last node of an axis and one fp32 step beside them, at phi = 0, pi / 2, pi, 3 pi / 2 and on the polar
axis, at times on and one fp32 step beside a frame boundary, with one frame of a pair on a narrower cube -- against the
fp64 restatement of the reference's MHDModel (tests/mhd_reference.py).

Only points whose reference fp32 (r, theta, phi) are the intended node values bit for bit enter the exact assertions (the
host's ``torch.sqrt`` is not the IEEE one); the counts are printed and asserted.  The bounds are the project's own
(``_check_field`` of tests/test_gpu_mhd.py): 2e-5 on ln rho and log10 T, 1e-6 on the fill pair.

Measured on MI355X: all 512 seam points qualify (axis 336, r-edge 128, diagonal 32, nan 8, origin 8; 56 inside one frame of
their pair only); NaN and fill masks equal (380 interpolated, 116 filled, 16 NaN); max |err| ln rho 1.9e-6, log10 T 4.8e-7, fill 0;
198 points on a node of all three axes at an exact frame time within 1.9e-6 of the logarithm of the node's own data; rays mode
bit-equal to points mode.  Nodes in general position (180 points): 1.9e-6 / 4.8e-7.  fp64 grid held in fp32 (2000 points):
4.3e-6 / 4.8e-7.  Cell choice at a node (126 points, 19 NaN in the reference): masks equal.  Scratch builds: an exclusive upper
r bound (``<`` for ``<=``) fails the seam-point fill mask; ``g[i] > x`` for ``>=`` in ``find_cell`` fails the cell-choice test and
nothing else in the suite (the field is continuous across a node, so the choice shows only beside a non-finite node)."""
import collections

import numpy as np
import pytest
import torch

import mhd_reference as ref

pytestmark = pytest.mark.gpu

FFIRST, FLAST = 10, 12
TOL, TOL_FILL = 2e-5, 1e-6            # test_gpu_mhd._check_field
FILL = torch.tensor([np.log(np.float32(1e-10)), np.log10(np.float32(1e6) * np.float32(1e-10))], dtype=torch.float32)


def _model(tmp_path, frames):
    from sunerf.model.mhd_model import MHDModel
    root = ref.write_placeholders(tmp_path / 'run', sorted(frames))
    return MHDModel(root, reader=ref.DictReader(frames)).cuda()


def _check(got, want, what, select=None):
    """NaN mask and fill mask equal the reference's exactly; the fill pair within 1e-6, everything else within 2e-5."""
    got = got.detach().cpu()
    select = torch.ones(want.shape[0], dtype=torch.bool) if select is None else torch.as_tensor(select)
    got, want = got[select], want[select]
    nan = torch.isnan(want)
    assert torch.equal(nan[:, 0], nan[:, 1])
    assert torch.equal(torch.isnan(got), nan), (what, 'NaN mask')
    is_fill = (want == FILL).all(-1)
    got_fill = ((got - FILL).abs() <= TOL_FILL).all(-1)
    assert torch.equal(got_fill, is_fill), (what, 'fill mask', torch.nonzero(got_fill != is_fill).reshape(-1)[:8].tolist())
    inside = ~is_fill & ~nan[:, 0]
    err = (got[inside] - want[inside]).abs().max(0).values if inside.any() else torch.zeros(2)
    err_fill = (got[is_fill] - want[is_fill]).abs().max().item() if is_fill.any() else 0.
    print(f'{what}: {int(inside.sum())} interpolated, {int(is_fill.sum())} filled, {int(nan[:, 0].sum())} NaN; '
          f'max |err| ln rho {err[0]:.2e}, log10 T {err[1]:.2e} (bound {TOL:.0e}), fill {err_fill:.1e} (bound {TOL_FILL:.0e})')
    assert err_fill <= TOL_FILL, what
    assert (err <= TOL).all(), (what, err)
    return inside, is_fill


def test_points_on_nodes_bounds_and_frame_boundaries(tmp_path):
    frames = {10: ref.seam_frame(1), 11: ref.seam_frame(2, r_nodes=ref.SEAM_R_NARROW), 12: ref.seam_frame(3)}
    pts, cat, intended = ref.seam_cases()
    assert not np.signbit(pts.numpy()[pts.numpy() == 0]).any()                 # zeros are +0
    want, coords, (f1, f2, w), inb = ref.mhd_field_parts(pts, frames, FFIRST, FLAST)
    # preconditions, on the reference alone
    q = ref.qualifying(coords, intended)
    cat = np.array(cat)
    counts = collections.Counter(cat[q].tolist())
    half = (inb[:, 0] ^ inb[:, 1]).numpy() & q
    print(f'seam points: {int(q.sum())} of {q.size} qualify {dict(counts)}; {int(half.sum())} inside one frame of their pair only')
    assert q.sum() >= 40 and all(counts[c] > 0 for c in ('axis', 'r-edge', 'diagonal', 'nan', 'origin')), counts
    assert half.sum() > 0 and set(w.tolist()) == {0., 0.5}
    assert {(int(a), int(b)) for a, b in zip(f1, f2)} == {(10, 10), (10, 11), (11, 11), (11, 12), (12, 12)}
    edge = q & (cat == 'r-edge')
    ok_edge = ~torch.isnan(want[:, 0]).numpy() & edge
    assert (inb.any(1).numpy() & ok_edge).any() and (~inb.any(1).numpy() & ok_edge).any()    # one step inside and one outside

    model = _model(tmp_path, frames)
    got = model(pts.cuda())['inferences']
    inside, is_fill = _check(got, want, 'seam points', select=q)
    assert inside.sum() >= 100 and is_fill.sum() >= 40
    got = got.cpu()

    # a node of all three axes at an exact frame time: the logarithm of that node's own data
    checked, worst = 0, 0.
    for i in np.nonzero(q & (cat == 'axis') & (w.numpy() == 0.))[0]:
        r, th, phi, rho, temp = frames[int(f1[i])]
        axes, x = (phi, th, r), intended[i][::-1]
        node = tuple(int(np.searchsorted(a, v)) for a, v in zip(axes, x))
        if not all(k < a.size and a[k] == v for k, a, v in zip(node, axes, x)):
            assert torch.equal(want[i], FILL)                                  # frame 11 has no node at this radius: filled
            continue
        direct = torch.stack([torch.log(torch.tensor(rho[node], dtype=torch.float64).to(torch.float32)),
                              torch.log10(1e6 * torch.tensor(temp[node], dtype=torch.float64).to(torch.float32))])
        assert torch.equal(want[i], direct), (i, want[i], direct)
        worst = max(worst, (got[i] - direct).abs().max().item())
        checked += 1
    print(f'nodes of all three axes at exact frame times: {checked} points, max |err| against the node\'s own data {worst:.2e}')
    assert checked >= 100 and worst <= TOL

    # rays mode, o = 0, d = (1, 0, 0), z = the radii of the +x points: the same bits as points mode
    on_x = [i for i in range(0, pts.shape[0], len(ref.SEAM_TIMES)) if pts[i, 0] > 0 and pts[i, 1] == 0 and pts[i, 2] == 0]
    z = torch.cat([pts[on_x, 0], torch.tensor([0., float('nan')])])
    nt = len(ref.SEAM_TIMES)
    t = torch.tensor(ref.SEAM_TIMES, dtype=torch.float32)[:, None]
    o = torch.zeros(nt, 3)
    d = torch.tensor([[1., 0., 0.]]).expand(nt, 3).contiguous()
    raw = model.field_on_rays(o.cuda(), d.cuda(), z[None].expand(nt, -1).contiguous().cuda(), t.cuda()).cpu()
    p = torch.zeros(nt, z.numel(), 4)
    p[..., 0] = z
    p[..., 3] = t
    same = model(p.reshape(-1, 4).cuda())['inferences'].cpu().reshape(nt, z.numel(), 2)
    assert torch.isnan(raw[:, -2:]).all() and not torch.isnan(raw[:, :-2]).any()
    assert torch.equal(torch.isnan(raw), torch.isnan(same))
    assert torch.equal(raw.nan_to_num(nan=0.).view(torch.int32), same.nan_to_num(nan=0.).view(torch.int32))
    by_point = got.reshape(-1, nt, 2)[[i // nt for i in on_x]].transpose(0, 1)
    assert torch.equal(raw[:, :-2].view(torch.int32), by_point.contiguous().view(torch.int32))


def test_cell_choice_at_a_node_is_scipys(tmp_path):
    """Which of the two cells that share a node is taken shows only when a neighbouring node is not finite: scipy takes the
    cell BELOW a node it is on (``searchsorted(grid, x) - 1``), whose weights are (0, 1); with an Inf two nodes down the axis
    the cell above would give 0 * Inf = NaN.  One frame per axis carries an Inf plane at node index 4: points on node 3 are
    finite in the reference, points on nodes 4 and 5 are NaN (their cell below touches the plane: 0 * Inf).  The axis
    points reach r nodes 3, 4, 5, phi nodes 3 (pi / 2) and 5 (pi), and theta node 3 (pi / 2)."""
    frames = {}
    for f, axis in ((10, 2), (11, 1), (12, 0)):               # data[i_phi, i_theta, i_r]
        r, th, phi, rho, temp = ref.seam_frame(30 + f)
        index = [slice(None)] * 3
        index[axis] = 4
        rho[tuple(index)] = np.inf
        temp[tuple(index)] = np.inf
        frames[f] = (r, th, phi, rho, temp)
    assert (frames[10][0][4], frames[11][1][3], frames[12][2][3], frames[12][2][5]) == (1.25, ref.HALF_PI32, ref.HALF_PI32, ref.PI32)
    xyz, cat, intended = ref.seam_points()
    keep = [i for i, c in enumerate(cat) if c == 'axis']
    times = torch.tensor([0., 0.5, 1.])
    pts = torch.cat([xyz[keep][:, None, :].expand(-1, 3, -1), times[None, :, None].expand(len(keep), -1, 1)], -1).reshape(-1, 4)
    pts = pts.contiguous()
    with np.errstate(invalid='ignore'):
        want, coords, (f1, f2, w), inb = ref.mhd_field_parts(pts, frames, FFIRST, FLAST)
    assert ref.qualifying(coords, np.repeat(intended[keep], 3, 0)).all() and inb.all() and not w.any()
    outcomes = {f: (int(torch.isfinite(want[f1 == f]).all(1).sum()), int(torch.isinf(want[f1 == f]).all(1).sum()),
                    int(torch.isnan(want[f1 == f]).all(1).sum())) for f in (10, 11, 12)}
    print('cell choice at a node, reference (finite, Inf, NaN) per frame:', outcomes)
    assert outcomes == {10: (30, 0, 12), 11: (42, 0, 0), 12: (35, 0, 7)}, outcomes
    got = _model(tmp_path, frames)(pts.cuda())['inferences'].cpu()
    finite = torch.isfinite(want)
    print(f'cell choice at a node: {int(finite.all(1).sum())} finite, {int(torch.isinf(want).all(1).sum())} Inf, '
          f'{int(torch.isnan(want).all(1).sum())} NaN; max |err| {(got[finite] - want[finite]).abs().max().item():.2e} (bound {TOL:.0e})')
    assert torch.equal(torch.isnan(got), torch.isnan(want)), torch.nonzero(torch.isnan(got) != torch.isnan(want))[:8].tolist()
    assert torch.equal(got[torch.isinf(want)], want[torch.isinf(want)])
    assert torch.equal(torch.isfinite(got), finite) and ((got[finite] - want[finite]).abs() <= TOL).all()


def test_nodes_in_general_position(tmp_path):
    """Every point on a theta node and a phi node (the grids are built from the reference's own fp32 angles of the points):
    the device's acosf / atan2f land on, just below or just above the node, which runs both equality branches of the cell
    search's walk; the field is continuous across a node, so the project's bound holds whichever cell is taken."""
    gen = torch.Generator().manual_seed(4)
    n = 60
    d = torch.randn(n, 3, generator=gen)
    xyz = d / d.norm(dim=1, keepdim=True) * (1.05 + 0.85 * torch.rand(n, 1, generator=gen))
    frames = dict(zip((10, 11), ref.general_position_frames(xyz)))
    times = torch.tensor([0., 0.4, 1.])
    pts = torch.cat([xyz[:, None, :].expand(-1, 3, -1), times[None, :, None].expand(n, -1, 1)], -1).reshape(-1, 4).contiguous()
    want, (r, th, phi), _, inb = ref.mhd_field_parts(pts, frames, 10, 11)
    fr = frames[10]
    assert np.isin(th.numpy().astype(np.float64), fr[1][1:-1]).all() and np.isin(phi.numpy().astype(np.float64), fr[2][1:-1]).all()
    assert inb.all()
    for v, axis in ((r, fr[0]), (th, fr[1]), (phi, fr[2])):
        assert (v.numpy() - axis[0]).min() > 1e-4 and (axis[-1] - v.numpy()).min() > 1e-4      # no point within 1e-4 of a bound
    got = _model(tmp_path, frames)(pts.cuda())['inferences']
    inside, is_fill = _check(got, want, 'theta and phi nodes in general position')
    assert inside.all()


def test_fp64_grid_that_fp32_cannot_hold(tmp_path):
    """The model keeps fp32 copies of the grids (``astype(np.float32)`` in ``MHDModel.load_frame``); the reference interpolates
    on the fp64 grids as they are read.  Points more than 1e-5 inside the bounds, so that both agree on where the cube ends."""
    frames = {10: ref.unrounded_frame(5), 11: ref.unrounded_frame(6)}
    rng = np.random.default_rng(8)
    n = 2000
    r, th, phi, _, _ = frames[10]
    c = [rng.uniform(a[0] + 1e-3, a[-1] - 1e-3, n) for a in (r, th, phi)]
    xyz = np.stack([c[0] * np.sin(c[1]) * np.cos(c[2]), c[0] * np.sin(c[1]) * np.sin(c[2]), c[0] * np.cos(c[1])], 1)
    t = np.array([0., 0.3, 0.5, 1.])[rng.integers(0, 4, n)]
    pts = torch.from_numpy(np.concatenate([xyz, t[:, None]], 1)).float().contiguous()
    want, (rr, tt, pp), _, inb = ref.mhd_field_parts(pts, frames, 10, 11)
    for v, axis in ((rr, r), (tt, th), (pp, phi)):
        v = v.numpy().astype(np.float64)
        assert (v - axis[0]).min() > 1e-5 and (axis[-1] - v).min() > 1e-5
    assert inb.all()
    got = _model(tmp_path, frames)(pts.cuda())['inferences']
    inside, _ = _check(got, want, 'fp64 grid held in fp32')
    assert inside.all()
