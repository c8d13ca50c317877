"""CPU checks of what the MHD seam tests (tests/test_gpu_mhd_seams.py) stand on: ``mhd_reference.mhd_field_parts`` is
``mhd_reference.mhd_field`` with its intermediates, the seam frames are what they claim to be, and on this host the
reference's fp32 coordinates of the seam points are the intended node values bit for bit (measured: all 512 points qualify)."""
import collections

import numpy as np
import torch

import mhd_reference as ref

FFIRST, FLAST = 10, 12


def seam_frames():
    return {10: ref.seam_frame(1), 11: ref.seam_frame(2, r_nodes=ref.SEAM_R_NARROW), 12: ref.seam_frame(3)}


def _same(a, b):
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a.nan_to_num(nan=0.), b.nan_to_num(nan=0.))


def test_parts_variant_is_the_field_on_the_existing_frames():
    frames = {10: ref.synthetic_frame(1),
              11: ref.synthetic_frame(2, n_phi=19, n_theta=21, n_r=33, r_range=(1.03, 1.35), phi_end=0.93 * 2 * np.pi),
              12: ref.synthetic_frame(3)}
    gen = torch.Generator().manual_seed(1)
    n = 3000
    d = torch.randn(n, 3, generator=gen)
    d = d / d.norm(dim=1, keepdim=True)
    rad = 0.9 + 0.6 * torch.rand(n, 1, generator=gen)
    t = torch.tensor([0.0, 0.5, 1.0, 0.3, 0.8, float('nan')])[torch.randint(6, (n,), generator=gen)]
    pts = torch.cat([d * rad, t[:, None]], 1).float()
    pts[7, 0] = float('nan')
    pts[8, :3] = 0.
    want = ref.mhd_field(pts, frames, FFIRST, FLAST)
    got, (r, th, phi), (f1, f2, w), inside = ref.mhd_field_parts(pts, frames, FFIRST, FLAST)
    assert _same(got, want)
    r2, th2, phi2 = ref.spherical(pts.clone())
    assert _same(r, r2) and _same(th, th2) and _same(phi, phi2)
    # the in-bounds mask says where the fill value comes from: both frames outside <=> the fill pair
    fill = torch.tensor([np.log(np.float32(1e-10)), np.log10(np.float32(1e6) * np.float32(1e-10))], dtype=torch.float32)
    ok = ~torch.isnan(want).any(1)
    assert torch.equal((want == fill).all(1)[ok], ~inside.any(1)[ok])
    assert 0 < int((inside[:, 0] ^ inside[:, 1]).sum())           # frame 11's narrower cube: inside one frame of a pair only
    assert not inside[torch.isnan(t)].any()


def test_seam_frames_are_what_they_claim():
    frames = seam_frames()
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)     # noqa: E731
    for f, (r, th, phi, rho, temp) in frames.items():
        for a in (r, th, phi):
            assert np.array_equal(a, f32(a)) and (np.diff(a) > 0).all()
        assert rho.min() > 0 and temp.min() > 0 and rho.shape == (phi.size, th.size, r.size)
        assert th[0] == 0 and th[-1] == np.float32(np.pi) and np.float32(np.pi / 2) in th
        assert phi[0] == 0 and phi[-1] == np.float32(2 * np.pi)
        assert all(v in phi for v in (np.float32(np.pi / 2), np.float32(np.pi), np.float32(-np.pi / 2) + np.float32(2 * np.pi)))
    assert tuple(frames[10][0]) == (1.0, 1.03125, 1.0625, 1.125, 1.25, 1.5, 2.0) and tuple(frames[11][0]) == (1.0625, 1.125, 1.25, 1.5)
    assert ref.SEAM_TIMES[2] < 0.5 < ref.SEAM_TIMES[4] and ref.SEAM_TIMES[6] < 1 and len(ref.SEAM_TIMES) == 8
    # an fp64 grid that fp32 cannot hold
    r, th, phi, _, _ = ref.unrounded_frame(5)
    assert all((a != f32(a)).mean() > 0.8 for a in (r, th, phi))


def test_seam_preconditions_hold_on_this_host():
    """The reference's fp32 (r, theta, phi) of the seam points equal the intended node values bit for bit: at least 40
    points, and at least one of every category."""
    frames = seam_frames()
    pts, cat, intended = ref.seam_cases()
    out, coords, (f1, f2, w), inside = ref.mhd_field_parts(pts, frames, FFIRST, FLAST)
    q = ref.qualifying(coords, intended)
    counts = collections.Counter(np.array(cat)[q].tolist())
    print(f'seam points: {int(q.sum())} of {len(cat)} qualify: {dict(counts)}')
    assert q.sum() >= 40 and all(counts[c] > 0 for c in ('axis', 'r-edge', 'diagonal', 'nan', 'origin')), counts
    assert torch.isnan(out[[i for i, c in enumerate(cat) if c in ('nan', 'origin')]]).all()
    # a qualifying axis point at an exact frame time: the logarithm of its own node's data, without the interpolator
    checked = 0
    for i in np.nonzero(q)[0]:
        if cat[i] != 'axis' or float(w[i]) != 0.:
            continue
        r, th, phi, rho, temp = frames[int(f1[i])]
        node = tuple(int(np.searchsorted(a, v)) for a, v in zip((phi, th, r), intended[i][::-1]))
        if not all(k < a.size and a[k] == v for k, a, v in zip(node, (phi, th, r), intended[i][::-1])):
            assert not inside[i, 0]            # the narrow cube has no such node: filled
            continue
        want = torch.stack([torch.log(torch.tensor(rho[node], dtype=torch.float64).to(torch.float32)),
                            torch.log10(1e6 * torch.tensor(temp[node], dtype=torch.float64).to(torch.float32))])
        assert torch.equal(out[i], want), (i, out[i], want)
        checked += 1
    assert checked >= 100, checked


def test_general_position_nodes():
    gen = torch.Generator().manual_seed(4)
    d = torch.randn(60, 3, generator=gen)
    p = d / d.norm(dim=1, keepdim=True) * (1.05 + 0.85 * torch.rand(60, 1, generator=gen))
    frames = ref.general_position_frames(p)
    r, th, phi = ref.spherical(p.clone())
    for fr in frames:
        assert np.isin(th.numpy().astype(np.float64), fr[1][1:-1]).all() and np.isin(phi.numpy().astype(np.float64), fr[2][1:-1]).all()
        assert fr[1].size == 62 and fr[2].size == 62
