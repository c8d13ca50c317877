"""The polarisation-ratio method closed on a known scene (sunerf_hip.polarimetry): a compact Gaussian blob of
electrons in a ``GridField``, off the plane of the sky at a known position, is

    rendered by ThompsonScattering from 1 AU  ->  polarise (0 / 60 / 120 degrees)  ->  Instrument.observe (two photon levels)
    ->  Instrument.stokes  ->  view_ratio_depth

and the report sets the blob's true distance from the closest-approach point of its line of sight next to the brightness-weighted
mean ``depth`` over the blob's pixels and its scatter, without noise and at either photon level, and says which of ``points_front``
and ``points_back`` the truth falls on (the method cannot tell; the blob is placed in front).  One JSON line.

    python tools/polarimetry_loop.py [--impact 4.0] [--depth 2.0] [--sigma 0.35] [--resolution 64] [--photons 1e4 1e6]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, '2024-hl-spi3s-sunerf_amd')]

AU = 215.032
ANGLES = np.radians([0.0, 60.0, 120.0])


def scene(args):
    """(rendering module, observer, blob centre [3], true signed geometry) of a blob ``--depth`` in front of the plane of the sky at
    the impact parameter ``--impact``."""
    from sunerf.model.grid_model import GridField
    from sunerf.rendering.thompson import ThompsonScattering
    from sunerf_hip.reprojection import Observer
    from sunerf_hip.volume import CartesianGrid
    half = (args.impact + 4.0 * args.sigma + 1.0) / AU
    axis = torch.linspace(-half, half, args.resolution, dtype=torch.float64, device='cuda')
    observer = Observer(0.0, 0.0, AU, tx=axis, ty=axis)
    o = observer.c2w[:3, 3].double().numpy()
    n = -o / np.linalg.norm(o)                                   # towards the Sun's centre
    e = np.cross(n, [0.3, 0.5, 0.8])
    e /= np.linalg.norm(e)
    centre = args.impact * e - args.depth * n                    # in front of the plane of the sky through the Sun's centre
    d = (centre - o) / np.linalg.norm(centre - o)
    z0 = -float(o @ d)
    closest = o + z0 * d
    truth = {'impact': float(np.linalg.norm(closest)), 'depth': float(np.linalg.norm(centre - closest)),
             'side': 'front' if float((centre - o) @ d) < z0 else 'back'}
    ax = torch.linspace(-4.0 * args.sigma, 4.0 * args.sigma, args.nodes, dtype=torch.float64)
    grid = CartesianGrid(ax, ax, ax, origin=tuple(centre.tolist()))
    r2 = ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2
    ln_rho = (-0.5 * r2 / args.sigma ** 2)[..., None].float()
    span = args.impact + args.depth + 4.0 * args.sigma + 1.0          # the sampled slab: this far either side of the Sun's distance
    mod = ThompsonScattering(Rs_per_ds=1.0, model=GridField, model_config={'grid': grid, 'd_output': 1, 'init': ln_rho, 'trainable': False},
                             sampling_config={'type': 'stratified', 'distance': span, 'n_samples': args.samples, 'perturb': False},
                             hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': args.samples, 'perturb': False}).cuda()
    return mod, observer, axis, centre, truth


def report(depth, weight, blob, centre, truth):
    """Brightness-weighted mean and scatter of ``depth`` over the blob's pixels with an inversion, and the side the truth is on."""
    use = blob & torch.isfinite(depth['depth'])
    w = torch.where(use, weight, weight.new_zeros(())).double()
    mean = float((w * torch.nan_to_num(depth['depth']).double()).sum() / w.sum())
    var = float((w * (torch.nan_to_num(depth['depth']).double() - mean) ** 2).sum() / w.sum())
    c = torch.as_tensor(centre, dtype=torch.float32, device=weight.device)
    miss = {side: float((w * (torch.nan_to_num(depth[f'points_{side}']) - c).norm(dim=-1).double()).sum() / w.sum()) for side in ('front', 'back')}
    return {'pixels': int(use.sum()), 'of': int(blob.sum()), 'depth_mean': mean, 'depth_scatter': var ** 0.5, 'depth_true': truth['depth'],
            'mean_distance_of_points_to_truth': miss, 'truth_falls_on': min(miss, key=miss.get), 'truth_is': truth['side']}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--impact', type=float, default=4.0, help='impact parameter of the blob, solar radii')
    ap.add_argument('--depth', type=float, default=2.0, help='distance of the blob in front of the plane of the sky, solar radii')
    ap.add_argument('--sigma', type=float, default=0.35, help='width of the Gaussian blob, solar radii')
    ap.add_argument('--resolution', type=int, default=64)
    ap.add_argument('--nodes', type=int, default=48)
    ap.add_argument('--samples', type=int, default=128)
    ap.add_argument('--photons', type=float, nargs='*', default=[1e4, 1e6], help='photons at the brightest pixel of a polariser frame')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('polarimetry_loop.py needs a ROCm device')
    from sunerf_hip import polarimetry as pl
    from sunerf_hip.enhance import sun_geometry
    from sunerf_hip.instrument import Instrument
    from sunerf_hip.rays import render_frame
    mod, observer, axis, centre, truth = scene(args)
    frame = render_frame(mod, axis, axis, observer.c2w, 0.0, keys=('pixel_B',))['pixel_B']
    tb, pb = frame[..., 0].contiguous(), frame[..., 1].contiguous()
    sun, _ = sun_geometry(observer)
    blob = tb > 0.05 * tb.max()
    frames = pl.polarise(tb, pb, ANGLES, center=sun)
    clean = pl.view_ratio_depth(tb, pb, observer, mod)
    out = {'truth': truth, 'blob_centre': centre.tolist(), 'noise_free': report(clean, tb, blob, centre, truth)}
    for level in args.photons:
        inst = Instrument(unit=level / float(frames.max()), exposure=1.0, dn_per_photon=1.0, read_noise=1.0)
        seen = inst.observe(frames, seed=int(level) % 1000 + 1)['image']
        got = inst.stokes(seen[:, None].contiguous(), ANGLES, center=sun)
        ratio_sigma = (got['pb'][0] / got['tb'][0]).abs() * torch.sqrt((got['sigma_pb'][0] / got['pb'][0]) ** 2 + (got['sigma_tb'][0] / got['tb'][0]) ** 2)
        depth = pl.view_ratio_depth(got['tb'][0].contiguous(), got['pb'][0].contiguous(), observer, mod, ratio_sigma=ratio_sigma)
        row = report(depth, tb, blob, centre, truth)
        use = blob & torch.isfinite(depth['depth_sigma'])
        row['median_depth_sigma'] = float(depth['depth_sigma'][use].median()) if bool(use.any()) else None
        row['status_counts'] = torch.bincount(depth['status'][blob].reshape(-1).long(), minlength=6).tolist()
        out[f'photons_{level:g}'] = row
    print(json.dumps({'polarimetry_loop': out}))


if __name__ == '__main__':
    main()
