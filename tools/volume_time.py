"""Time of 3-D volumes: python tools/volume_time.py [--cube 256] [--repeats 10] [--only cube|shell] [--tile-points N]

The reference's 256^3 emission cube and a 181 x 361 x 128 density-temperature shell with 7 channels through 8 x 256 networks
(sunerf_hip.volume.sample_volume), and volume_metrics on both.  The cube's points/s stands next to tools/points_rate.py at the
same count: that tool times the MLP alone on points that already lie on the device.  ``--only`` keeps a kernel trace to one
workload; ``--tile-points`` sets the voxels per tile (default: sample_volume's 2^22), to see where the per-tile host work shows."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, '2024-hl-spi3s-sunerf_amd'))

from sunerf.model.model import NeRF_DT  # noqa: E402
from sunerf.rendering.density_temperature import DensityTemperatureRadiativeTransfer  # noqa: E402
from sunerf.rendering.emission import EmissionRadiativeTransfer  # noqa: E402
from sunerf_hip.volume import CartesianGrid, SphericalGrid, sample_volume, volume_metrics  # noqa: E402


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(repeats):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / repeats, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cube', type=int, default=256)
    ap.add_argument('--shell', type=int, nargs=3, default=(181, 361, 128))
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--tile-points', type=int, default=None)
    ap.add_argument('--only', choices=('cube', 'shell'), default=None)
    args = ap.parse_args()
    cfg = dict(Rs_per_ds=1.0, sampling_config={'type': 'stratified', 'n_samples': 64, 'perturb': False},
               hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 64})
    if args.only != 'shell':
        torch.manual_seed(0)
        emission = EmissionRadiativeTransfer(model_config={'d_filter': 256, 'n_layers': 8}, **cfg).cuda()
        cube = CartesianGrid.cube(1.3, args.cube)
        dt, vol = timed(lambda: sample_volume(emission, cube, 0.5, tile_points=args.tile_points), args.repeats)
        n = cube.n_voxels
        print(f'emission cube {args.cube}^3 = {n} voxels, tiles of {args.tile_points or "2^22"}: {dt * 1e3:.1f} ms = {n / dt:.3e} points/s')
        shifted = vol['emission'] * 1.01
        mt, m = timed(lambda: volume_metrics(vol['emission'], shifted, cube), args.repeats)
        print(f'volume_metrics on the cube: {mt * 1e3:.2f} ms ({m["count"]} of {n} voxels counted, mae {m["mae"]:.3e})')
    if args.only == 'cube':
        return

    with np.load(os.path.join(ROOT, 'tests', 'golden', 'g6_dt_e2e.npz')) as g:
        table = (g['aia_logte'], g['aia_tresp'])
    cfg = dict(Rs_per_ds=1.0, sampling_config={'type': 'stratified', 'n_samples': 64, 'perturb': False},
               hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 64})
    density = DensityTemperatureRadiativeTransfer(model=NeRF_DT, model_config={'d_filter': 256, 'n_layers': 8},
                                                  response_table=table, **cfg).cuda()
    n_lat, n_lon, n_r = args.shell
    shell = SphericalGrid(np.linspace(-np.pi / 2, np.pi / 2, n_lat), np.linspace(-np.pi, np.pi, n_lon), np.linspace(1.0, 1.3, n_r))
    wl = np.array([94., 131., 171., 193., 211., 304., 335.])
    dt, vol = timed(lambda: sample_volume(density, shell, 0.5, wavelengths=wl, tile_points=args.tile_points), args.repeats)
    n = shell.n_voxels
    print(f'density-temperature shell {n_lat} x {n_lon} x {n_r} = {n} voxels, 7 channels: {dt * 1e3:.1f} ms = {n / dt:.3e} points/s')
    other = vol['density'] * 0.99
    mt, m = timed(lambda: volume_metrics(vol['density'], other, shell), args.repeats)
    print(f'volume_metrics on the shell: {mt * 1e3:.2f} ms ({m["count"]} of {n} voxels counted, me {m["me"]:.3e})')


if __name__ == '__main__':
    main()
