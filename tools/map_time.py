"""Times a heliographic map (sunerf_hip.maps.render_columns) next to the observer-frame driver of
tools/frame_time.py at the same width: device-synchronised wall time and MLP samples / s.

    python tools/map_time.py [n_lat n_lon n_samples]        (default 721 1441 512, d_filter 256 and 512)"""
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), '2024-hl-spi3s-sunerf_amd'))
from sunerf.rendering.emission import EmissionRadiativeTransfer  # noqa: E402
from sunerf_hip.maps import render_columns  # noqa: E402
from sunerf_hip.rays import fov_axis, pose_spherical, render_frame  # noqa: E402

n_lat, n_lon, S = (int(v) for v in sys.argv[1:4]) if len(sys.argv) > 3 else (721, 1441, 512)
REPS = 2


def timed(fn):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(REPS):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / REPS


lat = torch.linspace(-math.pi / 2, math.pi / 2, n_lat, dtype=torch.float64, device='cuda')
lon = torch.linspace(-math.pi, math.pi, n_lon, dtype=torch.float64, device='cuda')
for d_filter in (256, 512):
    torch.manual_seed(7)
    r = EmissionRadiativeTransfer(Rs_per_ds=1.0, sampling_config={'type': 'stratified', 'n_samples': 64, 'perturb': False},
                                  hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 64},
                                  model_config={'d_filter': d_filter}).cuda()
    dt = timed(lambda: render_columns(r, lat, lon, 0.2, (1.0, 1.3), S))
    samples = n_lat * n_lon * S
    print(f'd_filter {d_filter}: {n_lat}x{n_lon}x{S} map {dt * 1e3:.1f} ms = {samples / dt:.3e} samples/s')
    res = 1024
    ax = fov_axis(res, 1.1 * 960. / 206264.806, 'cuda')
    c2w = pose_spherical(-0.3, 0.1, 215.032)
    df = timed(lambda: render_frame(r, ax, ax, c2w, 0.2, keys=('image', 'height_map', 'absorption_map')))
    print(f'd_filter {d_filter}: {res}x{res} two-pass frame {df * 1e3:.1f} ms = {res * res * 192 / df:.3e} samples/s '
          f'(map / frame rate {samples / dt / (res * res * 192 / df):.3f})')
