"""Cost of registration (csrc/register.hip, sunerf_hip.register) at 16 x 1 x 2048^2 and 8 x 7 x 1024^2, orders 1
and 3: ``sunerf_register_frames`` on prefiltered frames (the prefilter is timed on its own), next to

* ``sunerf_prep_affine_resample`` on the same planes at the same order -- the same tap sum without the geometry: a rotation by
  the angle the Sun's centre turns in the sequence about the image centre, one launch for all ``T C`` planes;
* the kernel's own HBM byte model: every source coefficient read once (8 bytes per plane and source pixel), every value written
  once (4 bytes per plane and pixel) plus the status byte per pixel and frame, at ``--hbm-tbs`` (8 TB/s is the MI355X's peak).  It
  ignores the axes, the descriptors and every tap that is fetched more than once.

The frames are a disk of 0.8 of the grid's half width seen by observers 1 degree apart, one hour apart, under the Snodgrass law.
Per row: the CUDA-event time per call over ``--repeats`` windows of ``--calls`` back-to-back calls after a warm-up -- median,
fastest and slowest window.  A record, not a gate.  One JSON line.

    python tools/register_time.py [--repeats 5] [--calls 2] [--hbm-tbs 8.0] [--shapes 16x1x2048,8x7x1024]
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, '2024-hl-spi3s-sunerf_amd'), os.path.join(ROOT, 'tools'), os.path.join(ROOT, 'tests')]

from coalign_time import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--calls', type=int, default=2)
    ap.add_argument('--hbm-tbs', type=float, default=8.0)
    ap.add_argument('--shapes', default='16x1x2048,8x7x1024')
    args = ap.parse_args()
    import register_reference as rr
    from sunerf_hip.prep import affine_resample, spline_prefilter
    from sunerf_hip.register import FRAME_DESC, launch, rotation_rates
    dev = torch.device('cuda')
    A, B, C = rotation_rates('snodgrass')
    rows = []
    for spec in args.shapes.split(','):
        t, c, n = (int(v) for v in spec.split('x'))
        tx, ty = rr.axes_for((n, n), 1.25 * rr.DISK)
        tx_d, ty_d = torch.from_numpy(tx).to(dev), torch.from_numpy(ty).to(dev)
        g = torch.Generator(device=dev).manual_seed(1)
        frames = torch.rand((t * c, n, n), device=dev, generator=g)
        for order in (1, 3):
            prefilter_ms = timed(lambda: spline_prefilter(frames, order), args.repeats, args.calls)
            coef, _ = spline_prefilter(frames, order)
            table = np.zeros(t, dtype=FRAME_DESC)
            for k, row in enumerate(table):
                row['coefficients'], row['mask'] = coef[k * c:(k + 1) * c].data_ptr(), 0
                row['tx'], row['ty'], row['height'], row['width'] = tx_d.data_ptr(), ty_d.data_ptr(), n, n
                row['c2w'] = rr.look_at_pose(0.0, math.radians(1.0 * k), rr.AU).reshape(-1)
                row['dt'] = k / 24.0
            table_d = torch.from_numpy(table.view(np.uint8).reshape(-1).copy()).to(dev)
            c2w_ref = torch.from_numpy(rr.look_at_pose(0.0, 0.0, rr.AU).reshape(-1).copy()).to(dev)
            call = lambda coords: launch(table_d, t, c, order, c2w_ref, tx_d, ty_d, 1.0, A, B, C, 1, float('nan'), 0, want_coords=coords)  # noqa: E731
            ms = timed(lambda: call(False), args.repeats, args.calls)
            ms_coords = timed(lambda: call(True), args.repeats, args.calls)
            state = call(False)[3].sum(0).tolist()
            angle = math.radians(1.0) * (t - 1) / 2.0
            m = np.array([[math.cos(angle), -math.sin(angle)], [math.sin(angle), math.cos(angle)]])
            centre = np.array([(n - 1) / 2.0, (n - 1) / 2.0])
            affine_ms = timed(lambda: affine_resample(coef, m, centre - m @ centre, (n, n), order), args.repeats, args.calls)
            pixels = t * n * n
            model_bytes = pixels * c * 12 + pixels
            rows.append({'shape': [t, c, n, n], 'order': order, 'ms': [round(v, 3) for v in ms], 'with_coords_ms': [round(v, 3) for v in ms_coords],
                         'prefilter_ms': [round(v, 3) for v in prefilter_ms], 'affine_resample_ms': [round(v, 3) for v in affine_ms],
                         'ratio_to_affine': round(ms[0] / affine_ms[0], 2), 'model_bytes_per_pixel': 12 * c + 1,
                         'floor_ms': round(model_bytes / (args.hbm_tbs * 1e9), 3), 'achieved_model_tbs': round(model_bytes / (ms[0] * 1e9), 3),
                         'gpixels_per_s': round(pixels / (ms[0] * 1e6), 3), 'status_counts': state})
            del coef
    print(json.dumps({'hbm_tbs': args.hbm_tbs, 'rows': rows}))


if __name__ == '__main__':
    main()
