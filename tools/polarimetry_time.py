"""Cost of white-light polarimetry (csrc/polarimetry.hip, sunerf_hip.polarimetry):

* ``stokes`` on 3 x 1 x 2048^2 and 4 x 7 x 1024^2 exposures with the noise model and every output, next to the HBM floor -- every
  sample read once and the ten output planes and the status written, ``4 N + 41`` bytes per pixel at ``--hbm-tbs`` (8 TB/s is the
  MI355X's peak; about 6.3 are reachable) -- and next to a batched ``torch.linalg.lstsq`` of the same weighted system in fp64 on
  the first ``--lstsq-pixels`` pixels (the design matrix expanded per pixel; a subsample, so that the comparison's own cost stays
  bounded), its time per pixel set against the kernel's;
* ``ratio_depth`` on 2048^2 rays (``20`` bytes in and ``21`` out per ray), next to the same 64-step bisection written as torch fp64
  elementwise passes.

Per row: the CUDA-event time per call over ``--repeats`` windows of ``--calls`` back-to-back calls after a warm-up -- median,
fastest and slowest window.  One JSON line.

    python tools/polarimetry_time.py [--repeats 7] [--calls 3] [--hbm-tbs 8.0] [--lstsq-pixels 65536] [--no-torch]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, '2024-hl-spi3s-sunerf_amd'), os.path.join(ROOT, 'tools')]

from coalign_time import timed  # noqa: E402

A, B = 0.01, 0.02


def torch_lstsq(frames, rows, pixels):
    """(I, Q, U) of the first ``pixels`` pixels by ``torch.linalg.lstsq`` on the weighted rows, fp64: ``[pixels, 3]``."""
    y = frames.reshape(frames.shape[0], -1)[:, :pixels].t().double()
    sw = torch.rsqrt(A + B * y.clamp(min=0))
    return torch.linalg.lstsq(sw[:, :, None] * rows[None], (sw * y)[:, :, None]).solution[:, :, 0]


def torch_ratio(x, b2, R, u):
    r2 = b2 + x * x
    r = torch.sqrt(r2)
    s = R / r
    s2 = s * s
    c2 = (r2 - R * R) / r2
    c = torch.sqrt(c2)
    k = c2 * r / R * (0.5 * torch.log1p(2.0 * s / (1.0 - s)))
    ip = b2 / r2 * ((1.0 - u) * (c * s2) + u * (-0.125 * ((1.0 - 3.0 * s2) - k * (1.0 + 3.0 * s2))))
    it = (1.0 - u) * (s2 / (1.0 + c) * (4.0 + c + c2) / 3.0) + u * (0.125 * ((5.0 + s2) - k * (5.0 - s2)))
    return ip / (2.0 * it - ip)


def torch_bisection(q, b2, R, u, x_max_factor=64.0):
    lo, hi = torch.zeros_like(b2), x_max_factor * torch.sqrt(b2)
    for _ in range(64):
        m = 0.5 * (lo + hi)
        up = torch_ratio(m, b2, R, u) > q
        lo, hi = torch.where(up, m, lo), torch.where(up, hi, m)
    return 0.5 * (lo + hi)


def measure_stokes(n, c, size, args):
    from sunerf_hip import polarimetry as pl
    g = torch.Generator(device='cuda').manual_seed(n + size)
    angles = np.pi * np.arange(n) / n
    cos2, sin2, thr, eff = pl.design(angles)
    centre = (0.5 * size - 0.5, 0.5 * size - 0.5)
    tb = 5.0 + torch.rand(c, size, size, device='cuda', generator=g)
    frames = pl.polarise(tb, 0.3 * tb, angles, center=centre)
    frames = (frames + 0.05 * torch.randn(frames.shape, device='cuda', generator=g)).contiguous()
    a = torch.full((c,), A, dtype=torch.float64, device='cuda')
    b = torch.full((c,), B, dtype=torch.float64, device='cuda')
    px = c * size * size
    med, lo, hi = timed(lambda: pl.stokes_launch(frames, None, cos2, sin2, thr, eff, a, b, *centre), args.repeats, args.calls)
    floor = 1e3 * px * (4 * n + 41) / (args.hbm_tbs * 1e12)
    row = {'shape': [n, c, size, size], 'pixels': px, 'ms': {'median': med, 'min': lo, 'max': hi}, 'hbm_floor_ms': floor,
           'over_floor': med / floor, 'ns_per_pixel': 1e6 * med / px, 'hbm_TB_per_s': args.hbm_tbs}
    if not args.no_torch:
        rows = torch.tensor(np.stack([0.5 * thr, 0.5 * thr * eff * cos2, 0.5 * thr * eff * sin2], axis=1), device='cuda')
        some = min(px, args.lstsq_pixels)
        t = timed(lambda: torch_lstsq(frames, rows, some), 3, 1)
        row['torch_lstsq'] = {'pixels': some, 'ms': {'median': t[0], 'min': t[1], 'max': t[2]}, 'ns_per_pixel': 1e6 * t[0] / some}
        row['torch_over_device_per_pixel'] = row['torch_lstsq']['ns_per_pixel'] / row['ns_per_pixel']
        got = pl.stokes_launch(frames, None, cos2, sin2, thr, eff, a, b, *centre, outputs=('stokes',))['stokes'].reshape(3, -1).t().double()
        row['largest_difference_from_lstsq'] = float((got[:some] - torch_lstsq(frames, rows, some)).abs().max())
    return row


def measure_depth(size, args):
    from sunerf_hip import polarimetry as pl
    from sunerf_hip.rays import observer_rays
    n = size * size
    rays_o, rays_d = observer_rays(size, fov_half_rad=10.0 / 215.032)
    R, u = 1.0, 0.63
    o, d = rays_o.double(), rays_d.double()
    b2 = torch.linalg.cross(o, d).pow(2).sum(-1) / d.pow(2).sum(-1)
    b2 = b2.clamp(min=1.3 ** 2)
    x = torch.sqrt(b2) * (0.1 + 2.9 * torch.rand(n, device='cuda', dtype=torch.float64))
    q = torch_ratio(x, b2, R, u)
    tb = torch.ones(n, device='cuda')
    pb = q.float()
    rs, ld = torch.tensor([R], device='cuda'), torch.tensor([u], device='cuda')
    med, lo, hi = timed(lambda: pl.ratio_depth_launch(tb, pb, rays_o, rays_d, rs, ld), args.repeats, args.calls)
    floor = 1e3 * n * 53 / (args.hbm_tbs * 1e12)
    status = pl.ratio_depth_launch(tb, pb, rays_o, rays_d, rs, ld)['status']
    row = {'rays': n, 'ms': {'median': med, 'min': lo, 'max': hi}, 'hbm_floor_ms': floor, 'over_floor': med / floor, 'ns_per_ray': 1e6 * med / n,
           'inverted_fraction': float((status == pl.OK).float().mean())}
    if not args.no_torch:
        t = timed(lambda: torch_bisection(q, b2, R, u), max(3, args.repeats // 2), 1)
        row['torch_bisection_ms'] = {'median': t[0], 'min': t[1], 'max': t[2]}
        row['torch_over_device'] = t[0] / med
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--calls', type=int, default=3)
    ap.add_argument('--hbm-tbs', type=float, default=8.0, help='HBM bandwidth the floor is computed for, TB/s (MI355X: 8 peak, about 6.3 reachable)')
    ap.add_argument('--lstsq-pixels', type=int, default=65536, help='pixels torch.linalg.lstsq solves (the first ones of the frame)')
    ap.add_argument('--no-torch', action='store_true', help='skip the torch compositions')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('polarimetry_time.py needs a ROCm device')
    print(json.dumps({'polarimetry_time': {'stokes': [measure_stokes(3, 1, 2048, args), measure_stokes(4, 7, 1024, args)],
                                           'ratio_depth': measure_depth(2048, args)}}))


if __name__ == '__main__':
    main()
