"""Cost of the enhancement filters (csrc/enhance.hip, sunerf_hip.enhance) at 1 x 4096^2 and 7 x 1024^2.

``sunerf_enhance_mgn`` under the default six scales, next to

* what a user would write in PyTorch on the same device: the same separable convolutions as ``torch.nn.functional.conv2d`` on a
  replicate-padded plane (no mask), the same r, s, atan and gamma term;
* the byte model of the passes: per pixel 8 bytes for the cleaning pass and 44 per scale (row pass: 4 in, 4 out; column pass with
  r: 8 in, 4 out; row pass of r^2: 4 in, 4 out; column pass with t_i: 12 in, 4 out; the first scale reads no accumulator, the last
  reads the image), at ``--hbm-tbs`` (8 TB/s is the MI355X's peak).  It ignores every halo.

The same with an invalid pixel in every plane (the mask sums run), and ``sunerf_enhance_nrgf`` at the same shapes with 512 rings, its
statistics computed in the call and given by the caller.

Per row: the CUDA-event time per call over ``--repeats`` windows of ``--calls`` back-to-back calls after a warm-up -- median,
fastest and slowest window.  A record, not a gate.  One JSON line.

    python tools/enhance_time.py [--repeats 5] [--calls 2] [--hbm-tbs 8.0] [--shapes 1x4096,7x1024]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, '2024-hl-spi3s-sunerf_amd'), os.path.join(ROOT, 'tools'), os.path.join(ROOT, 'tests')]

from coalign_time import timed  # noqa: E402


def torch_mgn(x, sigma, k=0.7, gamma=3.2, h=0.7, truncate=3.0):
    """MGN of ``x`` [C, H, W] as plain PyTorch: separable ``conv2d`` on replicate-padded planes."""
    import torch.nn.functional as F
    planes = x[:, None]
    lo, hi = planes.amin((2, 3), keepdim=True), planes.amax((2, 3), keepdim=True)
    floor2 = (torch.maximum(lo.abs(), hi.abs()) * 2.0 ** -16) ** 2
    acc = torch.zeros_like(planes)
    for s in sigma:
        r = int(truncate * s + 0.5)
        j = torch.arange(-r, r + 1, dtype=torch.float64, device=x.device)
        w = torch.exp(-(j * j) / (2.0 * s * s))
        w = (w / w.sum()).float()

        def blur(f):
            f = F.conv2d(F.pad(f, (r, r, 0, 0), mode='replicate'), w.view(1, 1, 1, -1))
            return F.conv2d(F.pad(f, (0, 0, r, r), mode='replicate'), w.view(1, 1, -1, 1))
        res = planes - blur(planes)
        acc += torch.atan(k * res / torch.sqrt(blur(res * res) + floor2))
    g = ((planes - lo) / (hi - lo)).clamp(0.0, 1.0) ** (1.0 / gamma)
    return (h * g + (1.0 - h) / len(sigma) * acc)[:, 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--calls', type=int, default=2)
    ap.add_argument('--hbm-tbs', type=float, default=8.0)
    ap.add_argument('--shapes', default='1x4096,7x1024')
    args = ap.parse_args()
    from sunerf_hip.enhance import DEFAULT_SIGMA, mgn, nrgf
    dev = torch.device('cuda')
    rows = []
    for spec in args.shapes.split(','):
        c, n = (int(v) for v in spec.split('x'))
        g = torch.Generator(device=dev).manual_seed(1)
        x = torch.exp(0.5 * torch.randn((c, n, n), device=dev, generator=g)) + torch.linspace(0.0, 4.0, n, device=dev)
        holed = x.clone()
        holed[:, n // 3, n // 2] = float('nan')
        ms = timed(lambda: mgn(x), args.repeats, args.calls)
        masked_ms = timed(lambda: mgn(holed), args.repeats, args.calls)
        torch_ms = timed(lambda: torch_mgn(x, DEFAULT_SIGMA), args.repeats, args.calls)
        got, want = mgn(x)['image'], torch_mgn(x, DEFAULT_SIGMA)
        pixels = c * n * n
        per_pixel = 8 + 44 * len(DEFAULT_SIGMA)
        flops = sum(2 * 4 * (2 * int(3.0 * s + 0.5) + 1) for s in DEFAULT_SIGMA)          # 4 passes per scale, a multiply-add per tap
        center, edges = ((n - 1) / 2.0 + 0.3, (n - 1) / 2.0 - 0.4), np.linspace(0.0, 0.6 * n, 513)
        nrgf_ms = timed(lambda: nrgf(x, center, edges), args.repeats, args.calls)
        table = nrgf(x, center, edges)['statistics']
        apply_ms = timed(lambda: nrgf(x, center, edges, statistics=table), args.repeats, args.calls)
        rows.append({'shape': [c, n, n], 'mgn_ms': [round(v, 3) for v in ms], 'mgn_with_an_invalid_pixel_ms': [round(v, 3) for v in masked_ms],
                     'torch_conv2d_ms': [round(v, 3) for v in torch_ms], 'ratio_to_torch': round(ms[0] / torch_ms[0], 3),
                     'max_abs_difference_to_torch': float((got - want).abs().max()), 'model_bytes_per_pixel': per_pixel,
                     'floor_ms': round(pixels * per_pixel / (args.hbm_tbs * 1e9), 3), 'achieved_model_tbs': round(pixels * per_pixel / (ms[0] * 1e9), 3),
                     'flops_per_pixel': flops, 'achieved_tflops': round(pixels * flops / (ms[0] * 1e9), 2), 'nrgf_512_rings_ms': [round(v, 3) for v in nrgf_ms],
                     'nrgf_given_statistics_ms': [round(v, 3) for v in apply_ms]})
    print(json.dumps({'hbm_tbs': args.hbm_tbs, 'rows': rows}))


if __name__ == '__main__':
    main()
