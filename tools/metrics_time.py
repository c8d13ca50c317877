"""Cost of the image scores (csrc/metrics.hip, sunerf_hip.metrics.image_metrics) at 7 x 4096^2 and 64 x 1024^2.

Per shape: milliseconds per ``image_metrics`` call (CUDA-event median over ``--repeats`` windows of ``--calls`` back-to-back
calls, after a warm-up), the input bytes per second, the counted fp64 operations per second, and the two lower bounds: the
input bytes at 6.3 TB/s (measured HBM copy rate, MI355X_MICROARCH) and the counted fp64 operations at 78.6 TFLOP/s (the
MI355X's FP64 vector rate as AMD specifies it, not measured here).  The kernels' own time comes from a separate
``rocprofv3 --kernel-trace --stats -- python tools/metrics_time.py`` run, which also shows two launches per call
(``image_metrics_tiles_kernel`` and ``image_metrics_finish_kernel``, ``calls`` of each per shape plus the warm-up).  One JSON
line.

    python tools/metrics_time.py [--repeats 5] [--calls 10]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, '2024-hl-spi3s-sunerf_amd')]

HBM_BYTES_PER_S = 6.3e12          # measured float4 copy rate
FP64_FLOP_PER_S = 78.6e12         # MI355X FP64 vector peak, vendor specification
TILE_W, TILE_H, WIN = 64, 16, 7
# fp64 operations the kernel performs per output pixel: 7-column sums of x, y, x^2, y^2, xy on (16 + 6) / 16 staged rows per
# output row (3 products + 5 adds per tap), 7-row sums of the five (5 x 7 adds) and their five divisions, the SSIM formula
# (21: 3 squares / products, 3 differences, 3 covariance scalings, a1, a2, b1, b2, the product and the division), and the
# pixel sums (d, d^2, |d|, four adds).  Conversions fp32 -> fp64 are not counted.
FLOP_PER_PIXEL = WIN * 8 * (TILE_H + WIN - 1) / TILE_H + 5 * WIN + 5 + 21 + 7


def measure(n, h, w, repeats, calls):
    from sunerf_hip.metrics import image_metrics
    g = torch.Generator(device='cuda').manual_seed(n * h)
    target = torch.rand(n, h, w, device='cuda', generator=g)
    pred = (target + 0.05 * torch.randn(n, h, w, device='cuda', generator=g)).clamp_(0, 1)
    image_metrics(pred, target, 1.0)
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(calls):
            image_metrics(pred, target, 1.0)
        stop.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(stop) / calls)
    ms = sorted(times)[len(times) // 2]
    pixels = n * h * w
    nbytes = 2 * 4 * pixels
    flop = FLOP_PER_PIXEL * pixels
    return {'shape': [n, h, w], 'ms_per_call': ms, 'input_bytes': nbytes, 'input_GB_per_s': nbytes / ms / 1e6,
            'counted_fp64_flop': flop, 'fp64_TFLOP_per_s': flop / ms / 1e9,
            'bound_ms_hbm': nbytes / HBM_BYTES_PER_S * 1e3, 'bound_ms_fp64_spec': flop / FP64_FLOP_PER_S * 1e3,
            'calls_timed': repeats * calls, 'spread_ms': [min(times), max(times)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--calls', type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('metrics_time.py needs a ROCm device')
    rows = [measure(n, h, w, args.repeats, args.calls) for n, h, w in ((7, 4096, 4096), (64, 1024, 1024))]
    print(json.dumps({'metrics_time': rows, 'flop_per_pixel': FLOP_PER_PIXEL, 'fp64_rate': 'spec 78.6 TFLOP/s',
                      'hbm_rate': 'measured 6.3 TB/s'}))


if __name__ == '__main__':
    main()
