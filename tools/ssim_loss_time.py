"""Cost of the structural loss (csrc/ssim_loss.hip, sunerf_hip.ssim_loss.ssim_loss) at two shapes: the default
patch batch of the emission module, 4 patches of 16 x 16 detector pixels and one channel, where the call is latency-bound, and
512 patches of 16 x 16 with 7 channels.  Beside it, in the same process, the same loss as a composition of torch operations on
the device: fp64 ``avg_pool2d`` SSIM with autograd, on permuted copies of the same rows.

Per shape and implementation: microseconds of the forward alone and of forward + ``backward()``, CUDA-event median over
``--repeats`` windows of ``--calls`` back-to-back calls after a warm-up, Python call and allocations included.  Both are run with
the asinh stretch of the emission module and a window of 7.  One JSON line.  Not gated.

    python tools/ssim_loss_time.py [--repeats 7] [--calls 20]
"""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, '2024-hl-spi3s-sunerf_amd')]

ASINH = (1.0, 0.005)
WINDOW = 7


def timed(fn, repeats, calls):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(calls):
            fn()
        stop.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(stop) / calls)
    return sorted(times)[len(times) // 2], [min(times), max(times)]


def torch_loss(coarse, fine, target, n, P):
    """``dssim(coarse) + dssim(fine)`` by torch operations in fp64."""
    w, norm = WINDOW, WINDOW * WINDOW / (WINDOW * WINDOW - 1.0)

    def planes(v):
        v = torch.asinh(v.double() / ASINH[0] / ASINH[1]) / math.asinh(1.0 / ASINH[1])
        return v.reshape(n, P, P, -1).permute(0, 3, 1, 2)

    def pool(v):
        return torch.nn.functional.avg_pool2d(v, w, stride=1)
    y = planes(target)
    mu_y = pool(y)
    var_y = norm * (pool(y * y) - mu_y * mu_y)
    total = 0.0
    for image in (coarse, fine):
        x = planes(image)
        mu_x = pool(x)
        var_x, cov = norm * (pool(x * x) - mu_x * mu_x), norm * (pool(x * y) - mu_x * mu_y)
        s = (2 * mu_x * mu_y + 1e-4) * (2 * cov + 9e-4) / ((mu_x * mu_x + mu_y * mu_y + 1e-4) * (var_x + var_y + 9e-4))
        total = total + (1.0 - s.mean(dim=(2, 3)).mean())
    return total


def measure(n, P, C, repeats, calls):
    from sunerf_hip.ssim_loss import ssim_loss
    g = torch.Generator(device='cuda').manual_seed(n + C)
    target = torch.rand(n * P * P, C, device='cuda', generator=g) + 0.05
    coarse = (target * (0.8 + 0.4 * torch.rand(n * P * P, C, device='cuda', generator=g))).requires_grad_(True)
    fine = (target * (0.9 + 0.2 * torch.rand(n * P * P, C, device='cuda', generator=g))).requires_grad_(True)
    losses = {'ssim_loss (one kernel)': lambda: ssim_loss(coarse, fine, target, n, P, 1.0, window=WINDOW, asinh_scaling=ASINH)[0],
              'torch fp64 avg_pool2d': lambda: torch_loss(coarse, fine, target, n, P)}
    values = {name: float(forward()) for name, forward in losses.items()}
    rows = []
    for name, forward in losses.items():
        def step():
            coarse.grad = fine.grad = None
            forward().backward()
        with torch.no_grad():
            fwd, fwd_range = timed(forward, repeats, calls)
        both, both_range = timed(step, repeats, calls)
        rows.append({'loss': name, 'value': values[name], 'forward_us': 1e3 * fwd, 'forward_range_us': [1e3 * v for v in fwd_range],
                     'forward_backward_us': 1e3 * both, 'forward_backward_range_us': [1e3 * v for v in both_range]})
    return {'patches': n, 'P': P, 'channels': C, 'window': WINDOW, 'rows': rows,
            'value_difference': abs(values['ssim_loss (one kernel)'] - values['torch fp64 avg_pool2d'])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--calls', type=int, default=20)
    args = ap.parse_args()
    shapes = [(4, 16, 1), (512, 16, 7)]
    print(json.dumps({'ssim_loss_time': [measure(n, P, C, args.repeats, args.calls) for n, P, C in shapes],
                      'device': torch.cuda.get_device_name(0), 'repeats': args.repeats, 'calls': args.calls}))


if __name__ == '__main__':
    main()
