"""Cost of combining a stack (csrc/stack.hip, sunerf_hip.stack.combine) at 8 x 7 x 1024^2 and 64 x 1 x 2048^2 -- the
median and the clipped mean (noise model, 5 sigma, 2 passes at most), each with and without the mask -- next to

* the HBM floor: every sample read once and the image and count written, ``4 T + 5`` bytes per pixel, ``5 T + 5`` with the mask,
  at ``--hbm-tbs`` (8 TB/s is the MI355X's peak; about 6.3 are reachable);
* a stack of 33 frames at 2048^2: the same instantiation on half the HBM bytes.  It still issues 64 loads per lane (registers past
  the last frame load the last frame's line again) and does the same arithmetic, so where it costs what 64 frames cost the kernel
  is not bound by HBM bytes -- whether by its arithmetic or by the issue of its loads this run cannot tell -- and where it costs
  half it is;
* a torch composition on the same device: ``torch.sort`` over dim 0 of a copy with +inf for the invalid samples, the two middle
  order statistics gathered, and for the clipped mean ONE pass of the test as masked arithmetic;
* unless ``--no-host``: ``np.nanmedian`` over axis 0 on the host.

Every case is timed twice: ``launch`` on device tensors (the entry point and its output allocations) and ``combine``, the wrapper,
which also validates and copies the ``[C, 4]`` parameters from pageable host memory -- a copy torch synchronises the stream for, so
the wrapper's figure includes a host round trip per call (``wrapper_ms``).  The floor is compared with ``launch``.

Per row: the CUDA-event time per call over ``--repeats`` windows of ``--calls`` back-to-back calls after a warm-up -- median,
fastest and slowest window.  One JSON line.

    python tools/stack_time.py [--repeats 7] [--calls 3] [--no-host] [--hbm-tbs 8.0]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, '2024-hl-spi3s-sunerf_amd'), os.path.join(ROOT, 'tools')]

from coalign_time import timed  # noqa: E402

A, B, N_SIGMA = 9.0, 1.0, 5.0


def torch_median(frames):
    valid = torch.isfinite(frames)
    s, _ = torch.sort(torch.where(valid, frames, frames.new_tensor(float('inf'))), dim=0)
    n = valid.sum(0, keepdim=True)
    lo, hi = torch.gather(s, 0, ((n - 1) // 2).clamp_(min=0)), torch.gather(s, 0, n // 2)
    med = 0.5 * (lo.double() + hi.double())
    return s, n, med


def torch_clipped_mean(frames):
    """One pass of the model test on the sorted copy, then the mean of what is left (fp64, torch's own order of summation)."""
    s, n, med = torch_median(frames)
    d = s.double() - med
    keep = torch.isfinite(s) & ~((d > 0) & (d * d > (N_SIGMA * N_SIGMA) * (A + B * med.clamp(min=0))))
    return (torch.where(keep, s.double(), d.new_zeros(())).sum(0) / keep.sum(0)).float()


def measure(t, c, n, repeats, calls, with_torch, with_host, hbm_tbs):
    from sunerf_hip.stack import METHODS, combine, launch
    g = torch.Generator(device='cuda').manual_seed(t + n)
    frames = 100.0 + 10.0 * torch.randn(t, c, n, n, device='cuda', generator=g)
    frames[torch.rand(t, c, n, n, device='cuda', generator=g) < 0.01] += 300.0
    frames[torch.rand(t, c, n, n, device='cuda', generator=g) < 0.001] = float('nan')
    px = c * n * n
    row = {'shape': [t, c, n, n], 'pixels': px, 'hbm_TB_per_s': hbm_tbs}
    clip = dict(method='mean', a=A, b=B, n_sigma=N_SIGMA, iterations=2)
    params = torch.tensor([[A, B, 0.0, 0.0]] * c, dtype=torch.float64, device='cuda')
    for key, kw, nbytes in (('median', dict(method='median'), 4 * t + 5), ('median_mask', dict(method='median', return_mask=True), 5 * t + 5),
                            ('clipped_mean', clip, 4 * t + 5), ('clipped_mean_mask', dict(clip, return_mask=True), 5 * t + 5)):
        direct = lambda: launch(frames, None, params, METHODS[kw['method']], 0.0, 0, 0, 0, N_SIGMA, kw.get('iterations', 0), 3, 1,          # noqa: E731
                                with_mask=kw.get('return_mask', False))
        med, lo, hi = timed(direct, repeats, calls)
        wrapped = timed(lambda: combine(frames, **kw), repeats, calls)
        floor = 1e3 * px * nbytes / (hbm_tbs * 1e12)
        row[key] = {'ms': {'median': med, 'min': lo, 'max': hi}, 'wrapper_ms': {'median': wrapped[0], 'min': wrapped[1], 'max': wrapped[2]},
                    'hbm_floor_ms': floor, 'over_floor': med / floor, 'ns_per_pixel': 1e6 * med / px}
        image, out = direct()[0], combine(frames, **kw)
        assert torch.equal(image.view(torch.int32), out['image'].view(torch.int32)), f'{key}: launch and combine differ'
    if with_torch:
        for key, fn in (('torch_median_ms', lambda: torch_median(frames)[2]), ('torch_clipped_mean_ms', lambda: torch_clipped_mean(frames))):
            med, lo, hi = timed(fn, max(3, repeats // 2), 1)
            row[key] = {'median': med, 'min': lo, 'max': hi}
        row['torch_median_over_device'] = row['torch_median_ms']['median'] / row['median']['ms']['median']
        row['torch_clipped_mean_over_device'] = row['torch_clipped_mean_ms']['median'] / row['clipped_mean']['ms']['median']
        same = combine(frames, method='median')['image'] == torch_median(frames)[2][0].float()
        row['median_equals_torch'] = bool(same.all())
    if with_host:
        host = frames.cpu().numpy()
        start = time.perf_counter()
        want = np.nanmedian(host, axis=0)
        row['host_nanmedian_s'] = time.perf_counter() - start
        row['host_over_device'] = row['host_nanmedian_s'] * 1e3 / row['median']['ms']['median']
        row['median_equals_nanmedian'] = bool(np.array_equal(combine(frames, method='median')['image'].cpu().numpy(), want, equal_nan=True))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--calls', type=int, default=3)
    ap.add_argument('--no-host', action='store_true', help='skip np.nanmedian on the host')
    ap.add_argument('--hbm-tbs', type=float, default=8.0, help='HBM bandwidth the floor is computed for, TB/s (MI355X: 8 peak, about 6.3 reachable)')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('stack_time.py needs a ROCm device')
    rows = [measure(8, 7, 1024, args.repeats, args.calls, True, not args.no_host, args.hbm_tbs),
            measure(64, 1, 2048, args.repeats, args.calls, True, not args.no_host, args.hbm_tbs),
            measure(33, 1, 2048, args.repeats, args.calls, False, False, args.hbm_tbs)]
    big, half = rows[1], rows[2]
    for key in ('median', 'median_mask', 'clipped_mean', 'clipped_mean_mask'):
        ratio = half[key]['ms']['median'] / big[key]['ms']['median']
        big[key]['33_frames_over_64'] = ratio
        big[key]['hbm_bytes'] = 'do not bound it' if ratio > 0.85 else ('bound it' if ratio < 0.6 else 'bound it in part')
    print(json.dumps({'stack_time': rows}))


if __name__ == '__main__':
    main()
