"""Cost of the shift sums of the co-alignment step (csrc/coalign.hip, sunerf_hip.coalign.shift_sums) at 7 x 1024^2 with
``max_shift`` 8 (289 shifts) and at 4096^2 with ``max_shift`` 32 (4225 shifts), with and without masks, next to

* one ``sunerf_psf_grad_taps`` call of the same geometry (``bin = 1``, BOUNDARY_ZERO, one kernel per plane): the plain cross term
  Sab alone, ONE of the six sums, from the same staged data -- a ratio above 6 would mean that fusing the six bought nothing;
* unless ``--no-host``: a masked normalised cross-correlation on the host, the six correlations through
  ``scipy.signal.fftconvolve`` in fp64 (Padfield's masked NCC), cropped to the window.

Per row: the CUDA-event time per call over ``--repeats`` windows of ``--calls`` back-to-back calls after a warm-up -- median,
fastest and slowest window -- the pair updates per second, and the fp64 floor: a pair update is 7 multiplies, 6 adds and 2
converts in fp64 (15 full-rate VALU operations per lane) against one 8-byte LDS read, so the adds and multiplies bound the kernel,
not the LDS (four SIMDs of 16 lanes share 128 bytes per clock of LDS: 16 clocks of LDS per 60 clocks of VALU).  One JSON line.

    python tools/coalign_time.py [--repeats 7] [--calls 3] [--no-host] [--clock-mhz 2400]
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

VALU_OPS_PER_PAIR = 15


def timed(fn, repeats, calls):
    """ms per call: (median, fastest, slowest) of ``repeats`` windows of ``calls`` calls, after two warm-up calls."""
    fn()
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
    times.sort()
    return times[len(times) // 2], times[0], times[-1]


def host_masked_ncc(image, templ, my, mx):
    """Seconds of the six masked correlations of ONE plane through fftconvolve (fp64), cropped to the window."""
    from scipy.signal import fftconvolve
    h, w = image.shape
    va, vb = np.isfinite(image), np.isfinite(templ)
    a, b = np.where(va, image, 0.0).astype(np.float64), np.where(vb, templ, 0.0).astype(np.float64)
    va, vb = va.astype(np.float64), vb.astype(np.float64)
    flip = lambda x: x[::-1, ::-1]          # noqa: E731
    start = time.perf_counter()
    out = []
    for x, y in ((va, vb), (a, vb), (va, b), (a * a, vb), (va, b * b), (a, b)):
        full = fftconvolve(x, flip(y), mode='full')
        out.append(full[h - 1 - my:h + my, w - 1 - mx:w + mx])
    return time.perf_counter() - start, np.stack(out, -1)


def measure(c, n, m, repeats, calls, with_host, clock_mhz):
    from sunerf_hip.coalign import shift_sums
    from sunerf_hip.psf_fit import tap_gradient
    g = torch.Generator(device='cuda').manual_seed(n + m)
    image = torch.rand(c, n, n, device='cuda', generator=g)
    templ = torch.rand(c, n, n, device='cuda', generator=g)
    holes = templ.clone()
    holes[torch.rand(c, n, n, device='cuda', generator=g) < 0.3] = float('nan')
    bad = (torch.rand(c, n, n, device='cuda', generator=g) < 0.01).to(torch.uint8)
    shifts = (2 * m + 1) ** 2
    pairs = c * n * n * shifts
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    row = {'shape': [c, n, n], 'max_shift': m, 'shifts': shifts, 'pair_updates': pairs}
    for key, fn in (('shift_sums_ms', lambda: shift_sums(image, templ, m)),
                    ('shift_sums_masked_ms', lambda: shift_sums(image, holes, m, bad_image=bad)),
                    ('tap_gradient_ms', lambda: tap_gradient(image, templ, c, 2 * m + 1, 2 * m + 1, 1, m, m, 1.0, 0))):
        med, lo, hi = timed(fn, repeats, calls)
        row[key] = {'median': med, 'min': lo, 'max': hi}
    row['shift_sums_over_tap_gradient'] = row['shift_sums_ms']['median'] / row['tap_gradient_ms']['median']
    row['G_pair_updates_per_s'] = pairs / row['shift_sums_ms']['median'] / 1e6
    row['fp64_floor_ms'] = 1e3 * pairs * VALU_OPS_PER_PAIR / (cus * 64 * clock_mhz * 1e6)          # 64 fp64 lanes per compute unit and clock
    row['compute_units'], row['clock_MHz'] = cus, clock_mhz
    witness = tap_gradient(image, templ, c, 2 * m + 1, 2 * m + 1, 1, m, m, 1.0, 0)
    sums = shift_sums(image, templ, m)
    row['Sab_equals_tap_gradient'] = bool(torch.equal(sums[..., 5], witness))
    if with_host:
        seconds, host = host_masked_ncc(image[0].cpu().numpy(), holes[0].cpu().numpy(), m, m)
        dev = shift_sums(image[:1], holes[:1], m)[0].cpu().numpy()
        row['host_fftconvolve_s_per_plane'] = seconds
        row['host_fftconvolve_s'] = seconds * c
        row['host_max_abs_difference_of_n'] = float(np.abs(host[..., 0] - dev[..., 0]).max())
        row['host_max_relative_difference_of_Sab'] = float((np.abs(host[..., 5] - dev[..., 5]) / np.abs(dev[..., 5])).max())
        row['host_over_device'] = seconds * c * 1e3 / row['shift_sums_masked_ms']['median']
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--calls', type=int, default=3)
    ap.add_argument('--no-host', action='store_true', help='skip the masked NCC through scipy.signal.fftconvolve on the host')
    ap.add_argument('--clock-mhz', type=float, default=2400.0, help='engine clock the fp64 floor is computed for (MI355X: 2400)')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('coalign_time.py needs a ROCm device')
    rows = [measure(c, n, m, args.repeats, args.calls, not args.no_host, args.clock_mhz) for c, n, m in ((7, 1024, 8), (1, 4096, 32))]
    print(json.dumps({'coalign_time': rows}))


if __name__ == '__main__':
    main()
