"""Cost of one Richardson-Lucy iteration (csrc/deconvolve.hip, sunerf_hip.deconvolve) at two shapes: seven channels
of 1024 x 1024 under a 9 x 9 PSF, and one plane of 4096 x 4096 under a 33 x 33 PSF, both at bin 1.  Three implementations of the same
iteration, in the same process:

* the fused loop: ``sunerf_deconvolve_richardson_lucy``, all iterations enqueued by one call;
* the composition: ``Instrument.expected``, torch elementwise operations (fp32) and ``correlate_bin_adjoint`` per iteration;
* the host: ``scipy.signal.fftconvolve`` Richardson-Lucy in fp64 on the CPU (one iteration, wall clock).

Device times are CUDA-event medians over ``--repeats`` calls after a warm-up.  A call of n updates runs n + 1 ratio passes, so the
fused loop's time per iteration is (time of ``--iterations`` updates - time of none) / ``--iterations``; the time of the call without
an update (one ratio pass, one reduction) is reported beside it.  One JSON line.  Not gated.

    python tools/deconvolve_time.py [--repeats 5] [--iterations 10] [--skip-host]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, '2024-hl-spi3s-sunerf_amd')]

DETECTOR = dict(unit=1000.0, exposure=2.9, dn_per_photon=1.2, read_noise=1.2)


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(stop))
    return sorted(times)[len(times) // 2], [min(times), max(times)]


def host_iteration(u, d, psf, off, norm):
    """One iteration of the same rule on the host, fp64, zero boundary: two FFT convolutions (and one for the normalisation,
    which a loop would form once: taken outside the timed region by the caller)."""
    from scipy.signal import fftconvolve
    den = fftconvolve(u, psf, mode='same') + off
    ratio = np.where(den > 0, np.maximum(d + off, 0.0) / np.where(den > 0, den, 1.0), 0.0)
    return u * fftconvolve(ratio, psf[::-1, ::-1], mode='same') / norm


def measure(channels, size, radius, fwhm, repeats, iterations, skip_host):
    from sunerf_hip.deconvolve import initial_image, launch, photon_params
    from sunerf_hip.instrument import BOUNDARY, Instrument, correlate_bin_adjoint, gaussian_psf
    psf = gaussian_psf(fwhm, radius)
    inst = Instrument(psf=psf, boundary='zero', **DETECTOR)
    g = torch.Generator(device='cuda').manual_seed(size + channels)
    truth = torch.rand(channels, size, size, device='cuda', generator=g) + 0.05
    d = inst.observe(truth, seed=1)['image']
    K, (ay, ax) = inst.effective_kernel()
    call = (inst._taps(K, d.device), K.shape[0], K.shape[1], K.shape[2], 1, ay, ax, inst.scale, BOUNDARY['zero'])
    valid = torch.isfinite(d)
    norm = correlate_bin_adjoint(valid.to(torch.float32), size, size, *call)
    params = torch.from_numpy(photon_params(inst, channels)).to(d.device)
    start = initial_image(d, valid, inst, 'image')
    off = float(params[0, 1] / params[0, 0])
    u = start.clone()

    def fused(n):
        def run():
            u.copy_(start)
            launch(u, d, None, norm, params, *call, n, 0.0)
        return run

    def composed():
        v = start.clone()
        for _ in range(iterations):
            den = inst.expected(v) + off
            ratio = torch.where(valid & (den > 0), (d + off).clamp_min(0.0) / den, torch.zeros_like(den))
            t = correlate_bin_adjoint(ratio, size, size, *call)
            v = torch.where(norm > 0, v * t / norm, v)
        return v
    none_ms, none_range = timed(fused(0), repeats)
    full_ms, full_range = timed(fused(iterations), repeats)
    comp_ms, comp_range = timed(composed, repeats)
    fused(iterations)()
    difference = ((u - composed()).abs().max() / u.abs().max()).item()          # fp32 elementwise stages against fp64 ones
    row = {'channels': channels, 'size': size, 'psf': 2 * radius + 1, 'iterations': iterations,
           'fused_ms_per_iteration': (full_ms - none_ms) / iterations, 'fused_call_ms': full_ms, 'fused_call_range_ms': full_range,
           'fused_no_update_ms': none_ms, 'fused_no_update_range_ms': none_range,
           'composed_ms_per_iteration': comp_ms / iterations, 'composed_call_range_ms': comp_range,
           'largest_relative_difference': difference}
    if not skip_host:
        from scipy.signal import fftconvolve
        plane, u_host = d[0].double().cpu().numpy(), start[0].double().cpu().numpy()
        host_norm = fftconvolve(np.ones_like(plane), psf[::-1, ::-1], mode='same')
        u_host = host_iteration(u_host, plane, psf, off, host_norm)          # warm-up: the FFT plans and the pages
        t0 = time.perf_counter()
        host_iteration(u_host, plane, psf, off, host_norm)
        row['host_fftconvolve_ms_per_iteration'] = 1e3 * (time.perf_counter() - t0) * channels          # one plane timed, times the planes
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--iterations', type=int, default=10)
    ap.add_argument('--skip-host', action='store_true')
    args = ap.parse_args()
    shapes = [(7, 1024, 4, 2.5), (1, 4096, 16, 8.0)]
    print(json.dumps({'deconvolve_time': [measure(*s, args.repeats, args.iterations, args.skip_host) for s in shapes],
                      'device': torch.cuda.get_device_name(0), 'repeats': args.repeats}))


if __name__ == '__main__':
    main()
