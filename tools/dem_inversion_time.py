"""Times the per-pixel DEM inversion (sunerf_hip.dem_inversion.invert_dem) of a 7-channel frame of a SimpleStar
rendering on K = 101 (the response table's grid) and K = 21 nodes, with a fixed lam and in discrepancy mode, each with the errors
and the prior given and with the defaults (``default_errors`` and ``flat_prior`` computed inside the call): medians of ``--reps``
calls between device events after a warm-up.  Next to it: ``render_dem_frame`` of the same frame (the model's own
line-of-sight DEM), and ``scipy.optimize.nnls`` on 256 of the frame's pixels on the host, extrapolated to the frame.

    python tools/dem_inversion_time.py [--resolution 1024] [--samples 64] [--reps 7] [--lam 1e-2]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, '2024-hl-spi3s-sunerf_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

AIA = (94, 131, 171, 193, 211, 304, 335)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--resolution', type=int, default=1024)
    ap.add_argument('--samples', type=int, default=64)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--lam', type=float, default=1e-2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('dem_inversion_time.py measures on a ROCm device; none is visible')
    from scipy.optimize import nnls
    from dem_inversion_loop import star
    from sunerf.evaluation.loader import ModelLoader
    from sunerf_hip import dem_inversion as inv
    fx = np.load(os.path.join(ROOT, 'tests', 'golden', 'g9_simple_star.npz'))
    cfg = dict(sampling_config={'type': 'stratified', 'n_samples': args.samples, 'perturb': False},
               hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': args.samples, 'perturb': False})
    rendering = star((fx['aia_logte'], fx['aia_tresp']), cfg)
    res = args.resolution
    grid = {'shape': (res, res), 'cdelt': (2400. / res, 2400. / res), 'meta': {'t_obs': '2022-01-01T00:00:00.000'}}
    loader = ModelLoader(rendering=rendering, model=rendering.fine_model, ref_map=grid)
    frame = loader.render_observer_image(0.1, 0.3, 0.0, wl=np.array(AIA), as_numpy=False)['image'].contiguous()
    sigma = inv.default_errors(frame)
    n = res * res
    what = f'{res}x{res} x 7 channels'
    t = timed(lambda: loader.render_dem_image(0.1, 0.3, 0.0, as_numpy=False), args.reps)
    print(f'{what}: render_dem_frame (SimpleStar, {args.samples}+{args.samples} samples)   median {statistics.median(t):9.3f} ms  min {min(t):9.3f}  max {max(t):9.3f}')
    for k in (101, 21):
        nodes = None if k == 101 else torch.linspace(5.5, 7.5, k)
        G = rendering.inversion_response(None, nodes)
        nd = rendering.dem_nodes(nodes)
        prior = inv.flat_prior(frame, G)
        for name, kw in ((f'lam = {args.lam:g}', dict(lam=args.lam, errors=sigma, prior=prior)),
                         ('discrepancy, 20 halvings', dict(errors=sigma, prior=prior)),
                         (f'lam = {args.lam:g}, defaults', dict(lam=args.lam)), ('discrepancy, defaults', {})):
            last = {}

            def call():
                last['out'] = inv.invert_dem(frame, G, nd, **kw)
            t = timed(call, args.reps)
            status = last['out']['status']
            steps = (status >> 8).float()
            print(f'{what}: invert_dem K = {k:3d}, {name:28s} median {statistics.median(t):9.3f} ms  min {min(t):9.3f}  max {max(t):9.3f}'
                  f'  ({n / statistics.median(t) / 1e3:.2f} Mpixel/s; Newton steps mean {float(steps.mean()):.1f}, most {int(steps.max())}; '
                  f'not converged {int((status & 1 != 0).sum())})')
        # the host: nnls on the stacked system, 256 pixels spread over the frame
        pick = torch.linspace(0, n - 1, 256).long().cuda()
        y = frame.reshape(n, 7)[pick].double().cpu().numpy()
        s = sigma.reshape(n, 7)[pick].double().cpu().numpy()
        g, p = G.cpu().numpy(), prior.cpu().numpy()
        reg = np.sqrt(args.lam) * np.diag(1.0 / p)
        t0 = time.perf_counter()
        for i in range(256):
            a = np.concatenate([g / s[i][:, None], reg])
            b = np.concatenate([y[i] / s[i], np.zeros(k)])
            scale = np.linalg.norm(b)
            nnls(a, b / max(scale, 1e-300), maxiter=100 * (k + a.shape[0]))
        dt = time.perf_counter() - t0
        print(f'{what}: scipy nnls K = {k:3d}, lam = {args.lam:g}: {dt / 256 * 1e3:.3f} ms per pixel on one host core = {dt / 256 * n:.1f} s per frame (extrapolated from 256 pixels)')


if __name__ == '__main__':
    main()
