"""The comparison the per-pixel DEM inversion exists for: a density-temperature model renders a 7-channel frame,
``ModelLoader.invert_dem_image`` inverts it (default errors, discrepancy mode), and the result is scored against the model's own
line-of-sight DEM of the same frame (``render_dem_image``, optically thin): Pearson of log10 em, MAE of logt_mean, the PSNR of
the folded-back channels against the frame, and the share of pixels per status bit.

    python tools/dem_inversion_loop.py [--model star|nerf] [--resolution 256] [--samples 64] [--steps 300] [--lam LAM] [--lam-range MIN MAX] [--tol TOL]

``--model star``: the analytic ``SimpleStar``.  ``--model nerf``: a ``NeRF_DT`` (8 x 256) trained for ``--steps`` steps on eight
64 x 64 views of that star, as tools/mini_train_dt.py does.  The AIA response table comes from tests/golden/g9_simple_star.npz."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, '2024-hl-spi3s-sunerf_amd'))

AIA = (94, 131, 171, 193, 211, 304, 335)


def thin(rendering):
    with torch.no_grad():
        for m in (rendering.coarse_model, rendering.fine_model):
            for w in AIA:
                m.log_absortpion[str(w)].fill_(0.0)
    return rendering


def star(table, cfg):
    from sunerf.model.stellar_model import SimpleStar
    from sunerf.rendering.density_temperature import DensityTemperatureRadiativeTransfer
    return thin(DensityTemperatureRadiativeTransfer(Rs_per_ds=1, model=SimpleStar, model_config={}, response_table=table,
                                                    **{k: dict(v) for k, v in cfg.items()}).cuda())


def brief_nerf(table, cfg, steps):
    """A NeRF_DT fitted for ``steps`` steps to eight views of the (optically thin) star; returns its rendering module."""
    from sunerf.model.model import NeRF_DT
    from sunerf.model.sunerf import DensityTemperatureSuNeRFModule, fit_steps
    from sunerf_hip.rays import observer_rays
    target_of = star(table, cfg)
    views = [observer_rays(64, theta=-0.3 + 0.785 * k, phi=0.1 * (k % 3 - 1)) for k in range(8)]
    rays_o, rays_d = torch.cat([v[0] for v in views]), torch.cat([v[1] for v in views])
    n = rays_o.shape[0]
    times = torch.zeros(n, 1, device='cuda')
    wl = torch.tensor(AIA, dtype=torch.float32, device='cuda').repeat(n, 1)
    with torch.no_grad():
        target = target_of(rays_o, rays_d, times, wl)['image']
    target = target / target.abs().max()
    mod = DensityTemperatureSuNeRFModule(Rs_per_ds=1.0, seconds_per_dt=1.0, image_scaling_config={}, model=NeRF_DT,
                                         pixel_intensity_factor=1e10, response_table=table, model_config={'d_filter': 256},
                                         lr_config={'start': 5e-4, 'end': 5e-5, 'iterations': steps},
                                         **{k: dict(v) for k, v in cfg.items()}).cuda()
    mod.strict_finite_check = False

    def batches():
        for _ in range(steps):
            idx = torch.randint(0, n, (2048,), device='cuda')
            yield {'tracing': {'rays': torch.stack([rays_o[idx], rays_d[idx]], 1), 'time': times[idx], 'target_image': target[idx],
                               'wavelength': wl[idx]}}
    losses = torch.stack(fit_steps(mod, batches()))
    print(f'NeRF_DT: {steps} steps, loss {losses[:10].mean().item():.3e} -> {losses[-10:].mean().item():.3e}')
    return thin(mod.rendering)


def pearson(a, b):
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / torch.sqrt((a * a).sum() * (b * b).sum()))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--model', choices=('star', 'nerf'), default='star')
    ap.add_argument('--resolution', type=int, default=256)
    ap.add_argument('--samples', type=int, default=64, help='coarse and fine samples per ray, each')
    ap.add_argument('--steps', type=int, default=300)
    ap.add_argument('--lam', type=float, default=None, help='a fixed lam instead of discrepancy mode')
    ap.add_argument('--tol', type=float, default=1e-10, help='the Newton iteration stops at max |F| <= tol max |y / sigma|')
    ap.add_argument('--lam-range', type=float, nargs=2, default=(1e-4, 1e4), help='the bracket of discrepancy mode')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('dem_inversion_loop.py runs on a ROCm device; none is visible')
    from sunerf.evaluation.loader import ModelLoader
    from sunerf_hip import dem, metrics
    torch.manual_seed(0)
    fx = np.load(os.path.join(ROOT, 'tests', 'golden', 'g9_simple_star.npz'))
    table = (fx['aia_logte'], fx['aia_tresp'])
    cfg = dict(sampling_config={'type': 'stratified', 'n_samples': args.samples, 'perturb': False},
               hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': args.samples, 'perturb': False})
    rendering = star(table, cfg) if args.model == 'star' else brief_nerf(table, cfg, args.steps)
    res = args.resolution
    grid = {'shape': (res, res), 'cdelt': (2400. / res, 2400. / res), 'meta': {'t_obs': '2022-01-01T00:00:00.000'}}
    loader = ModelLoader(rendering=rendering, model=rendering.fine_model, ref_map=grid)
    frame = loader.render_observer_image(0.1, 0.3, 0.0, wl=np.array(AIA), as_numpy=False)['image']
    model = loader.render_dem_image(0.1, 0.3, 0.0, as_numpy=False)
    solver = dict({'lam_range': tuple(args.lam_range)} if args.lam is None else {'lam': args.lam}, tol=args.tol)
    out = loader.invert_dem_image(frame, as_numpy=False, **solver)
    status = out['status']
    n = status.numel()
    print(f'{args.model}, {res}x{res}, {args.samples}+{args.samples} samples, {f"discrepancy mode on lam in [{args.lam_range[0]:g}, {args.lam_range[1]:g}]" if args.lam is None else f"lam = {args.lam:g}"}; '
          f'flat prior {float(out["prior"][0]):.4e}')
    for bit, name in ((1, 'not converged'), (2, 'no channel'), (4, 'at lam_min (positivity binds)'), (8, 'at lam_max')):
        print(f'  status bit {bit:2d} {name:30s} {float((status & bit != 0).sum()) / n:8.3%}')
    steps = (status >> 8).float()
    print(f'  Newton steps per pixel (all solves): mean {float(steps.mean()):.1f}, most {int(steps.max())}')
    ok = (status & 2 == 0) & (out['em'] > 0) & (model['em'] > 0)
    print(f'  scored pixels: {int(ok.sum())} of {n}')
    print(f'  Pearson of log10 em (inversion vs render_dem_image): {pearson(out["em"][ok].double().log10(), model["em"][ok].double().log10()):.4f}')
    print(f'  em ratio inversion / model: median {float((out["em"][ok] / model["em"][ok]).median()):.3f}')
    print(f'  MAE of logt_mean: {float((out["logt_mean"][ok] - model["logt_mean"][ok]).abs().mean()):.4f} dex')
    folded = dem.fold(out['dem'].double(), rendering.inversion_response()).float()
    for c, w in enumerate(AIA):
        top = float(frame[..., c].max())
        m = metrics.image_metrics(folded[..., c][None].contiguous(), frame[..., c][None].contiguous(), top)
        print(f'  folded back, {w:3d} A: PSNR {float(m["psnr"][0]):6.2f} dB, SSIM {float(m["ssim"][0]):.4f} (data range {top:.3e})')
    if args.lam is None and bool(((status & 0xff) == 0).any()):
        chi2 = out['chi2'][(status & 0xff) == 0]
        print(f'  interior pixels: chi2 / 7 in [{float(chi2.min()) / 7:.6f}, {float(chi2.max()) / 7:.6f}], lam median {float(out["lam"][(status & 0xff) == 0].median()):.3e}')


if __name__ == '__main__':
    main()
