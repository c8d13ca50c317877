"""Fit a NeRF to white-light (tB, pB) frames of a SimpleStar, both rendered by ThompsonScattering: the target frames through
the analytic field (ln rho), the NeRF (log10 rho) through the fused Thomson pass, its gradients through the Thomson
backward kernel and the MLP backward.  Prints the loss and the fine image's PSNR as it trains.

    python tools/mini_train_thomson.py [--steps 400] [--resolution 48] [--views 4] [--batch 4096]
"""
import argparse
import json
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, '2024-hl-spi3s-sunerf_amd')]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=400)
    ap.add_argument('--resolution', type=int, default=48)
    ap.add_argument('--views', type=int, default=4)
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--lr', type=float, default=5e-4)
    args = ap.parse_args()
    from sunerf.model.stellar_model import SimpleStar
    from sunerf.rendering.thompson import ThompsonScattering
    from sunerf_hip.rays import fov_axis, grid_rays, pose_spherical
    from sunerf_hip.train import ClipAdam
    torch.manual_seed(0)

    def config():
        return dict(Rs_per_ds=1.0, sampling_config={'type': 'stratified', 'n_samples': 32, 'perturb': False},
                    hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 32})
    star = ThompsonScattering(model=SimpleStar, model_config={}, **config()).cuda()
    nerf = ThompsonScattering(model_config={'d_filter': 128, 'n_layers': 4}, **config()).cuda()

    # target frames: several observers at 1 AU, a field of view out to 1.3 solar radii
    axis = fov_axis(args.resolution, 1.3 / 215.032, 'cuda')
    rays_o, rays_d, target = [], [], []
    with torch.no_grad():
        for v in range(args.views):
            o, d, _ = grid_rays(axis, axis, pose_spherical(2 * math.pi * v / args.views, 0.2 * (v % 3 - 1), 215.032), time=0.)
            rays_o.append(o)
            rays_d.append(d)
            target.append(star(o, d, torch.zeros(o.shape[0], 1, device='cuda'))['image'])
    rays_o, rays_d, target = torch.cat(rays_o), torch.cat(rays_d), torch.cat(target)
    scale = target.max(0).values                        # tB and pB to O(1): the NeRF's log10 rho starts near 0
    target = target / scale
    times = torch.zeros(rays_o.shape[0], 1, device='cuda')
    opt = ClipAdam(list(nerf.parameters()), lr=args.lr, max_norm=0.5)
    n = rays_o.shape[0]

    def evaluate():
        with torch.no_grad():
            out = nerf(rays_o, rays_d, times)
            mse = ((out['fine_image'] - target) ** 2).mean().item()
        return mse, 10 * math.log10(1.0 / max(mse, 1e-30))

    first, _ = evaluate()
    t0 = time.perf_counter()
    log = []
    for step in range(args.steps + 1):
        idx = torch.randint(0, n, (min(args.batch, n),), device='cuda')
        opt.zero_grad()
        out = nerf(rays_o[idx], rays_d[idx], times[idx])
        loss = ((out['coarse_image'] - target[idx]) ** 2).mean() + ((out['fine_image'] - target[idx]) ** 2).mean()
        loss.backward()
        opt.step()
        if step % 50 == 0:
            mse, psnr = evaluate()
            log.append({'step': step, 'loss': round(loss.item(), 6), 'frame_mse': mse, 'psnr_db': round(psnr, 2)})
            print(json.dumps(log[-1]), flush=True)
    last, psnr = evaluate()
    print(json.dumps({'frames': args.views, 'rays': n, 'steps': args.steps, 'initial_mse': first, 'final_mse': last,
                      'reduction': first / last, 'final_psnr_db': round(psnr, 2),
                      'seconds': round(time.perf_counter() - t0, 1)}))


if __name__ == '__main__':
    main()
