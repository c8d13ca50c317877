"""Classical rotational tomography next to the neural reconstruction and the reprojection baseline, every stage
on the device: an analytic disk + corona is rendered from ``--views`` viewpoints into an ``ObservationSet`` (one view held
out, as tools/closed_loop.py does), then

- a voxel grid of (ln emissivity, absorption) -- ``GridField`` on a ``--grid``^3 cube -- is fitted through the emission
  integral with ``fit_steps`` (clip + Adam) and the smoothness prior ``--lambda-smoothness``,
- an ``EmissionSuNeRFModule`` with the MLP is trained on the same pool for the same number of steps,
- the reprojection baseline is taken from the training views,

and all three are scored on the held-out view (SSIM / PSNR / MAE of the images ``validation_metrics`` scores); the two volumetric
reconstructions are also scored in 3-D against the truth sampled on the same grid (``volume_metrics`` of the emissivity in the
shell 1.02 <= r <= half width).  One line per method on stderr, one JSON line on stdout.

The truth is a field, not an image formula, so that it has a volume: an opaque sphere (emissivity 4, absorption 40 per solar
radius inside r < 1) under a corona 0.5 exp(-(r - 1) / 0.12), evaluated in plain torch (it is the problem, not the solver).

    python tools/tomography_loop.py [--views 8] [--size 64] [--steps 1500] [--batch 2048] [--grid 48] [--half-width 1.3]
                                    [--lambda-smoothness 1e-4] [--lr 5e-2] [--d-filter 256] [--skip-network]
"""
import argparse
import json
import os
import sys
import time

import torch
from torch import nn

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(R, '2024-hl-spi3s-sunerf_amd'))
sys.path.insert(0, os.path.join(R, 'tools'))
from closed_loop import baseline_scores, held_out_scores                          # noqa: E402
from sunerf.evaluation.loader import ModelLoader                                  # noqa: E402
from sunerf.model.grid_model import GridField                                     # noqa: E402
from sunerf.model.sunerf import EmissionSuNeRFModule, fit_steps                   # noqa: E402
from sunerf.rendering.emission import EmissionRadiativeTransfer                   # noqa: E402
from sunerf_hip.feed import training_batches                                      # noqa: E402
from sunerf_hip.metrics import image_metrics                                      # noqa: E402
from sunerf_hip.observations import ObservationSet                                # noqa: E402
from sunerf_hip.volume import CartesianGrid, sample_volume, volume_metrics       # noqa: E402


class DiskAndCorona(nn.Module):
    """The truth: ``(ln emissivity, absorption)`` of an opaque sphere under an exponential corona."""

    def __init__(self, d_input=4, d_output=2):
        super().__init__()
        self.register_buffer('dummy', torch.zeros(1))

    def _raw(self, points):
        r = points[..., :3].pow(2).sum(-1).sqrt()
        inside = r < 1
        raw0 = torch.where(inside, torch.full_like(r, 1.3862944), -0.6931472 - (r - 1) / 0.12)
        return torch.stack([raw0, torch.where(inside, torch.full_like(r, 40.), torch.zeros_like(r))], -1)

    def field_on_rays(self, rays_o, rays_d, z_vals):
        return self._raw(rays_o[:, None, :] + rays_d[:, None, :] * z_vals[..., None])

    def forward(self, query_points):
        return {'inferences': self._raw(query_points.reshape(-1, query_points.shape[-1]))}


def sampling(perturb):
    return dict(sampling_config={'type': 'stratified', 'n_samples': 64, 'perturb': perturb},
                hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 128, 'perturb': perturb})


def image_scores(module, obs):
    scores = held_out_scores(module, obs, 1 << 14)
    stored = module.validation_outputs['test_image']
    (val,) = obs.validation_batches(1 << 14)
    h, w = val['image_shape']
    fine, target = module._validation_images(stored['fine_image'].reshape(h, w, -1), stored['target_image'].reshape(h, w, -1))
    mae = image_metrics(fine.permute(2, 0, 1).float().contiguous(), target.permute(2, 0, 1).float().contiguous(), 1.0)['mae']
    return {'ssim': scores['validation.ssim'], 'psnr': scores['validation.psnr'], 'mae': mae.mean().item()}


def volume_scores(rendering, truth_volume, grid, half_width):
    vol = sample_volume(rendering, grid, 0.0, r_range=(1.02, half_width))
    m = volume_metrics(vol['emission'], truth_volume['emission'], grid)
    return {k: m[k] for k in ('mae', 'rmse', 'pearson', 'mean_a', 'mean_b', 'count')}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--views', type=int, default=8)
    ap.add_argument('--size', type=int, default=64)
    ap.add_argument('--steps', type=int, default=1500)
    ap.add_argument('--batch', type=int, default=2048)
    ap.add_argument('--grid', type=int, default=48)
    ap.add_argument('--half-width', type=float, default=1.3)
    ap.add_argument('--lambda-smoothness', type=float, default=1e-4)
    ap.add_argument('--lr', type=float, default=5e-2)
    ap.add_argument('--d-filter', type=int, default=256)
    ap.add_argument('--skip-network', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('tomography_loop.py runs on a ROCm device; none is visible')
    torch.manual_seed(0)
    frame = {'shape': (args.size, args.size), 'cdelt': (2.2 * 960. / args.size, 2.2 * 960. / args.size),
             'meta': {'t_obs': '2022-01-01T00:00:00.000'}}
    poses = [(0.1 * (k % 3 - 1), 0.3 - 6.2832 / args.views * k) for k in range(args.views)]
    truth = EmissionRadiativeTransfer(Rs_per_ds=1.0, model=DiskAndCorona, **sampling(False)).cuda()
    loader = ModelLoader(rendering=truth, model=truth.fine_model, ref_map=frame)
    obs = ObservationSet(Rs_per_ds=1.0, seconds_per_dt=1.0, device='cuda')
    for lat, lon in poses:
        obs.add_rendered_view(loader, lat, lon, 0.0)
    obs.hold_out('reference')
    pool = obs.pool(batch_size=args.batch, seed=0, reshuffle='rays')
    grid = CartesianGrid.cube(args.half_width, args.grid)
    truth_volume = sample_volume(truth, grid, 0.0, r_range=(1.02, args.half_width))

    common = dict(Rs_per_ds=1.0, seconds_per_dt=1.0, image_scaling_config={'vmax': 1, 'a': 0.005})
    methods = {'tomography': EmissionSuNeRFModule(
        model=GridField, model_config={'grid': grid, 'init': (-4.0, 0.0)}, lambda_smoothness=args.lambda_smoothness,
        lr_config={'start': args.lr, 'end': args.lr / 10, 'iterations': args.steps}, **common, **sampling(True)).cuda()}
    if not args.skip_network:
        methods['network'] = EmissionSuNeRFModule(model_config={'d_filter': args.d_filter},
                                                  lr_config={'start': 5e-4, 'end': 5e-5, 'iterations': args.steps},
                                                  **common, **sampling(True)).cuda()
    result = {'views': args.views, 'held_out': obs.held_out, 'size': args.size, 'steps': args.steps, 'batch': args.batch,
              'grid': args.grid, 'half_width': args.half_width, 'lambda_smoothness': args.lambda_smoothness}
    for name, module in methods.items():
        module.strict_finite_check = False
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        losses = torch.stack(fit_steps(module, training_batches(pool, args.steps)))
        torch.cuda.synchronize()
        seconds = time.perf_counter() - t0
        module.check_finite(module.optimizer)
        result[name] = {'train_seconds': seconds, 'loss_first_10': losses[:10].mean().item(),
                        'loss_last_10': losses[-10:].mean().item(), 'image': image_scores(module, obs),
                        'volume': volume_scores(module.rendering, truth_volume, grid, args.half_width)}
    base = baseline_scores(next(iter(methods.values())), obs)
    result['reprojection'] = {'image': {'ssim': base['baseline.ssim'], 'psnr': base['baseline.psnr']}}
    for name in ('reprojection', 'tomography', 'network'):
        if name in result:
            img, vol = result[name]['image'], result[name].get('volume')
            line = f"{name:12s} held-out view: PSNR {img['psnr']:6.2f} dB  SSIM {img['ssim']:.4f}"
            if 'mae' in img:
                line += f"  MAE {img['mae']:.4f}"
            if vol is not None:
                line += f"   volume: MAE {vol['mae']:.4g}  RMSE {vol['rmse']:.4g}  Pearson {vol['pearson']:.4f}"
                line += f"   ({result[name]['train_seconds']:.1f} s)"
            print(line, file=sys.stderr)
    print(json.dumps({'tomography_loop': result}))


if __name__ == '__main__':
    main()
