"""Time-dependent rotational tomography next to static tomography, the neural reconstruction and the reprojection baseline
(DESIGN.md 8l), every stage on the device.  tools/tomography_loop.py compares them on a corona that stands still; real
rotational tomography collects its views while the Sun rotates and the corona changes between them.  Here the truth changes:
the disk and corona of tools/tomography_loop.py plus a Gaussian blob of emissivity that rises radially with time.  It is
rendered from ``--views`` viewpoints stepping round the Sun, view ``k`` at the normalised time ``k / (views - 1)``, into an
``ObservationSet`` (one view held out), then, for the same number of steps each,

- a static voxel grid -- ``GridField`` on a ``--grid``^3 cube -- is fitted with the smoothness prior (it can only smear the change),
- a grid with a time axis -- ``DynamicGridField``, the same cube x ``--frames`` frames over [0, 1] -- is fitted with the smoothness
  prior and the temporal prior ``--lambda-temporal``: classical time-dependent tomography,
- an ``EmissionSuNeRFModule`` with the 8 x ``--d-filter`` MLP is trained on the same pool,
- the reprojection baseline is taken from the training views,

and all are scored on the held-out view (PSNR / SSIM / MAE of the images ``validation_metrics`` scores); the volumetric
reconstructions are also scored in 3-D against the truth sampled on the same grid at t = 0.25 and t = 0.75 (``volume_metrics`` of
the emissivity in the shell 1.02 <= r <= half width).  One line per method on stderr, one JSON line on stdout.  Results to
report, not gates.

The truth is a ``time_dependent`` field in plain torch (it is the problem, not the solver).

    python tools/dynamic_tomography_loop.py [--views 12] [--size 64] [--steps 1500] [--batch 2048] [--grid 48] [--frames 5]
                                            [--half-width 1.3] [--lambda-smoothness 1e-4] [--lambda-temporal 1e-3] [--lr 5e-2]
                                            [--d-filter 256] [--skip-network]
"""
import argparse
import json
import math
import os
import sys
import time

import torch

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(R, '2024-hl-spi3s-sunerf_amd'))
sys.path.insert(0, os.path.join(R, 'tools'))
from tomography_loop import DiskAndCorona, image_scores, sampling                 # noqa: E402
from sunerf.evaluation.loader import ModelLoader                                  # noqa: E402
from sunerf.model.grid_model import DynamicGridField, GridField                   # noqa: E402
from sunerf.model.sunerf import EmissionSuNeRFModule, fit_steps                   # noqa: E402
from sunerf.rendering.emission import EmissionRadiativeTransfer                   # noqa: E402
from sunerf_hip.feed import training_batches                                      # noqa: E402
from sunerf_hip.observations import ObservationSet                                # noqa: E402
from sunerf_hip.volume import CartesianGrid, sample_volume, volume_metrics       # noqa: E402

SCORE_TIMES = (0.25, 0.75)


class RisingBlob(DiskAndCorona):
    """The truth: the disk and corona plus ``amplitude exp(-|p - c(t)|^2 / (2 width^2))`` of emissivity above the surface, its
    centre ``c(t)`` rising along one radius from ``r_start`` at t = 0 to ``r_end`` at t = 1 (times are clamped to [0, 1])."""

    time_dependent = True
    direction = (0.25, 0.6)                    # latitude, longitude [rad] of the radius the blob rises along
    r_start, r_end, width, amplitude = 1.05, 1.25, 0.1, 1.5

    def _raw_at(self, points, times):
        raw = self._raw(points)
        lat, lon = self.direction
        e = torch.tensor([-math.cos(lat) * math.sin(lon), math.cos(lat) * math.cos(lon), -math.sin(lat)], dtype=points.dtype,
                         device=points.device)
        t = times.clamp(0.0, 1.0)
        centre = (self.r_start + (self.r_end - self.r_start) * t)[..., None] * e
        blob = self.amplitude * torch.exp(-(points[..., :3] - centre).pow(2).sum(-1) / (2 * self.width ** 2))
        outside = points[..., :3].pow(2).sum(-1).sqrt() >= 1
        raw0 = torch.where(outside, torch.log(torch.exp(raw[..., 0]) + blob), raw[..., 0])
        return torch.stack([raw0, raw[..., 1]], -1)

    def field_on_rays(self, rays_o, rays_d, z_vals, times):
        points = rays_o[:, None, :] + rays_d[:, None, :] * z_vals[..., None]
        return self._raw_at(points, times.reshape(-1, 1).expand(z_vals.shape))

    def forward(self, query_points):
        q = query_points.reshape(-1, query_points.shape[-1])
        return {'inferences': self._raw_at(q[:, :3], q[:, 3])}


def reprojection_scores(module, obs):
    """The reprojection baseline on the held-out view under the scoring of ``validation_metrics`` (closed_loop.baseline_scores),
    with the MAE the other methods report."""
    def as_scored(planes):                                                 # (C, H, W) -> the images the callback scores
        image = planes.permute(1, 2, 0)
        return module._validation_images(image, image)[0].permute(2, 0, 1).float()
    scores = obs.baseline_metrics(data_range=1.0, normalize=as_scored)
    loss = scores['mse'].mean()
    return {'ssim': scores['ssim'][0].item(), 'psnr': (-10. * torch.log10(loss)).item(), 'mae': scores['mae'].mean().item()}


def volume_scores(rendering, truth, grid, half_width):
    out = {}
    for t in SCORE_TIMES:
        want = sample_volume(truth, grid, t, r_range=(1.02, half_width))
        vol = sample_volume(rendering, grid, t, r_range=(1.02, half_width))
        m = volume_metrics(vol['emission'], want['emission'], grid)
        out[f't={t}'] = {k: m[k] for k in ('mae', 'rmse', 'pearson', 'mean_a', 'mean_b', 'count')}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--views', type=int, default=12)
    ap.add_argument('--size', type=int, default=64)
    ap.add_argument('--steps', type=int, default=1500)
    ap.add_argument('--batch', type=int, default=2048)
    ap.add_argument('--grid', type=int, default=48)
    ap.add_argument('--frames', type=int, default=5)
    ap.add_argument('--half-width', type=float, default=1.3)
    ap.add_argument('--lambda-smoothness', type=float, default=1e-4)
    ap.add_argument('--lambda-temporal', type=float, default=1e-3)
    ap.add_argument('--lr', type=float, default=5e-2)
    ap.add_argument('--d-filter', type=int, default=256)
    ap.add_argument('--skip-network', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('dynamic_tomography_loop.py runs on a ROCm device; none is visible')
    if args.views < 2 or args.frames < 2:
        sys.exit('--views and --frames must be at least 2')
    torch.manual_seed(0)
    frame = {'shape': (args.size, args.size), 'cdelt': (2.2 * 960. / args.size, 2.2 * 960. / args.size),
             'meta': {'t_obs': '2022-01-01T00:00:00.000'}}
    poses = [(0.1 * (k % 3 - 1), 0.3 - 6.2832 / args.views * k, k / (args.views - 1)) for k in range(args.views)]
    truth = EmissionRadiativeTransfer(Rs_per_ds=1.0, model=RisingBlob, **sampling(False)).cuda()
    loader = ModelLoader(rendering=truth, model=truth.fine_model, ref_map=frame)
    obs = ObservationSet(Rs_per_ds=1.0, seconds_per_dt=1.0, device='cuda')
    for lat, lon, t in poses:
        obs.add_rendered_view(loader, lat, lon, t)
    obs.hold_out('reference')
    pool = obs.pool(batch_size=args.batch, seed=0, reshuffle='rays')
    grid = CartesianGrid.cube(args.half_width, args.grid)
    frame_times = [k / (args.frames - 1) for k in range(args.frames)]

    common = dict(Rs_per_ds=1.0, seconds_per_dt=1.0, image_scaling_config={'vmax': 1, 'a': 0.005})
    lr = {'start': args.lr, 'end': args.lr / 10, 'iterations': args.steps}
    methods = {
        'static grid': EmissionSuNeRFModule(model=GridField, model_config={'grid': grid, 'init': (-4.0, 0.0)},
                                            lambda_smoothness=args.lambda_smoothness, lr_config=dict(lr), **common,
                                            **sampling(True)).cuda(),
        'dynamic grid': EmissionSuNeRFModule(model=DynamicGridField,
                                             model_config={'grid': grid, 'init': (-4.0, 0.0), 'frame_times': frame_times},
                                             lambda_smoothness=args.lambda_smoothness, lambda_temporal=args.lambda_temporal,
                                             lr_config=dict(lr), **common, **sampling(True)).cuda()}
    if not args.skip_network:
        methods['network'] = EmissionSuNeRFModule(model_config={'d_filter': args.d_filter},
                                                  lr_config={'start': 5e-4, 'end': 5e-5, 'iterations': args.steps},
                                                  **common, **sampling(True)).cuda()
    result = {'views': args.views, 'view_times': [p[2] for p in poses], 'held_out': obs.held_out, 'size': args.size,
              'steps': args.steps, 'batch': args.batch, 'grid': args.grid, 'frames': args.frames, 'half_width': args.half_width,
              'lambda_smoothness': args.lambda_smoothness, 'lambda_temporal': args.lambda_temporal}
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
                        'volume': volume_scores(module.rendering, truth, grid, args.half_width)}
    result['reprojection'] = {'image': reprojection_scores(next(iter(methods.values())), obs)}
    for name in ('reprojection', 'static grid', 'dynamic grid', 'network'):
        if name in result:
            img, vol = result[name]['image'], result[name].get('volume')
            line = f"{name:12s} held-out view: PSNR {img['psnr']:6.2f} dB  SSIM {img['ssim']:.4f}"
            if 'mae' in img:
                line += f"  MAE {img['mae']:.4f}"
            if vol is not None:
                for key, v in vol.items():
                    line += f"   volume {key}: MAE {v['mae']:.4g} RMSE {v['rmse']:.4g} Pearson {v['pearson']:.4f}"
                line += f"   ({result[name]['train_seconds']:.1f} s)"
            print(line, file=sys.stderr)
    print(json.dumps({'dynamic_tomography_loop': result}))


if __name__ == '__main__':
    main()
