"""Cost of the white-light Thomson-scattering integral (csrc/thomson.hip) inside a frame and a training step.

  * a 1024^2 observer frame, 64 + 128 samples per ray, of a NeRF (d_filter 256) and of a PSI-sized synthetic MHD cube
    (tools/mhd_render_time.py's frames): the frame's time and the Thomson forward kernel's time on the frame's two passes;
  * a 32768-ray training step of the NeRF (coarse + fine pass, tB/pB MSE, backward): the step's time and the Thomson
    forward + backward kernels' time on its shapes.

Kernel times are CUDA-event medians of the kernel alone on the same shapes.  One JSON line.

    python tools/thomson_render_time.py [--resolution 1024] [--repeats 5] [--no-mhd]
"""
import argparse
import json
import os
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, '2024-hl-spi3s-sunerf_amd'), os.path.join(ROOT, 'tools')]


def median_ms(fn, repeats):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return sorted(times)[len(times) // 2]


def kernel_ms(ops, rendering, rays_o, rays_d, n_samples, repeats, kappa, backward):
    """Median time of the Thomson forward (and backward) kernel alone on (rays, n_samples) with the module's constants."""
    n = rays_o.shape[0]
    gen = torch.Generator(device='cuda').manual_seed(0)
    z = torch.sort(213.7 + 2.6 * torch.rand(n, n_samples, device='cuda', generator=gen), -1).values
    raw = 0.3 * torch.randn(n, n_samples, 2, device='cuda', generator=gen)
    consts = rendering._constants()
    fwd = median_ms(lambda: ops.thomson_integral_fwd(raw, z, rays_o, rays_d, consts, kappa), repeats)
    if not backward:
        return fwd, 0.0
    g_b = torch.randn(n, 2, device='cuda', generator=gen)
    bwd = median_ms(lambda: ops.thomson_integral_bwd(raw, z, rays_o, rays_d, consts, kappa, g_b), repeats)
    return fwd, bwd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--resolution', type=int, default=1024)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--batch', type=int, default=32768)
    ap.add_argument('--no-mhd', action='store_true')
    args = ap.parse_args()
    from sunerf.rendering.functional import LN10
    from sunerf.rendering.thompson import ThompsonScattering
    from sunerf_hip import ops
    from sunerf_hip.rays import fov_axis, pose_spherical, render_frame, observer_rays

    torch.manual_seed(0)
    cfg = dict(Rs_per_ds=1.0, sampling_config={'type': 'stratified', 'n_samples': 64, 'perturb': False},
               hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 128})
    nerf = ThompsonScattering(model_config={'d_filter': 256}, **{k: dict(v) if isinstance(v, dict) else v
                                                                  for k, v in cfg.items()}).cuda()
    res = args.resolution
    axis = fov_axis(res, 1.1 * 960. / 206264.806, 'cuda')
    c2w = pose_spherical(-0.3, 0.1, 215.032)
    result = {'resolution': res, 'samples': [64, 128], 'library': os.path.basename(ops._l.LIB_PATH)}

    def frame_ms(rendering):
        with torch.no_grad():
            return median_ms(lambda: render_frame(rendering, axis, axis, c2w, 0.3, tile_rays=1 << 18,
                                                  keys=('image',)), args.repeats)

    o, d = observer_rays(res, device='cuda')
    k64, _ = kernel_ms(ops, nerf, o, d, 64, args.repeats, LN10, False)
    k192, _ = kernel_ms(ops, nerf, o, d, 192, args.repeats, LN10, False)
    f_nerf = frame_ms(nerf)
    result['nerf_frame_ms'] = round(f_nerf, 2)
    result['frame_thomson_fwd_ms'] = round(k64 + k192, 3)
    result['nerf_frame_thomson_share'] = round((k64 + k192) / f_nerf, 4)

    if not args.no_mhd:
        from mhd_render_time import Reader, psi_like_frame
        from sunerf.model.mhd_model import MHDModel
        frames = {2531: psi_like_frame(1), 2532: psi_like_frame(2)}
        with tempfile.TemporaryDirectory() as tmp:
            for var in ('rho', 't'):
                os.makedirs(os.path.join(tmp, var))
                for f in frames:
                    open(os.path.join(tmp, var, f'{var}00{f}.h5'), 'w').close()
            mhd = ThompsonScattering(model=MHDModel, model_config={'data_path': tmp, 'reader': Reader(frames)},
                                     **{k: dict(v) if isinstance(v, dict) else v for k, v in cfg.items()}).cuda()
            f_mhd = frame_ms(mhd)
        result['mhd_frame_ms'] = round(f_mhd, 2)
        result['mhd_frame_thomson_share'] = round((k64 + k192) / f_mhd, 4)

    # training step: 32768 rays, coarse + fine pass, MSE on tB / pB, backward into the MLP parameters
    n = args.batch
    o_t, d_t = o[:n].contiguous(), d[:n].contiguous()
    t_t = torch.rand(n, 1, device='cuda')
    target = torch.rand(n, 2, device='cuda')
    params = list(nerf.parameters())

    def step():
        for p in params:
            p.grad = None
        out = nerf(o_t, d_t, t_t)
        loss = ((out['coarse_image'] - target) ** 2).mean() + ((out['fine_image'] - target) ** 2).mean()
        loss.backward()
    step_ms = median_ms(step, args.repeats)
    f64, b64 = kernel_ms(ops, nerf, o_t, d_t, 64, args.repeats, LN10, True)
    f192, b192 = kernel_ms(ops, nerf, o_t, d_t, 192, args.repeats, LN10, True)
    result.update(step_rays=n, step_ms=round(step_ms, 2),
                  step_thomson_fwd_ms=round(f64 + f192, 4), step_thomson_bwd_ms=round(b64 + b192, 4),
                  step_thomson_share=round((f64 + f192 + b64 + b192) / step_ms, 4),
                  kernel_fwd_1024sq_x192_ms=round(k192, 3), kernel_bwd_32768_x192_ms=round(b192, 4))
    print(json.dumps(result))


if __name__ == '__main__':
    main()
