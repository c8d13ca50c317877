"""Times the voxel-grid field (csrc/grid_field.hip) on a ROCm device, every figure a median of ``--reps`` calls
bracketed by device events after a warm-up:

1. the gather (forward), the gather that also leaves the backward's index, and the backward (stable sort of the cell ids,
   segment starts, the two scatter kernels) on ``--rays`` x ``--samples`` samples (default 32768 x 192) of rays through the
   corona, for a 128^3 cube and a 91 x 181 x 64 spherical shell, two channels;
2. a ``--frame``^2 frame (default 1024) rendered from a cube of ``--cube``^3 nodes (default 256) baked from a network, next
   to the same frame from the network itself, alternating in one timed loop, and the PSNR of the baked frame against the
   network's, over the whole frame and off the disk.  The cube spans +-``--half-width`` solar radii (default 2.1: the samples of a frame 2.2 solar radii wide reach
   2.03 from the centre; outside the cube a field answers its fill).  The network (8 x ``--d-filter``) is first trained for ``--train-steps`` steps on the analytic disk + corona of
   tools/closed_loop.py, so that the field it bakes is a corona and not the noise of a fresh initialisation (a network
   trained for a few hundred steps still carries structure below the voxel size, which no cube reproduces).

    python tools/grid_field_time.py [--rays 32768] [--samples 192] [--reps 7] [--frame 1024] [--cube 256] [--half-width 2.1]
                                    [--d-filter 256] [--train-steps 3000] [--skip-frame] [--skip-kernels]
"""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, '2024-hl-spi3s-sunerf_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def timed(fn, reps):
    import torch
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


def show(what, t, extra=''):
    print(f'{what:58s} median {statistics.median(t):9.3f} ms  min {min(t):9.3f}  max {max(t):9.3f}  ({len(t)} runs){extra}')


def kernels(args):
    import numpy as np
    import torch
    from sunerf.model.grid_model import GridField
    from sunerf_hip import grid_field as gf
    from sunerf_hip.volume import CartesianGrid, SphericalGrid
    gen = torch.Generator().manual_seed(1)
    n, s = args.rays, args.samples
    o = torch.randn(n, 3, generator=gen)
    o = o / o.norm(dim=1, keepdim=True) * 215.
    target = torch.randn(n, 3, generator=gen)
    target = target / target.norm(dim=1, keepdim=True) * (1.25 * torch.rand(n, 1, generator=gen))
    d = target - o
    dist = d.norm(dim=1, keepdim=True)
    d = d / dist
    z = dist + torch.linspace(-1.3, 1.3, s)[None, :]
    o, d, z = o.float().cuda(), d.float().cuda(), z.float().contiguous().cuda()
    grids = {'cube 128^3': CartesianGrid.cube(1.3, 128),
             'shell 91 x 181 x 64': SphericalGrid(np.linspace(-math.pi / 2, math.pi / 2, 91), np.linspace(-math.pi, math.pi, 181),
                                                  np.linspace(1.0, 1.6, 64))}
    total = n * s
    for name, grid in grids.items():
        field = GridField(grid, d_output=2, init=torch.randn(*grid.shape, 2, generator=gen)).cuda()
        desc, values = field.descriptor(), field.values.detach()
        raw, index = gf.grid_field_rays(desc, values, o, d, z, want_index=True)
        inside = (index[0] < desc.n_cells).float().mean().item()
        g_raw = torch.randn_like(raw)
        what = f'{name}, {n} x {s} samples ({inside:.0%} inside)'
        fwd = timed(lambda: gf.grid_field_rays(desc, values, o, d, z), args.reps)
        show(f'{what}: forward', fwd, f'  {total / statistics.median(fwd) / 1e6:.2f} G samples/s')
        fwd_i = timed(lambda: gf.grid_field_rays(desc, values, o, d, z, want_index=True), args.reps)
        show(f'{what}: forward + index', fwd_i)
        bwd = timed(lambda: gf.grid_field_bwd(desc, g_raw, index), args.reps)
        show(f'{what}: backward', bwd, f'  {statistics.median(bwd) / statistics.median(fwd):.1f} x the forward')
        sort = timed(lambda: torch.sort(index[0], stable=True), args.reps)
        show(f'{what}:   of which the stable sort', sort)


def frame(args):
    import torch
    from closed_loop import emission_problem
    from sunerf.evaluation.loader import ModelLoader
    from sunerf.model.grid_model import GridField
    from sunerf.model.sunerf import fit_steps
    from sunerf.rendering.emission import EmissionRadiativeTransfer
    from sunerf_hip.feed import training_batches
    from sunerf_hip.volume import CartesianGrid
    torch.manual_seed(0)
    size = 64
    small = {'shape': (size, size), 'cdelt': (2.2 * 960. / size, 2.2 * 960. / size), 'meta': {'t_obs': '2022-01-01T00:00:00.000'}}
    poses = [(0.1 * (k % 3 - 1), 0.3 - 6.2832 / 8 * k) for k in range(8)]
    problem = argparse.Namespace(size=size, d_filter=args.d_filter, steps=max(args.train_steps, 1))
    obs, module = emission_problem(problem, small, poses)
    module.strict_finite_check = False
    if args.train_steps > 0:
        fit_steps(module, training_batches(obs.pool(batch_size=2048, seed=0, reshuffle='rays'), args.train_steps))
    net = module.rendering
    for sampler in (net.sampler, net.sampler_hierarchical):                # a frame is rendered without jitter
        if hasattr(sampler, 'perturb'):
            sampler.perturb = False
    grid = CartesianGrid.cube(args.half_width, args.cube)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    baked = EmissionRadiativeTransfer(Rs_per_ds=1.0, model=GridField, model_config={'grid': CartesianGrid.cube(1.3, 2)},
                                      sampling_config={'type': 'stratified', 'n_samples': 64, 'perturb': False},
                                      hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 128, 'perturb': False})
    baked.fine_model, baked.coarse_model = GridField.bake(net, grid, 0.0), GridField.bake(net, grid, 0.0, model='coarse')
    baked = baked.cuda()
    ev[1].record()
    ev[1].synchronize()
    print(f'baking two {args.cube}^3 cubes from the 8 x {args.d_filter} network: {ev[0].elapsed_time(ev[1]):.1f} ms')
    res = args.frame
    big = {'shape': (res, res), 'cdelt': (2.2 * 960. / res, 2.2 * 960. / res), 'meta': {'t_obs': '2022-01-01T00:00:00.000'}}
    loaders = {'network': ModelLoader(rendering=net, model=net.fine_model, ref_map=big),
               'baked cube': ModelLoader(rendering=baked, model=baked.fine_model, ref_map=big)}
    frames, times = {}, {k: [] for k in loaders}
    for k, loader in loaders.items():                                       # warm-up, and the frames that are compared
        frames[k] = loader.render_observer_image(0.1, 0.3, 0.0, as_numpy=False)['image']
    torch.cuda.synchronize()
    for _ in range(args.reps):                                              # alternating: drift and neighbours hit both alike
        for k, loader in loaders.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            loader.render_observer_image(0.1, 0.3, 0.0, as_numpy=False)
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    what = f'{res} x {res} frame, 64 + 128 samples'
    for k, t in times.items():
        show(f'{what}: {k}', t)
    print(f'{what}: network / baked cube = {statistics.median(times["network"]) / statistics.median(times["baked cube"]):.1f}')
    a, b = frames['baked cube'].double(), frames['network'].double()
    peak = b.max().item()
    mse = ((a - b) ** 2).mean().item()
    print(f'baked {args.cube}^3 frame against the network\'s: PSNR {10 * math.log10(peak * peak / mse):.2f} dB '
          f'(peak {peak:.4f}, rmse {math.sqrt(mse):.3e})')
    # the corona alone: pixels whose line of sight passes the centre at more than 1.05 solar radii (the disk's brightness comes
    # from a layer at the photosphere that is thinner than a voxel)
    from sunerf.evaluation.loader import AU_IN_SOLAR_RADII, linear_plate_scale_axes
    tx, ty = linear_plate_scale_axes(big, None, 'cuda')
    impact = AU_IN_SOLAR_RADII * torch.sqrt(torch.tan(tx)[None, :] ** 2 + torch.tan(ty)[:, None] ** 2)
    off = (impact > 1.05).reshape(-1)
    a, b = a.reshape(-1)[off], b.reshape(-1)[off]
    peak, mse = b.max().item(), ((a - b) ** 2).mean().item()
    print(f'  off the disk (impact parameter > 1.05, {off.float().mean().item():.0%} of the pixels): PSNR '
          f'{10 * math.log10(peak * peak / mse):.2f} dB (peak {peak:.4f}, rmse {math.sqrt(mse):.3e})')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rays', type=int, default=32768)
    ap.add_argument('--samples', type=int, default=192)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--frame', type=int, default=1024)
    ap.add_argument('--cube', type=int, default=256)
    ap.add_argument('--half-width', type=float, default=2.1, help='of the baked cube [solar radii]: it must hold every sample of a frame')
    ap.add_argument('--d-filter', type=int, default=256)
    ap.add_argument('--train-steps', type=int, default=3000)
    ap.add_argument('--skip-frame', action='store_true')
    ap.add_argument('--skip-kernels', action='store_true')
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('grid_field_time.py measures on a ROCm device; none is visible')
    if not args.skip_kernels:
        kernels(args)
    if not args.skip_frame:
        frame(args)


if __name__ == '__main__':
    main()
