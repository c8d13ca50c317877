"""Times the voxel-grid field with a time axis (csrc/dynamic_grid.hip) on a ROCm device next to the static field
(csrc/grid_field.hip) on the same cube, measured in the same process and alternating with it; every figure a median of
``--reps`` calls bracketed by device events after a warm-up.  Nothing about speed is asserted.

1. ``--rays`` x ``--samples`` samples (default 32768 x 192) of rays through the corona, two channels, a ``--grid``^3 cube
   (default 128) with ``--frames`` frames (default 8): the gather (forward), the gather that also leaves the backward's index,
   and the backward split into its three parts -- the stable sort of the ids, the segment search (``searchsorted`` of
   ``(T - 1) n_cells + 1`` ids against the sorted ones) and the two scatter kernels.  The dynamic forward does twice the gathers
   of the static one; its backward carries 36 instead of 28 bytes of index per sample and ``T - 1`` times the segment starts.
2. a ``--frame``^2 frame (default 1024) rendered from a sequence of ``--cube``^3 cubes baked from a network at ``--frames``
   times, from the network itself and from one static cube baked at the frame's time, alternating in one timed loop.  The
   network (8 x ``--d-filter``) is first trained for ``--train-steps`` steps on the analytic disk + corona of
   tools/closed_loop.py, as tools/grid_field_time.py does.

    python tools/dynamic_grid_time.py [--rays 32768] [--samples 192] [--grid 128] [--frames 8] [--reps 7] [--frame 1024]
                                      [--cube 128] [--half-width 2.1] [--d-filter 256] [--train-steps 1000] [--skip-frame]
                                      [--skip-kernels]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, '2024-hl-spi3s-sunerf_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def event_time(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def timed_alternating(fns, reps):
    """``{name: [ms] * reps}`` of the callables, one warm-up each, then alternating: drift and neighbours hit all alike."""
    import torch
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            out[k].append(event_time(fn))
    return out


def show(what, t, extra=''):
    print(f'{what:60s} median {statistics.median(t):9.3f} ms  min {min(t):9.3f}  max {max(t):9.3f}  ({len(t)} runs){extra}')


def kernels(args):
    import torch
    from sunerf.model.grid_model import DynamicGridField, GridField
    from sunerf_hip import dynamic_grid as dg
    from sunerf_hip import grid_field as gf
    from sunerf_hip import lib as _l
    from sunerf_hip.ops import _ptr, _stream
    from sunerf_hip.volume import CartesianGrid
    gen = torch.Generator().manual_seed(1)
    n, s, frames = args.rays, args.samples, args.frames
    o = torch.randn(n, 3, generator=gen)
    o = o / o.norm(dim=1, keepdim=True) * 215.
    target = torch.randn(n, 3, generator=gen)
    target = target / target.norm(dim=1, keepdim=True) * (1.25 * torch.rand(n, 1, generator=gen))
    d = target - o
    dist = d.norm(dim=1, keepdim=True)
    d = d / dist
    z = dist + torch.linspace(-1.3, 1.3, s)[None, :]
    t = torch.rand(n, 1, generator=gen)
    o, d, z, t = o.float().cuda(), d.float().cuda(), z.float().contiguous().cuda(), t.float().cuda()
    grid = CartesianGrid.cube(1.3, args.grid)
    tau = [k / (frames - 1) for k in range(frames)]
    dyn = DynamicGridField(grid, d_output=2, init=torch.randn(frames, *grid.shape, 2, generator=gen), frame_times=tau).cuda()
    sta = GridField(grid, d_output=2, init=torch.randn(*grid.shape, 2, generator=gen)).cuda()
    dd, dv = dyn.descriptor(), dyn.values.detach()
    sd, sv = sta.descriptor(), sta.values.detach()
    raw, d_index = dg.dynamic_grid_rays(dd, dv, o, d, z, t, want_index=True)
    _, s_index = gf.grid_field_rays(sd, sv, o, d, z, want_index=True)
    g_raw = torch.randn_like(raw)
    inside = (d_index[0] < dd.n_ids).float().mean().item()
    dev = raw.device
    total = n * s
    print(f'{args.grid}^3 cube, {frames} frames, {n} x {s} samples ({inside:.0%} inside), 2 channels; '
          f'seg_start of the dynamic field: {(dd.n_ids + 1) * 8 / 1e6:.1f} MB, of the static field: {(sd.n_cells + 1) * 8 / 1e6:.1f} MB')

    def sort_of(index):
        return torch.sort(index[0], stable=True)

    def search_of(ids, count):
        return torch.searchsorted(ids, torch.arange(count + 1, dtype=torch.int32, device=dev))

    d_ids, d_perm = sort_of(d_index)
    s_ids, s_perm = sort_of(s_index)
    d_seg, s_seg = search_of(d_ids, dd.n_ids), search_of(s_ids, sd.n_cells)
    lib = _l.load()
    d_bytes = lib.sunerf_dynamic_grid_bwd_workspace_bytes(total, 2)
    s_bytes = lib.sunerf_grid_field_bwd_workspace_bytes(total, 2)
    d_ws, s_ws = (torch.empty(b, dtype=torch.uint8, device=dev) for b in (d_bytes, s_bytes))
    d_out, s_out = torch.empty_like(dv), torch.empty_like(sv)

    def d_kernels():
        _l.call(dev, 'sunerf_dynamic_grid_bwd', dd.ref(), dd.n_frames, _ptr(g_raw), _ptr(d_index[0]), _ptr(d_index[1]), _ptr(d_perm),
                _ptr(d_seg), total, _ptr(d_ws), d_bytes, _ptr(d_out), 0, _stream(dev))

    def s_kernels():
        _l.call(dev, 'sunerf_grid_field_bwd', sd.ref(), _ptr(g_raw), _ptr(s_index[0]), _ptr(s_index[1]), _ptr(s_perm), _ptr(s_seg),
                total, _ptr(s_ws), s_bytes, _ptr(s_out), 0, _stream(dev))

    rows = [('forward', lambda: dg.dynamic_grid_rays(dd, dv, o, d, z, t), lambda: gf.grid_field_rays(sd, sv, o, d, z)),
            ('forward + index', lambda: dg.dynamic_grid_rays(dd, dv, o, d, z, t, want_index=True),
             lambda: gf.grid_field_rays(sd, sv, o, d, z, want_index=True)),
            ('backward', lambda: dg.dynamic_grid_bwd(dd, g_raw, d_index), lambda: gf.grid_field_bwd(sd, g_raw, s_index)),
            ('  of which the stable sort', lambda: sort_of(d_index), lambda: sort_of(s_index)),
            ('  of which the segment search', lambda: search_of(d_ids, dd.n_ids), lambda: search_of(s_ids, sd.n_cells)),
            ('  of which the two kernels', d_kernels, s_kernels)]
    for what, dyn_fn, sta_fn in rows:
        got = timed_alternating({'dynamic': dyn_fn, 'static': sta_fn}, args.reps)
        md, ms = statistics.median(got['dynamic']), statistics.median(got['static'])
        show(f'{what}: dynamic', got['dynamic'], f'  {total / md / 1e6:.2f} G samples/s' if what == 'forward' else '')
        show(f'{what}: static', got['static'], f'  dynamic / static = {md / ms:.2f}')


def frame(args):
    import torch
    from closed_loop import emission_problem
    from sunerf.evaluation.loader import ModelLoader
    from sunerf.model.grid_model import DynamicGridField, GridField
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
    tau = [k / (args.frames - 1) for k in range(args.frames)]
    when = 0.5 * (tau[0] + tau[1])                                         # between two baked times
    cfg = dict(sampling_config={'type': 'stratified', 'n_samples': 64, 'perturb': False},
               hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 128, 'perturb': False})
    tiny = CartesianGrid.cube(1.3, 2)
    sequence = EmissionRadiativeTransfer(Rs_per_ds=1.0, model=DynamicGridField, model_config={'grid': tiny, 'frame_times': tau},
                                         **{k: dict(v) for k, v in cfg.items()})

    def bake_sequence():
        sequence.fine_model, sequence.coarse_model = DynamicGridField.bake(net, grid, tau), DynamicGridField.bake(net, grid, tau, model='coarse')

    def bake_static():
        static.fine_model, static.coarse_model = GridField.bake(net, grid, when), GridField.bake(net, grid, when, model='coarse')
    ms = event_time(bake_sequence)
    print(f'baking two sequences of {args.frames} x {args.cube}^3 from the 8 x {args.d_filter} network: {ms:.1f} ms')
    static = EmissionRadiativeTransfer(Rs_per_ds=1.0, model=GridField, model_config={'grid': tiny}, **{k: dict(v) for k, v in cfg.items()})
    ms = event_time(bake_static)
    print(f'baking two static {args.cube}^3 cubes at t = {when:.4f}: {ms:.1f} ms')
    sequence, static = sequence.cuda(), static.cuda()
    res = args.frame
    big = {'shape': (res, res), 'cdelt': (2.2 * 960. / res, 2.2 * 960. / res), 'meta': {'t_obs': '2022-01-01T00:00:00.000'}}
    loaders = {'network': ModelLoader(rendering=net, model=net.fine_model, ref_map=big),
               'baked sequence': ModelLoader(rendering=sequence, model=sequence.fine_model, ref_map=big),
               'static bake': ModelLoader(rendering=static, model=static.fine_model, ref_map=big)}
    times = timed_alternating({k: (lambda loader=loader: loader.render_observer_image(0.1, 0.3, when, as_numpy=False))
                               for k, loader in loaders.items()}, args.reps)
    what = f'{res} x {res} frame at t = {when:.4f}, 64 + 128 samples'
    for k, v in times.items():
        show(f'{what}: {k}', v)
    med = {k: statistics.median(v) for k, v in times.items()}
    print(f'{what}: network / baked sequence = {med["network"] / med["baked sequence"]:.1f}, '
          f'baked sequence / static bake = {med["baked sequence"] / med["static bake"]:.2f}')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rays', type=int, default=32768)
    ap.add_argument('--samples', type=int, default=192)
    ap.add_argument('--grid', type=int, default=128)
    ap.add_argument('--frames', type=int, default=8)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--frame', type=int, default=1024)
    ap.add_argument('--cube', type=int, default=128)
    ap.add_argument('--half-width', type=float, default=2.1, help='of the baked cubes [solar radii]: they must hold every sample of a frame')
    ap.add_argument('--d-filter', type=int, default=256)
    ap.add_argument('--train-steps', type=int, default=1000)
    ap.add_argument('--skip-frame', action='store_true')
    ap.add_argument('--skip-kernels', action='store_true')
    args = ap.parse_args()
    if args.frames < 2:
        sys.exit('--frames must be at least 2')
    import torch
    if not torch.cuda.is_available():
        sys.exit('dynamic_grid_time.py measures on a ROCm device; none is visible')
    if not args.skip_kernels:
        kernels(args)
    if not args.skip_frame:
        frame(args)


if __name__ == '__main__':
    main()
