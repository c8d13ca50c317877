"""Times the line-of-sight DEM of a frame (ModelLoader.render_dem_image) next to the plain DT render of the
same frame (ModelLoader.render_observer_image, all seven channels) in the same session: both alternate inside one timed loop,
each call bracketed by device events after a warm-up of both, and the medians and the spread are printed.

    python tools/dem_time.py [--model star|nerf] [--resolution 512] [--samples 64] [--reps 7] [--d-filter 256]
    python tools/dem_time.py --profile ...          # one warm-up + one call of each and nothing else: run it under
        rocprofv3 --kernel-trace --stats -d <dir> -- python tools/dem_time.py --profile ...
    python tools/dem_time.py --share <dir>          # the DEM kernel's share of the GPU time in that directory's *_kernel_stats.csv

The DEM frame runs the sampler, the coarse pass, the resampler and the fine field like the render, and replaces the fine DT
integral (7 channels) by the DEM kernel (one optical depth, 101 bins), so a ratio near 1 is expected; only the MLP matters."""
import argparse
import csv
import glob
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, '2024-hl-spi3s-sunerf_amd'))

AIA = (94, 131, 171, 193, 211, 304, 335)


def share(directory):
    rows = []
    for path in glob.glob(os.path.join(directory, '**', '*kernel_stats.csv'), recursive=True):
        with open(path, newline='') as f:
            rows += list(csv.DictReader(f))
    if not rows:
        sys.exit(f'no *kernel_stats.csv under {directory}')
    total = sum(float(r['TotalDurationNs']) for r in rows)
    print(f'{"kernel":60s} {"calls":>6s} {"total ms":>10s} {"share":>7s}')
    for r in sorted(rows, key=lambda r: -float(r['TotalDurationNs']))[:12]:
        print(f'{r["Name"][:60]:60s} {r["Calls"]:>6s} {float(r["TotalDurationNs"]) / 1e6:10.3f} {float(r["TotalDurationNs"]) / total:7.2%}')
    dem = sum(float(r['TotalDurationNs']) for r in rows if 'dem_integral_kernel' in r['Name'])
    print(f'dem_integral_kernel: {dem / 1e6:.3f} ms of {total / 1e6:.3f} ms GPU time = {dem / total:.2%}')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--model', choices=('star', 'nerf'), default='star')
    ap.add_argument('--resolution', type=int, default=512)
    ap.add_argument('--samples', type=int, default=64, help='coarse and fine samples per ray, each')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--d-filter', type=int, default=256)
    ap.add_argument('--profile', action='store_true')
    ap.add_argument('--share', metavar='DIR')
    args = ap.parse_args()
    if args.share:
        return share(args.share)

    import numpy as np
    import torch
    from sunerf.evaluation.loader import ModelLoader
    from sunerf.rendering.density_temperature import DensityTemperatureRadiativeTransfer
    if not torch.cuda.is_available():
        sys.exit('dem_time.py measures on a ROCm device; none is visible')
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'g6_dt_e2e.npz'))
    common = dict(Rs_per_ds=1.0, sampling_config={'type': 'stratified', 'n_samples': args.samples, 'perturb': False},
                  hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': args.samples},
                  pixel_intensity_factor=float(g['pixel_intensity_factor']), response_table=(g['aia_logte'], g['aia_tresp']))
    torch.manual_seed(7)
    if args.model == 'star':
        from sunerf.model.stellar_model import SimpleStar
        mod = DensityTemperatureRadiativeTransfer(model=SimpleStar, model_config={}, **common)
    else:
        from sunerf.model.model import NeRF_DT
        mod = DensityTemperatureRadiativeTransfer(model=NeRF_DT, model_config={'d_filter': args.d_filter}, **common)
    res = args.resolution
    grid = {'shape': (res, res), 'cdelt': (2400. / res, 2400. / res), 'meta': {'t_obs': '2022-01-01T00:00:00.000'}}
    loader = ModelLoader(rendering=mod.cuda(), model=mod.fine_model, ref_map=grid)
    wl = np.array(AIA)

    def image():
        return loader.render_observer_image(0.1, 0.3, 0.4, wl=wl, as_numpy=False)

    def dem():
        return loader.render_dem_image(0.1, 0.3, 0.4, as_numpy=False)

    for fn in (image, dem, image, dem):          # warm-up of both, every shape of the timed loop
        fn()
    torch.cuda.synchronize()
    if args.profile:
        image(); dem()
        torch.cuda.synchronize()
        return
    times = {'image': [], 'dem': []}
    for _ in range(args.reps):                   # alternating: drift and neighbours hit both alike
        for name, fn in (('image', image), ('dem', dem)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b))
    what = f'{args.model}{"" if args.model == "star" else f" d_filter {args.d_filter}"}, {res}x{res}, {args.samples}+{args.samples} samples'
    for name, t in times.items():
        print(f'{what}: {name:5s} median {statistics.median(t):9.3f} ms  min {min(t):9.3f}  max {max(t):9.3f}  ({len(t)} runs)')
    print(f'{what}: DEM frame / DT frame = {statistics.median(times["dem"]) / statistics.median(times["image"]):.3f}')


if __name__ == '__main__':
    main()
