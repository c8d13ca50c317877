"""Cost of the reprojection baseline on the device (csrc/reprojection.hip, sunerf_hip.reprojection).

(a) a ``--map`` (1024 x 2048) synchronic map from 3 and from ``--views`` (64) views of ``--size``^2 (1024^2) pixels, one and
seven channels: CUDA-event medians over ``--repeats`` calls after one warm-up of the map launch alone (``map_rows``) and of
the whole ``synchronic_map`` (launch + fill + the covered count's host read); (b) ``load_views``' 703 observers of
``--observer-size``^2 (256^2) pixels from that map in one launch.  Bytes moved -- every source plane and the map read once,
the outputs written once -- next to the measured 6.3 TB/s copy rate of DESIGN.md 8e.  With ``--host`` also the host route:
the fp64 numpy restatement of tests/reprojection_reference.py on the same inputs (single thread, as numpy runs it; one
observer, scaled to 703).  The kernels' own times come from a separate
``rocprofv3 --kernel-trace --stats -- python tools/reprojection_time.py`` run.  One JSON line.

    python tools/reprojection_time.py [--views 64] [--size 1024] [--map 1024 2048] [--observer-size 256] [--repeats 10] [--host]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, '2024-hl-spi3s-sunerf_amd'), os.path.join(ROOT, 'tests')]

HBM_BYTES_PER_S = 6.3e12          # measured float4 copy rate
WL7 = [94., 131., 171., 193., 211., 304., 335.]


def observation_set(n_views, size, channels):
    from sunerf_hip.observations import ObservationSet
    obs = ObservationSet(device='cuda')
    grid = {'shape': (size, size), 'cdelt': (2400. / size, 2400. / size)}
    g = torch.Generator(device='cuda').manual_seed(size + channels)
    for k in range(n_views):
        image = torch.rand(channels, size, size, device='cuda', generator=g)
        obs.add_view(image, 0.1 * (k % 3 - 1), 6.2832 / n_views * k, 215.032, time=0.0, grid=grid,
                     wavelengths=WL7[:channels] if channels > 1 else None)
    return obs


def event_median(fn, repeats):
    fn()                                                  # warm-up
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


def rates(ms, moved):
    return {'bytes_moved': moved, 'moved_GB_per_s': moved / ms / 1e6, 'fraction_of_copy_rate': moved / ms / 1e-3 / HBM_BYTES_PER_S,
            'bound_ms_at_copy_rate': moved / HBM_BYTES_PER_S * 1e3}


def map_cost(obs, shape, repeats):
    from sunerf_hip.reprojection import map_axes, map_rows, synchronic_map
    lat, lon = (torch.from_numpy(a).cuda() for a in map_axes(shape))
    ms, spread = event_median(lambda: map_rows(obs.views, lat, lon), repeats)
    whole, _ = event_median(lambda: synchronic_map(obs.views, shape=shape), repeats)
    h_map = synchronic_map(obs.views, shape=shape)
    moved = sum(v.image.numel() * 4 for v in obs.views) + h_map.image.numel() * 8      # planes read once; map + footprint written
    out = {'views': len(obs.views), 'channels': int(h_map.image.shape[0]), 'map_launch_ms': ms, 'spread_ms': spread,
           'synchronic_map_ms': whole, 'covered_fraction': h_map.covered_fraction}
    out.update(rates(ms, moved))
    return h_map, out


def views_cost(h_map, size, repeats):
    from sunerf_hip.reprojection import Observer, view_grid_coordinates
    axis = torch.linspace(-1200., 1200., size, dtype=torch.float64, device='cuda') * (np.pi / 180. / 3600.)
    observers = [Observer(np.deg2rad(float(b)), np.deg2rad(float(l)), tx=axis, ty=axis) for b, l in view_grid_coordinates(10)]
    ms, spread = event_median(lambda: h_map.reproject_many(observers), repeats)
    n = len(observers) * size * size * h_map.image.shape[0]
    out = {'observers': len(observers), 'size': size, 'channels': int(h_map.image.shape[0]), 'launch_ms': ms, 'spread_ms': spread,
           'ms_per_observer': ms / len(observers)}
    out.update(rates(ms, n * 4 + h_map.image.numel() * 4))
    return out


def host_route(obs, h_map, shape, size):
    """The numpy restatement (fp64, one thread) on the same inputs: the coadd of all views, and one observer."""
    import reprojection_reference as ref
    from sunerf_hip.reprojection import map_axes
    lat, lon = map_axes(shape)
    views = [dict(planes=v.image.cpu().numpy(), wavelengths=v.wavelength, downscale=v.downscale, tx=v.tx.cpu().numpy(),
                  ty=v.ty.cpu().numpy(), c2w=v.c2w[:3, :4].numpy()) for v in obs.views]
    t0 = time.perf_counter()
    ref.synchronic_map(views, lat, lon, 1.0)
    t1 = time.perf_counter()
    axis = np.linspace(-1200., 1200., size) * (np.pi / 180. / 3600.)
    from sunerf_hip.rays import pose_spherical
    ref.reproject(h_map.image.cpu().numpy(), lat, lon, 1.0, dict(tx=axis, ty=axis, c2w=pose_spherical(-0.3, 0.1, 215.032)[:3, :4].numpy()))
    t2 = time.perf_counter()
    return {'views': len(views), 'map_s': t1 - t0, 'one_observer_s': t2 - t1, 'observers_703_s_scaled': 703 * (t2 - t1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--views', type=int, default=64)
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--map', type=int, nargs=2, default=(1024, 2048))
    ap.add_argument('--observer-size', type=int, default=256)
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--host', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('reprojection_time.py needs a ROCm device')
    shape = tuple(args.map)
    out = {'map_shape': shape, 'view_size': args.size, 'hbm_rate': 'measured 6.3 TB/s', 'maps': [], 'views': []}
    for channels in (1, 7):
        for n_views in (3, args.views):
            obs = observation_set(n_views, args.size, channels)
            h_map, cost = map_cost(obs, shape, args.repeats)
            out['maps'].append(cost)
            if n_views == 3:
                out['views'].append(views_cost(h_map, args.observer_size, args.repeats))
                if args.host and channels == 1:
                    out['host_route_single_channel_3_views'] = host_route(obs, h_map, shape, args.observer_size)
            del obs, h_map
            torch.cuda.empty_cache()
    print(json.dumps({'reprojection_time': out}))


if __name__ == '__main__':
    main()
