"""Cost of building a training set on the device (csrc/observations.hip, sunerf_hip.observations) against the host route.

Per set -- ``--views`` views of ``--size``^2 pixels, single channel and 7 channels -- the milliseconds of one
``sunerf_build_ray_pool`` launch over the whole set (CUDA-event median over ``--repeats`` builds after one warm-up; this is
also the cost of one ``reshuffle='rays'`` epoch rebuild on one rank), the bytes it writes and reads per second next to the
6.3 TB/s copy rate of DESIGN.md 8e, and its ratio to one training step at 32768 rays (20.7 ms, README).  For the
single-channel set also the route the package offered before: the host assembly of the reference
(``single_channel.py:44-52``: flatten, time broadcast, ``np.random.permutation``, fancy index -- numpy runs these on one
thread whatever the thread count) on arrays that are already in host memory, plus the ``RayPool`` upload.  The kernel's own
time comes from a separate ``rocprofv3 --kernel-trace --stats -- python tools/observation_time.py --no-host`` run.  One JSON line.

    python tools/observation_time.py [--views 64] [--size 1024] [--repeats 10] [--no-host]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, '2024-hl-spi3s-sunerf_amd')]

HBM_BYTES_PER_S = 6.3e12          # measured float4 copy rate
STEP_MS_32768 = 20.7              # one training step at 32768 rays (README)
WL7 = [94., 131., 171., 193., 211., 304., 335.]


def observation_set(n_views, size, channels):
    from sunerf_hip.observations import ObservationSet
    obs = ObservationSet(device='cuda')
    grid = {'shape': (size, size), 'cdelt': (2400. / size, 2400. / size)}
    g = torch.Generator(device='cuda').manual_seed(size + channels)
    for k in range(n_views):
        image = torch.rand(channels, size, size, device='cuda', generator=g)
        obs.add_view(image, 0.1 * (k % 3 - 1), 0.0982 * k, 215.032, time=0.01 * k, grid=grid,
                     wavelengths=WL7[:channels] if channels > 1 else None)
    return obs


def device_build(obs, repeats):
    pool = obs.pool(batch_size=32768, seed=0, reshuffle='rays')           # the warm-up build
    torch.cuda.synchronize()
    times = []
    for epoch in range(1, repeats + 1):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        pool.rebuild(epoch)
        stop.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(stop))
    ms = sorted(times)[len(times) // 2]
    written = sum(v.numel() * 4 for v in pool.data.values())
    read = sum(v.image.numel() * 4 for v in obs.views)                    # every pixel once; angles and descriptors are cached
    return pool, {'rays': pool.n_rays, 'ms_per_build': ms, 'spread_ms': [min(times), max(times)], 'bytes_written': written,
                  'bytes_read': read, 'written_GB_per_s': written / ms / 1e6, 'moved_GB_per_s': (written + read) / ms / 1e6,
                  'bound_ms_at_copy_rate': (written + read) / HBM_BYTES_PER_S * 1e3,
                  'builds_per_training_step_32768': STEP_MS_32768 / ms, 'rebuild_over_step': ms / STEP_MS_32768}


def host_route(obs):
    """single_channel.py:44-52 on host arrays + the RayPool upload; the per-view rays and images are fetched beforehand (the
    reference holds them in host memory at that point too) and that fetch is not timed."""
    from sunerf_hip.feed import RayPool
    from sunerf_hip.rays import grid_rays
    rays, images, times = [], [], []
    for v in obs.views:
        o, d = grid_rays(v.tx, v.ty, v.c2w)
        rays.append(torch.stack([o, d], 1).cpu().numpy().reshape(v.height, v.width, 2, 3))
        images.append(v.image[0].cpu().numpy())
        times.append(v.time)
    rays, images, times = np.stack(rays), np.stack(images), np.array(times, dtype=np.float32)
    t0 = time.perf_counter()
    flat_rays = rays.reshape((-1, 2, 3))
    flat_times = (np.ones_like(images) * times[:, None, None]).reshape(-1, 1)
    flat_images = images.reshape(-1, 1)
    r = np.random.permutation(flat_rays.shape[0])
    flat_rays, flat_times, flat_images = flat_rays[r], flat_times[r], flat_images[r]
    t1 = time.perf_counter()
    pool = RayPool({'rays': flat_rays, 'time': flat_times, 'target_image': flat_images}, batch_size=32768, device='cuda')
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return {'rays': pool.n_rays, 'assembly_s': t1 - t0, 'upload_s': t2 - t1, 'total_s': t2 - t0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--views', type=int, default=64)
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--no-host', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('observation_time.py needs a ROCm device')
    out = {'views': args.views, 'size': args.size, 'hbm_rate': 'measured 6.3 TB/s', 'step_ms_32768': STEP_MS_32768}
    obs = observation_set(args.views, args.size, 1)
    pool, out['single_channel'] = device_build(obs, args.repeats)
    del pool
    if not args.no_host:
        out['host_route_single_channel'] = host = host_route(obs)
        out['host_over_device'] = host['total_s'] * 1e3 / out['single_channel']['ms_per_build']
    del obs
    torch.cuda.empty_cache()
    obs = observation_set(args.views, args.size, 7)
    pool, out['seven_channels'] = device_build(obs, args.repeats)
    print(json.dumps({'observation_time': out}))


if __name__ == '__main__':
    main()
