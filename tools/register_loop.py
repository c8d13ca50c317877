"""What registration is for: a scene painted on the solar surface turns under the differential law in front of one
observer, 16 frames of 96 x 96 one hour apart under shot noise: the smooth function of the host test's closed scene plus fine
structure with a wavelength of 6 to 7 pixels at disk centre.  ``noise_gate`` (blocks of 8 frames) and ``combine(method='median')``
are run on the raw sequence and on the sequence derotated onto its middle frame; reported is the RMS error against the noiseless
middle frame on the disk away from the limb (m / radius^2 > 0.3).  On the raw sequence a feature at disk centre moves 5 pixels
in the 15 hours, so the median smears it and the gate sees motion it has to keep; on the registered one only the noise changes
from frame to frame.  One JSON line.

    python tools/register_loop.py [--frames 16] [--size 96] [--hours 1.0]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, '2024-hl-spi3s-sunerf_amd'), os.path.join(ROOT, 'tests')]

LEVEL, B = 100.0, 1.0          # image units of the painted scene, variance per unit
FINE = 0.6                     # amplitude of the fine structure (a wavelength of 6 to 7 pixels at disk centre on 96 x 96)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=16)
    ap.add_argument('--size', type=int, default=96)
    ap.add_argument('--hours', type=float, default=1.0)
    args = ap.parse_args()
    import register_reference as rr
    from sunerf_hip.noise_gate import noise_gate
    from sunerf_hip.register import derotate
    from sunerf_hip.reprojection import Observer
    from sunerf_hip.stack import combine
    t, n = args.frames, args.size
    rates = tuple(86400.0 * v for v in rr.SIDEREAL)          # per day, the observer fixed in the sidereal frame
    tx, ty = rr.axes_for((n, n), 1.25 * rr.DISK)
    c2w = rr.look_at_pose(0.05, 0.1, rr.AU)
    lat, lon, mrel, on_disk = rr.surface(c2w, tx, ty)
    sl2 = np.sin(lat) ** 2
    rate = (rates[0] + rates[1] * sl2) + rates[2] * sl2 * sl2
    times = (np.arange(t) - t // 2) * args.hours / 24.0
    scene = lambda b, l: 1.0 + rr.painted(b, l) + FINE * np.sin(36.0 * l) * np.cos(24.0 * b)          # noqa: E731
    clean = np.stack([LEVEL * scene(lat, lon - rate * dt) for dt in times])
    rng = np.random.default_rng(1)
    noisy = (clean + np.sqrt(B * clean) * rng.standard_normal(clean.shape)).astype(np.float32)
    truth, inner = clean[t // 2], mrel > 0.3
    rms = lambda img: float(np.sqrt(np.mean((np.asarray(img, dtype=np.float64) - truth)[inner] ** 2)))          # noqa: E731
    observer = Observer(0.0, 0.0, rr.AU, tx=tx, ty=ty)
    observer.c2w = torch.from_numpy(np.vstack([c2w, [[0, 0, 0, 1]]]).astype(np.float32))
    raw = torch.from_numpy(noisy).cuda()[:, None]
    reg = derotate(raw, observer, times.tolist(), reference=t // 2, rotation=rr.SIDEREAL, frame='sidereal', order=3)
    counts = reg['counts'].sum(0).tolist()
    rows = {}
    for name, seq in (('raw', raw), ('registered', reg['image'])):
        gated = noise_gate(seq, a=0.0, b=B, block_t=8)['image'][t // 2, 0].cpu().numpy()
        median = combine(seq, method='median')['image'][0].cpu().numpy()
        rows[name] = {'middle_frame': round(rms(seq[t // 2, 0].cpu().numpy()), 4), 'noise_gate': round(rms(gated), 4), 'median': round(rms(median), 4),
                      'nan_on_inner_disk': int(np.isnan(gated[inner]).sum() + np.isnan(median[inner]).sum())}
    moved = float(np.abs(rate[n // 2, n // 2] * (times[-1] - times[0])) * (n - 1) / 2.5)
    print(json.dumps({'scene': [t, 1, n, n], 'hours_between_frames': args.hours, 'pixels_moved_at_disk_centre': round(moved, 2),
                      'noise_sigma': round(float(np.sqrt(B * truth[inner]).mean()), 2), 'status_counts': counts, 'rms': rows}))


if __name__ == '__main__':
    main()
