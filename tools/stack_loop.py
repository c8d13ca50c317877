"""From raw white-light frames to a K-corona (sunerf_hip.stack.background): a sequence of coronagraph frames whose
K-corona moves from frame to frame over a static background, observed through an instrument with cosmic-ray hits, the background
estimated as a low percentile of the sequence and subtracted, and the recovered K-corona scored against the truth.

The scene is analytic.  The K-corona is three streamers, Gaussian in position angle and falling as ``r^-2.5``, that turn by
``--turn`` degrees over the sequence (the rotation of the Sun under a fixed coronagraph) over a faint ``r^-3`` hole-free floor that
turns with them; the static part is an F-corona ``r^-2.2``, flattened towards the ecliptic, plus uniform stray light, ``--ratio``
times the streamers' brightness at the inner edge.  Every frame is ``Instrument.noise`` of the sum (Poisson noise of ``--exposure``
photons per image unit, read noise of 3 DN) with ``add_cosmic_rays`` on top.  Pixels under the occulter (``r < 2``) are left out of
every score.

Per percentile ``q`` of ``--q``: ``image_metrics`` of ``frames - background(frames, q)`` against the true K-corona, mean over the
frames, next to the frames themselves (nothing subtracted) and to the K-corona less its own per-pixel minimum over the sequence --
the part of it that no statistic of the sequence can tell from the static background.  One JSON line.

    python tools/stack_loop.py [--frames 32] [--size 256] [--turn 180] [--ratio 5] [--exposure 100] [--q 0,2,5,10,25] [--cosmic-rays 0.01,20]
"""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, '2024-hl-spi3s-sunerf_amd'), os.path.join(ROOT, 'tools')]


def scene(n_frames, size, turn_deg, ratio, device):
    """``(k, static, outside)``: the K-corona [T, size, size], the static part [size, size] and the pixels outside the occulter,
    in image units where the brightest streamer is about 100 at the occulter's edge."""
    half = 10.0          # solar radii from the centre to the edge of the frame
    axis = (torch.arange(size, dtype=torch.float64, device=device) + 0.5) / size * 2.0 * half - half
    y, x = torch.meshgrid(axis, axis, indexing='ij')
    r = torch.hypot(x, y).clamp(min=1.0)
    angle = torch.atan2(y, x)
    outside = r >= 2.0
    edge = 2.0
    k = []
    for t in range(n_frames):
        phase = math.radians(turn_deg) * t / max(n_frames - 1, 1)
        frame = 3.0 * (r / edge) ** -3.0
        for centre, width, amp in ((0.3, 0.12, 100.0), (2.4, 0.2, 70.0), (-1.9, 0.08, 85.0)):
            d = torch.remainder(angle - centre - phase + math.pi, 2.0 * math.pi) - math.pi
            frame = frame + amp * torch.exp(-0.5 * (d / width) ** 2) * (r / edge) ** -2.5
        k.append(frame)
    static = ratio * 100.0 * (r / edge) ** -2.2 * (1.0 - 0.3 * torch.sin(angle) ** 2) + 0.05 * ratio * 100.0
    return torch.stack(k).float(), static.float(), outside


def scores(estimate, truth, outside, data_range):
    """Mean over the frames of image_metrics, the pixels under the occulter set to the truth in both."""
    from sunerf_hip.metrics import image_metrics
    estimate = torch.where(outside, estimate, truth).contiguous()
    m = image_metrics(estimate, truth.contiguous(), data_range)
    return {k: float(m[k].mean()) for k in ('ssim', 'psnr', 'mae', 'me')}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=32)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--turn', type=float, default=180.0, help='degrees the K-corona turns over the sequence')
    ap.add_argument('--ratio', type=float, default=5.0, help='static background over the streamers at the inner edge')
    ap.add_argument('--exposure', type=float, default=100.0, help='photons per image unit: the streamers peak near 100 image units')
    ap.add_argument('--q', default='0,2,5,10,25', help='percentiles of background() to try')
    ap.add_argument('--cosmic-rays', metavar='RATE,AMP', default='0.01,20', help='fraction of pixels hit per frame and the amplitude in sigma')
    ap.add_argument('--seed', type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('stack_loop.py needs a ROCm device')
    from sunerf_hip.despike import add_cosmic_rays
    from sunerf_hip.instrument import Instrument
    from sunerf_hip.stack import background
    dev = torch.device('cuda')
    k, static, outside = scene(args.frames, args.size, args.turn, args.ratio, dev)
    inst = Instrument(unit=1.0, exposure=args.exposure, dn_per_photon=1.0, read_noise=3.0)
    frames, sigma, _ = inst.noise(k + static[None], args.seed)
    rate, amp = (float(v) for v in args.cosmic_rays.split(','))
    hits = 0
    if rate > 0:
        frames, truth_hits = add_cosmic_rays(frames, rate, amp, sigma=sigma, seed=args.seed + 1)
        hits = int(truth_hits.sum())
    data_range = float(k[:, outside].max())
    out = {'frames': args.frames, 'size': args.size, 'turn_deg': args.turn, 'ratio': args.ratio, 'exposure': args.exposure, 'hits': hits, 'data_range': data_range,
           'nothing_subtracted': scores(frames, k, outside, data_range),
           'truth_less_its_own_minimum': scores(k - k.min(dim=0).values[None], k, outside, data_range), 'background': {}}
    for q in (float(v) for v in args.q.split(',')):
        bg = background(frames, q=q)
        row = scores(frames - bg['image'][0][None], k, outside, data_range)
        row['background_mae_against_static'] = float((bg['image'][0] - static)[outside].abs().mean())
        out['background'][f'{q:g}'] = row
    print(json.dumps({'stack_loop': out}))


if __name__ == '__main__':
    main()
