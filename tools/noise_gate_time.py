"""Cost of noise gating (csrc/noise_gate.hip, sunerf_hip.noise_gate) at 16 x 1 x 2048^2 for blocks of 1, 8 and 16
frames, next to

* the kernel's own HBM byte model: every pass reads the sequence once and reads and writes ``out`` (the first pass only writes),
  ``12 passes - 4`` bytes per sample -- 188 at 16 passes, 764 at 64 -- at ``--hbm-tbs`` (8 TB/s is the MI355X's peak).  The model
  ignores the folded samples read twice at the edges and every cache: two passes touch the same 0.5 GB;
* the same rule through ``torch.fft`` on the same device.  The 64-fold overlapping blocks unfolded at once would be a complex
  tensor of about 34 GB, so the formulation is chunked by pass: the blocks of one pass tile the padded sequence, which is viewed
  as ``[nt, bt, ny, 16, nx, 16]``, windowed, transformed with ``rfftn`` over the three block axes, gated, transformed back and
  added to the result -- 64 (16) chunks of one half spectrum each.  It handles no invalid samples.  Its result is compared with
  the kernel's (``max_diff``).

Per row: the CUDA-event time per call over ``--repeats`` windows of ``--calls`` back-to-back calls after a warm-up -- median,
fastest and slowest window.  One JSON line.

    python tools/noise_gate_time.py [--repeats 5] [--calls 2] [--size 2048] [--frames 16] [--hbm-tbs 8.0]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, '2024-hl-spi3s-sunerf_amd'), os.path.join(ROOT, 'tools')]

from coalign_time import timed  # noqa: E402

A, B, GAMMA = 1.0, 0.5, 3.0


def window(n, device):
    return torch.ones(1, device=device) if n == 1 else torch.sin(torch.pi * (torch.arange(n, device=device) + 0.5) / n) ** 2


def fold(i, n):
    m = torch.remainder(i, 2 * n)
    return torch.where(m < n, m, 2 * n - 1 - m)


def torch_gate(frames, bt):
    """``frames`` [T, H, W] without invalid samples: mode 'gate' of the header, pass by pass."""
    dev = frames.device
    sizes, blocks = frames.shape, (bt, 16, 16)
    w = window(bt, dev).view(1, bt, 1, 1, 1, 1) * window(16, dev).view(1, 1, 1, 16, 1, 1) * window(16, dev).view(1, 1, 1, 1, 1, 16)
    norm = 1.5 ** (3 if bt > 1 else 2)
    out = torch.zeros_like(frames)
    passes = [range(4) if n > 1 else range(1) for n in blocks]
    for pt in passes[0]:
        for py in passes[1]:
            for px in passes[2]:
                index, inside, count = [], [], []
                for p, n, size in zip((pt, py, px), blocks, sizes):
                    s = max(n // 4, 1)
                    o = p * s - (n - s)
                    nb = (size - o + n - 1) // n
                    pos = torch.arange(o, o + nb * n, device=dev)
                    index.append(fold(pos, size))
                    inside.append((max(o, 0) - o, min(size, o + nb * n) - o, max(o, 0)))
                    count.append(nb)
                vol = frames[index[0]][:, index[1]][:, :, index[2]].view(count[0], bt, count[1], 16, count[2], 16)
                spec = torch.fft.rfftn(vol * w, dim=(1, 3, 5))
                power = (w * w * (A + B * vol.clamp(min=0))).sum(dim=(1, 3, 5), keepdim=True)
                keep = (spec.real ** 2 + spec.imag ** 2 >= (GAMMA * GAMMA) * power)
                keep[:, 0, :, 0, :, 0] = True
                part = (torch.fft.irfftn(spec * keep, s=blocks, dim=(1, 3, 5)) * w / norm).reshape(count[0] * bt, count[1] * 16, count[2] * 16)
                (t0, t1, a0), (y0, y1, b0), (x0, x1, c0) = inside
                out[a0:a0 + t1 - t0, b0:b0 + y1 - y0, c0:c0 + x1 - x0] += part[t0:t1, y0:y1, x0:x1]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--calls', type=int, default=2)
    ap.add_argument('--size', type=int, default=2048)
    ap.add_argument('--frames', type=int, default=16)
    ap.add_argument('--hbm-tbs', type=float, default=8.0)
    ap.add_argument('--no-torch', action='store_true')
    args = ap.parse_args()
    from sunerf_hip.noise_gate import launch
    g = torch.Generator(device='cuda').manual_seed(1)
    y, x = torch.meshgrid(torch.arange(args.size, device='cuda'), torch.arange(args.size, device='cuda'), indexing='ij')
    truth = 4.0 + 3.0 * torch.sin(0.05 * x + 0.03 * y)[None] * torch.cos(0.2 * torch.arange(args.frames, device='cuda'))[:, None, None]
    frames = (truth + (A + B * truth).sqrt() * torch.randn(truth.shape, device='cuda', generator=g))[:, None].contiguous()
    params = torch.tensor([[A, B, 0.0, 0.0]], dtype=torch.float64, device='cuda')
    samples = frames.numel()
    rows = []
    for bt in (1, 8, 16):
        if bt > args.frames:
            continue
        passes = 64 if bt > 1 else 16
        ms = timed(lambda: launch(frames, None, params, None, bt, 0, 0, GAMMA), args.repeats, args.calls)
        out, state = launch(frames, None, params, None, bt, 0, 0, GAMMA)
        model_bytes = (12 * passes - 4) * samples
        row = {'block_t': bt, 'passes': passes, 'ms': [round(v, 3) for v in ms], 'model_bytes_per_sample': 12 * passes - 4,
               'floor_ms': round(model_bytes / (args.hbm_tbs * 1e9), 3), 'achieved_model_tbs': round(model_bytes / (ms[0] * 1e9), 3),
               'gsamples_per_s': round(samples / (ms[0] * 1e6), 3), 'kept_fraction': round(float(state[0, 2]) / float(state[0, 3]), 5)}
        if not args.no_torch:
            ref = torch_gate(frames[:, 0], bt)
            row['max_diff'] = float((ref - out[:, 0]).abs().max())
            row['torch_fft_chunked_ms'] = [round(v, 1) for v in timed(lambda: torch_gate(frames[:, 0], bt), max(args.repeats // 2, 1), 1)]
            del ref
        rows.append(row)
    print(json.dumps({'shape': [args.frames, 1, args.size, args.size], 'hbm_tbs': args.hbm_tbs, 'rows': rows}))


if __name__ == '__main__':
    main()
