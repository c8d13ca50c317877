"""Cost of the noise-weighted likelihood (csrc/likelihood.hip, sunerf_hip.likelihood.likelihood_loss) next to the MSE loss it
replaces (csrc/train_step.hip, sunerf_hip.train.training_loss, untouched by the likelihood) at the training batch of the
benchmark, 32768 rays x 1 channel (emission: asinh-scaled MSE) and 32768 x 7 (density-temperature: plain MSE).

Per shape and loss: milliseconds of the forward call alone (one kernel) and of forward + ``backward()`` (the autograd node's
products included), CUDA-event median over ``--repeats`` windows of ``--calls`` back-to-back calls after a warm-up.  The
likelihood is timed in both modes; at 7 columns with every ray carrying the same seven codes (an AIA batch) and with every SLOT
drawing its own code from 64 rows (the worst case of the per-row reduction: up to 64 distinct rows in a wave).  The lower bound
is the kernel's HBM traffic (three or four fp32 reads and two fp32 writes per slot) at 6.3 TB/s (measured copy rate,
MI355X_MICROARCH).  One JSON line.

    python tools/likelihood_time.py [--repeats 7] [--calls 20]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, '2024-hl-spi3s-sunerf_amd')]

HBM_BYTES_PER_S = 6.3e12          # measured float4 copy rate


def timed(fn, repeats, calls):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(calls):
            fn()
        stop.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(stop) / calls)
    return sorted(times)[len(times) // 2], [min(times), max(times)]


def measure(n, w, repeats, calls):
    from sunerf_hip.instrument import Instrument
    from sunerf_hip.likelihood import NoiseLikelihood, likelihood_loss
    from sunerf_hip.train import training_loss
    g = torch.Generator(device='cuda').manual_seed(n + w)
    target = torch.rand(n, w, device='cuda', generator=g) + 0.05
    coarse = (target * (0.8 + 0.4 * torch.rand(n, w, device='cuda', generator=g))).requires_grad_(True)
    fine = (target * (0.9 + 0.2 * torch.rand(n, w, device='cuda', generator=g))).requires_grad_(True)
    reg = torch.rand(n, 192, device='cuda', generator=g).requires_grad_(True)
    inst = Instrument(unit=200.0, exposure=2.9, dn_per_photon=1.2, read_noise=1.2)
    scaling = (1.0, 0.005) if w == 1 else None
    rows = []

    def both(name, forward, slot_bytes):
        def step():
            for t in (coarse, fine, reg):
                t.grad = None
            forward().backward()
        with torch.no_grad():
            fwd, fwd_spread = timed(forward, repeats, calls)
        full, full_spread = timed(step, repeats, calls)
        nbytes = slot_bytes * n * w + 4 * reg.numel()
        rows.append({'shape': [n, w], 'loss': name, 'forward_ms': fwd, 'forward_spread_ms': fwd_spread, 'forward_backward_ms': full,
                     'forward_backward_spread_ms': full_spread, 'kernel_bytes': nbytes,
                     'bound_ms_hbm': nbytes / HBM_BYTES_PER_S * 1e3, 'calls_timed': repeats * calls})

    both('training_loss' + (' (asinh)' if scaling else ''),
         lambda: training_loss(coarse, fine, target, reg, asinh_scaling=scaling)[0], 20)
    variants = [('one row, no codes', NoiseLikelihood(inst, free='all'), None)] if w == 1 else []
    if w > 1:
        seven = [94, 131, 171, 193, 211, 304, 335][:w]
        variants.append((f'{w} rows, every ray the same codes', NoiseLikelihood(inst, codes=seven, free=seven[1:]),
                         torch.tensor(seven, dtype=torch.float32, device='cuda').repeat(n, 1).contiguous()))
        many = list(range(1, 65))
        table = torch.tensor(many, dtype=torch.float32, device='cuda')
        variants.append(('64 rows, every slot its own code', NoiseLikelihood(inst, codes=many, free=many),
                         table[torch.randint(0, 64, (n, w), device='cuda', generator=g)].contiguous()))
    for label, like, codes in variants:
        like = like.cuda()
        for mode in ('observed', 'model'):
            like.mode = mode
            both(f'likelihood_loss {mode}: {label}', lambda: likelihood_loss(coarse, fine, target, reg, like, codes=codes)[0],
                 20 if codes is None else 24)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--calls', type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('likelihood_time.py needs a ROCm device')
    rows = [r for n, w in ((32768, 1), (32768, 7)) for r in measure(n, w, args.repeats, args.calls)]
    for r in rows:
        print(f"{r['shape'][0]} x {r['shape'][1]}  {r['loss']:<62s} forward {r['forward_ms'] * 1e3:7.1f} us   forward + backward "
              f"{r['forward_backward_ms'] * 1e3:7.1f} us   (HBM bound {r['bound_ms_hbm'] * 1e3:.1f} us)", file=sys.stderr)
    print(json.dumps({'likelihood_time': rows, 'hbm_rate': 'measured 6.3 TB/s'}))


if __name__ == '__main__':
    main()
