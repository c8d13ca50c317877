#!/usr/bin/env python3
"""The input-gradient backward (csrc/bwd_exact.hip: sunerf_mlp_input_grad_exact) on an 8 x 256 network: ms per call (HIP events) for
a 256^3 volume query (16.7 M free-standing points, the size of the reference's voxel_volume.py) and a 1024 x 128 ray batch, input
gradients only (a frozen model) and with the parameter gradients alongside, and the fp32 matrix rate from the GEMM operation count.
usage: input_grad_time.py [--side 256] [--rays 1024 128]"""
import argparse
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, '2024-hl-spi3s-sunerf_amd'))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
import sunerf_oracle as orc   # noqa: E402  (initial weights / synthetic rays only)
from sunerf_hip import ops    # noqa: E402

dev = torch.device('cuda')
D, N_LAYERS = 256, 8


def gemm_flop_per_sample(D, n_linear, params, d_out=2, d_in=84):
    """forward (n_linear - 1 layers), data gradients (n_linear - 1) + the 84-column encoder gradient, weight gradients when asked
    for (n_linear): 2 flop per multiply-add."""
    fwd = d_in * D + (n_linear - 2) * D * D
    dgrad = d_out * D + (n_linear - 2) * D * D + D * d_in
    wgrad = d_out * D + (n_linear - 2) * D * D + D * d_in
    return 2 * (fwd + dgrad + (wgrad if params else 0))


def timed(call, reps):
    call()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        call()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--side', type=int, default=256)
    ap.add_argument('--rays', type=int, nargs=2, default=(1024, 128))
    a = ap.parse_args()
    params = orc.init_params(d_filter=D, n_layers=N_LAYERS, seed=3)
    Ws, bs = [W.to(dev) for W, _ in params], [b.to(dev) for _, b in params]
    packed = ops.PackedMLP(Ws, bs)
    gW, gb = [torch.empty_like(W) for W in Ws], [torch.empty_like(b) for b in bs]
    flop = {p: gemm_flop_per_sample(D, N_LAYERS + 1, p) for p in (False, True)}

    side = a.side
    axis = torch.linspace(-1.5, 1.5, side, device=dev)
    pts = torch.stack(torch.meshgrid(axis, axis, axis, indexing='ij') + (torch.zeros(side, side, side, device=dev),), -1).reshape(-1, 4)
    m = pts.shape[0]
    g = torch.randn(m, 2, device=dev)
    for p in (False, True):
        extra = (gW, gb) if p else ()
        ms = timed(lambda: ops.mlp_input_backward(packed, g, ('points', pts), *extra), 2)
        print(f'{side}^3 volume ({m} points), {"inputs + parameters" if p else "inputs only"}: {ms:.1f} ms '
              f'({flop[p] * m / ms / 1e9:.1f} TF/s of GEMM)', flush=True)
    del pts, g
    torch.cuda.empty_cache()

    n_rays, S = a.rays
    o, d = orc.synthetic_rays(int(math.ceil(n_rays ** 0.5)))
    o, d = o[:n_rays].to(dev), d[:n_rays].to(dev)
    t = torch.rand(n_rays, 1, device=dev)
    z = orc.stratified_z(o.cpu(), d.cpu(), orc.linspace_t_vals(S), torch.tensor(1.3), torch.tensor(1.0)).to(dev)
    g = torch.randn(n_rays, S, 2, device=dev)
    n = n_rays * S
    for p in (False, True):
        extra = (gW, gb) if p else ()
        ms = timed(lambda: ops.mlp_input_backward(packed, g, ('rays', o, d, t, z), *extra), 10)
        print(f'{n_rays} rays x {S} samples ({n}), {"inputs + parameters" if p else "inputs only"}: {ms:.2f} ms '
              f'({flop[p] * n / ms / 1e9:.1f} TF/s of GEMM)', flush=True)


if __name__ == '__main__':
    main()
