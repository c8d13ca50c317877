#!/usr/bin/env python3
"""The any-size fp32 backward (SUNERF_BACKWARD_PRECISION=exact, csrc/bwd_exact.hip: sunerf_mlp_backward_exact_chunked) against the
default backward on the same batch: ms per emission backward call (integral backward included, HIP events), and the fp32 matrix
rate of the exact one from its GEMM operation count.  ``--small-kernel``: the small-batch fp32 kernel too (its limit raised).
usage: exact_any_batch_time.py [--small-kernel] [n_rays n_samples] ...   (default: 3072 256  8192 128  32768 128; 9 x 256 network)"""
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


def gemm_flop_per_sample(D, n_linear, d_out=2, d_in=84):
    """forward (n_linear - 1 layers), data gradients (n_linear - 1), weight gradients (n_linear): 2 flop per multiply-add."""
    fwd = d_in * D + (n_linear - 2) * D * D
    dgrad = d_out * D + (n_linear - 2) * D * D
    wgrad = d_out * D + (n_linear - 2) * D * D + D * d_in
    return 2 * (fwd + dgrad + wgrad)


def run(n_rays, S, small_kernel):
    params = orc.init_params(d_filter=D, n_layers=N_LAYERS, seed=3)
    o, d = orc.synthetic_rays(int(math.ceil(n_rays ** 0.5)))
    o, d = o[:n_rays].to(dev), d[:n_rays].to(dev)
    t = torch.rand(n_rays, 1, device=dev)
    z = orc.stratified_z(o.cpu(), d.cpu(), orc.linspace_t_vals(S), torch.tensor(1.3), torch.tensor(1.0)).to(dev)
    Ws, bs = [W.to(dev) for W, _ in params], [b.to(dev) for _, b in params]
    packed = ops.PackedMLP(Ws, bs)
    g_image = torch.randn(n_rays, device=dev) * 1e-3
    n = n_rays * S
    reps = max(3, min(20, int(2e6 // n)))
    line = f'{n_rays} rays x {S} samples ({n}):'
    modes = [('default', {}), ('exact any-size', {'SUNERF_BACKWARD_PRECISION': 'exact'})]
    if small_kernel:
        modes.append(('exact small-batch kernel', {'SUNERF_EXACT_BACKWARD_SAMPLES': str(n)}))
    for name, env in modes:
        for k in ('SUNERF_BACKWARD_PRECISION', 'SUNERF_EXACT_BACKWARD_SAMPLES'):
            os.environ.pop(k, None)
        os.environ.update(env)
        fwd = ops.emission_render_fwd(packed, o, d, t, z, reg_radius=1.2, training=True)
        gW, gb = [torch.empty_like(W) for W in Ws], [torch.empty_like(b) for b in bs]
        call = lambda: ops.emission_render_bwd(packed, o, d, z, fwd['raw'], fwd['stash'], g_image, None, 2e-5, 1.2, gW, gb, times=t)
        for _ in range(2):
            call()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(reps):
            call()
        ev[1].record()
        torch.cuda.synchronize()
        ms = ev[0].elapsed_time(ev[1]) / reps
        line += f'  {name} {ms:.2f} ms'
        if name.startswith('exact'):
            line += f' ({gemm_flop_per_sample(D, N_LAYERS + 1) * n / ms / 1e9:.1f} TF/s of GEMM)'
        del fwd
        torch.cuda.empty_cache()
    print(line, flush=True)


if __name__ == '__main__':
    args = sys.argv[1:]
    small = '--small-kernel' in args
    a = [int(v) for v in args if v != '--small-kernel']
    for n_rays, S in ([tuple(a[i:i + 2]) for i in range(0, len(a), 2)] or [(3072, 256), (8192, 128), (32768, 128)]):
        run(n_rays, S, small)
