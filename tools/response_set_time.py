"""Times the response-set kernels (csrc/dt_response_set.hip) next to the AIA kernels (csrc/dt.hip) on the same inputs:

  - the seven AIA rows as a ResponseSet against sunerf_dt_integral_fwd / _bwd, W = 7, at BASELINE config 5's integral shape
    (8192 rays x 256 samples) and at the fine pass of tools/simple_star_step.py (32768 rays x 192 samples);
  - an 11-channel set (the AIA rows and four synthetic channels of 2, 3, 37 and 256 nodes) at W = 8, which dt.hip cannot run.

The two are launched alternately, each call between two device events; the table gives the median of ``reps`` calls after
``warmup`` untimed ones, and the ratio new / old.  Outputs are compared first (image, weights, g_raw by bits on the AIA set).
Usage:  python tools/response_set_time.py [reps]"""
import os
import sys

import numpy as np
import torch

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(R, '2024-hl-spi3s-sunerf_amd'))
from sunerf_hip import ops                                                        # noqa: E402
from sunerf_hip.response import ResponseSet                                       # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
warmup = 5
g6 = np.load(os.path.join(R, 'tests', 'golden', 'g6_dt_e2e.npz'))
logte = torch.from_numpy(g6['aia_logte']).float()
resp = torch.from_numpy(g6['aia_tresp'] * 2.9).float()
aia = ResponseSet.aia((g6['aia_logte'], g6['aia_tresp']), exposure=2.9)


def bump(x, centre, width, height):
    return height * np.exp(-((x - centre) / width) ** 2) + 0.02 * height


steps = np.array([0.01 + 0.019 * ((7 * i) % 11) for i in range(36)])
x37 = 4.5 + np.concatenate([[0.], np.cumsum(steps)])
x256 = np.linspace(6.25, 8.8, 256)
eleven = aia.concat(ResponseSet([(174, 'two nodes', [5.5, 7.0], bump(np.array([5.5, 7.0]), 6.0, 0.6, 3e-25)),
                                 (10171, 'three nodes', [5.0, 6.1, 7.3], bump(np.array([5.0, 6.1, 7.3]), 5.95, 0.5, 2e-25)),
                                 (10195, '37 nodes', x37, bump(x37, 6.2, 0.35, 4e-25)),
                                 (20001, '256 nodes', x256, bump(x256, 7.0, 0.3, 1e-25))]))


def inputs(n, s, codes, w, seed=0):
    """NeRF_DT-like inputs: ln rho around 10, log T over 5.5 ... 7.5, optical depths of order 0.1."""
    gen = torch.Generator().manual_seed(seed)
    raw = torch.stack([0.3 * torch.randn(n, s, generator=gen), 0.5 + 2.0 * torch.rand(n, s, generator=gen)], -1)
    z = 213.7 + 2.6 * torch.sort(torch.rand(n, s, generator=gen), -1).values
    o = torch.randn(n, 3, generator=gen)
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=gen), dim=-1)
    table = torch.tensor(codes, dtype=torch.float32)
    wl = table[torch.argsort(torch.rand(n, len(codes), generator=gen), -1)[:, :w]].contiguous()
    la = 2e-6 * (0.5 + torch.rand(len(codes), generator=gen))
    g_image = 0.25 + torch.rand(n, w, generator=gen)
    return [t.cuda() for t in (raw, z, o, d, wl)], la.cuda(), torch.tensor([1.0]).cuda(), g_image.cuda()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3      # microseconds


def alternate(calls):
    """{name: median microseconds} of ``calls`` = {name: callable}, launched in turn."""
    for _ in range(warmup):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            times[k].append(timed(fn))
    return {k: float(np.median(v)) for k, v in times.items()}


tail = (10.0, 5.0, 1e17, 1.25)
print(f'{reps} calls each after {warmup} warm-up calls, launched alternately; median microseconds per call '
      f'(wrapper included: output allocation, the clear of the scalar gradients)')
print(f'{"shape":>24s} {"set":>10s} {"pass":>5s} {"dt.hip":>10s} {"response":>10s} {"ratio":>7s}')
for n, s in ((8192, 256), (32768, 192)):
    (raw, z, o, d, wl), la, vc, g_image = inputs(n, s, aia.codes, 7)
    old = (raw, z, o, d, wl, logte.cuda(), resp.cuda(), la, vc) + tail
    new = (raw, z, o, d, wl, aia, la, vc) + tail
    f_old, f_new = ops.dt_integral_fwd(*old, want_epilogues=True), ops.dt_response_fwd(*new, want_epilogues=True)
    b_old, b_new = ops.dt_integral_bwd(*old, g_image, None), ops.dt_response_bwd(*new, g_image, None)
    torch.cuda.synchronize()
    assert all(torch.equal(f_old[k], f_new[k]) for k in f_old) and torch.equal(b_old[0], b_new[0]), 'outputs differ'
    t = alternate({'fwd_old': lambda: ops.dt_integral_fwd(*old, want_epilogues=True),
                   'fwd_new': lambda: ops.dt_response_fwd(*new, want_epilogues=True),
                   'bwd_old': lambda: ops.dt_integral_bwd(*old, g_image, None),
                   'bwd_new': lambda: ops.dt_response_bwd(*new, g_image, None)})
    for p in ('fwd', 'bwd'):
        print(f'{f"{n} x {s} x 7":>24s} {"AIA (7)":>10s} {p:>5s} {t[p + "_old"]:10.1f} {t[p + "_new"]:10.1f} '
              f'{t[p + "_new"] / t[p + "_old"]:7.3f}')
    (raw, z, o, d, wl), la, vc, g_image = inputs(n, s, eleven.codes, 8, seed=1)
    new = (raw, z, o, d, wl, eleven, la, vc) + tail
    if not eleven.fits(s, 8):
        print(f'{f"{n} x {s} x 8":>24s} {"11 chan.":>10s}   the backward needs {eleven.bwd_lds_bytes(s, 8)} B of LDS: not run')
        continue
    t = alternate({'fwd_new': lambda: ops.dt_response_fwd(*new, want_epilogues=True),
                   'bwd_new': lambda: ops.dt_response_bwd(*new, g_image, None)})
    for p in ('fwd', 'bwd'):
        print(f'{f"{n} x {s} x 8":>24s} {"11 chan.":>10s} {p:>5s} {"-":>10s} {t[p + "_new"]:10.1f} {"-":>7s}')
