"""CPU-only: the float64 restatement of the training update (tests/update_reference.py) against torch's own operations in float64
(ImageAsinhScaling + MSELoss, clip_grad_norm_, torch.optim.Adam), and its per-thread term count against a walk of the kernel's
visiting order -- so that the GPU comparisons in tests/test_gpu_update_f64.py measure the kernels, not the reference."""
import math

import numpy as np
import pytest
import torch

import update_reference as ur


def _sweep_counts(n, threads, aligned):
    """Terms per thread of csrc/train_step.hip's sweep(): 16-byte vectors i -> thread i % threads, then the tail elements."""
    if not aligned:
        return np.bincount(np.arange(n) % threads, minlength=threads)
    n4 = n // 4
    counts = 4 * np.bincount(np.arange(n4) % threads, minlength=threads)
    return counts + np.bincount((np.arange(4 * n4, n) - 4 * n4) % threads, minlength=threads)


@pytest.mark.parametrize('n', [1, 3, 4, 5, 255, 257, 1023, 32767, 32768, 32769, 131071, 131073, 262147, 1048577])
def test_terms_per_thread_covers_both_sweep_paths(n):
    threads = ur.reduction_threads(n)
    most = max(_sweep_counts(n, threads, True).max(), _sweep_counts(n, threads, False).max())
    assert most <= ur.terms_per_thread(n, threads) <= most + 4
    assert ur.reduction_threads(n) == 256 * min(128, max(1, -(-n // 256)))


@pytest.mark.parametrize('scaling', [(1.0, 0.005), (2.0, 0.01), None])
def test_loss64_is_the_reference_loss(scaling):
    from sunerf.train.scaling import ImageAsinhScaling
    gen = torch.Generator().manual_seed(1)
    coarse, fine, target = (torch.rand(300, 1, generator=gen) * 3 - 1 for _ in range(3))
    reg = torch.rand(300, 7, generator=gen)
    got = ur.loss64(coarse, fine, target, reg, 0.7, 2.5, scaling)
    c, f = coarse.double().requires_grad_(True), fine.double().requires_grad_(True)
    if scaling is None:
        def s(x):
            return x
    else:
        mod = ImageAsinhScaling(vmax=scaling[0], a=scaling[1]).double()

        def s(x):
            return mod(x)
    mse = torch.nn.MSELoss()
    lc, lf = mse(s(c), s(target.double())), mse(s(f), s(target.double()))
    loss = ur.f32(0.7) * (lc + lf) + ur.f32(2.5) * reg.double().mean()
    loss.backward()
    # ImageAsinhScaling keeps asinh(1 / a) of the fp64 a; the kernel (and loss64) of the fp32 a: relative 1e-9 apart
    for key, want in (('loss', loss), ('coarse', lc), ('fine', lf), ('psnr', -10 * torch.log10(lf))):
        assert abs(got[key] - want.item()) <= 1e-8 * abs(want.item()), key
    assert abs(got['regularization'] - reg.double().mean().item()) <= 1e-15
    for key, want in (('g_coarse', c.grad), ('g_fine', f.grad)):
        assert torch.allclose(got[key], want.reshape(-1), rtol=1e-8, atol=0), key
    assert ur.loss64(fine, fine, fine, None, 1.0, 1.0, scaling)['psnr'] == math.inf


@pytest.mark.parametrize('max_norm', [0.0, 1e3, 0.5])
def test_clip64_and_adam64_are_torch_clip_grad_norm_and_adam(max_norm):
    gen = torch.Generator().manual_seed(2)
    n, step = 1000, 3
    p0, g, m0 = (torch.randn(n, generator=gen) for _ in range(3))
    v0 = torch.rand(n, generator=gen)
    total, coef = ur.clip64(g, 1.0, max_norm)
    grads = g.double().clone()
    want_total = torch.nn.utils.clip_grad_norm_([torch.nn.Parameter(torch.zeros(n, dtype=torch.float64))], 1.0)  # (no grad: 0)
    assert want_total.item() == 0.0
    p = torch.nn.Parameter(p0.double().clone())
    p.grad = grads
    if max_norm > 0:
        want_total = torch.nn.utils.clip_grad_norm_([p], max_norm)
        assert abs(total - want_total.item()) <= 1e-12 * total
        assert torch.allclose(p.grad, g.double() * coef, rtol=1e-12, atol=0)
    else:
        assert coef == 1.0
    opt = torch.optim.Adam([p], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, foreach=False)
    opt.state[p] = {'step': torch.tensor(float(step - 1), dtype=torch.float64), 'exp_avg': m0.double().clone(),
                    'exp_avg_sq': v0.double().clone()}
    opt.step()
    ref = ur.adam64(p0, g, m0, v0, step, 1e-3, (0.9, 0.999), 1e-8, 1.0, coef)
    # torch's float64 Adam keeps its constants in float64, the kernel (and adam64) rounds them to fp32: ~1e-8 apart
    # (relative to the terms: m = m0 + 0.1 (g - m0) may cancel)
    scale_m = m0.double().abs() + ref['g'].abs()
    assert bool(((ref['m'] - opt.state[p]['exp_avg']).abs() <= 1e-7 * scale_m).all())
    assert torch.allclose(ref['v'], opt.state[p]['exp_avg_sq'], rtol=1e-7, atol=0)
    err = (ref['dp'] - (p.detach() - p0.double())).abs()
    assert bool((err <= 1e-6 * ref['dp'].abs() + 1e-7 * ref['step_size'] * scale_m / ref['denom']).all())
