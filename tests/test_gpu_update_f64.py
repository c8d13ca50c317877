"""The training update (csrc/train_step.hip through sunerf_hip.train) against a float64 restatement of the same operations on the
same fp32 inputs (tests/update_reference.py): the loss, the gradient norm and clip, and Adam, at sizes on both sides of every
launch-shape seam (one vector, one workgroup, the 128-workgroup reduction grid, the 4096-workgroup Adam grid and its grid-stride
loop, the d512 parameter count), with the regularisation and finite-check tensors aligned and at storage offsets of 1, 2 and 3
floats (sweep()'s scalar path), and with values from subnormals to 1e6 in one tensor.

Every bound comes from the kernel's summation structure (update_reference.py), not from the measurements.  Worst ratio
error / bound measured on an MI355X (<= 1 passes):
    loss 0.21, coarse MSE 0.29, fine MSE 0.19, regularisation mean 0.097, PSNR 0.42, d loss / d image 0.46;
    norm 0.21, clip coefficient 0.38, written-back gradient 0.36, m 0.92, v 0.99, Delta p 0.50.
m and v come close to their bounds because every rounding of their few operations can reach U and millions of elements are
checked; Delta p sits at 0.5 because where the update is below half an ulp of p, the write-back rounds it away.
"""
import math

import pytest
import torch

import update_reference as ur

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 5, 255, 257, 32767, 32768, 32769, 131071, 131073, 262147, 1048575, 1048576, 1048577, 3766276]
GRAD_SCALES = (1.0, 0.5, 1.0 / 3.0, 0.125)
D512_PARAMS = 3766276           # coarse + fine NeRF(d_filter=512), counted from sunerf.model.model.NeRF


@pytest.fixture(scope='module')
def train():
    from sunerf_hip import train as t
    return t


def mixed(n, gen, signed=True, lo=-20.0, hi=6.0):
    """fp32 values with magnitudes log-uniform in [10^lo, 10^hi], random signs, every 7th a zero (from index 6), every 11th a
    subnormal (from index 3)."""
    x = torch.pow(10.0, torch.rand(n, generator=gen, dtype=torch.float64) * (hi - lo) + lo)
    if signed:
        x = x * (torch.randint(0, 2, (n,), generator=gen) * 2 - 1)
    x = x.float()
    x[6::7] = 0.0
    x[3::11] = torch.rand(x[3::11].shape, generator=gen) * 1e-39           # subnormal: below 2^-126 ~ 1.18e-38
    return x


def placed(x, offset):
    """``x`` on the device as a contiguous view at a storage offset of ``offset`` floats: offsets 1, 2, 3 are not 16-byte
    aligned and take sweep()'s scalar path, 0 (a fresh allocation) the 16-byte path."""
    buf = torch.full((x.numel() + offset,), float('nan'), device='cuda')
    view = buf[offset:].view(x.shape)
    view.copy_(x)
    assert view.is_contiguous() and (view.data_ptr() % 16 == 0) == (offset % 4 == 0)
    return view


def _check(name, got, ref, bound, worst):
    """|got - ref| <= bound elementwise (float64); records the worst ratio."""
    got = torch.as_tensor(got).detach().cpu().double().reshape(-1)
    ref = torch.as_tensor(ref, dtype=torch.float64).reshape(-1)
    bound = torch.as_tensor(bound, dtype=torch.float64).reshape(-1).expand_as(ref)
    assert bool(torch.isfinite(got).all()), name
    ratio = ((got - ref).abs() / bound.clamp_min(1e-300)).max().item()
    worst[name] = max(worst.get(name, 0.0), ratio)
    assert ratio <= 1.0, (name, ratio)


def _report(title, worst):
    print(f'\n{title}: worst error / bound ' + ', '.join(f'{k} {v:.3g}' for k, v in sorted(worst.items())))


def _loss_cases(n, gen):
    """(scaling, lambda_image, lambda_regularization, n_reg, finite-check sizes, offset, fine equals target) per case."""
    odd = min(96 * n, 4_000_000) | 1
    return [((1.0, 0.005), 1.0, 1.0, 0, [], 0, False),
            ((1.0, 0.005), 0.7, 2.5, 1, [n], 1, False),
            (None, 1.5, 0.3, odd, [n + 1] + [j * 37 + 1 for j in range(7)], 2, False),
            ((2.0, 0.01), 1.0, 1.0, odd, [odd], 3, True),
            ((1.0, 0.005), 3.0, 0.5, odd, [1], 0, False)]


@pytest.mark.parametrize('n', SIZES)
def test_training_loss_vs_float64(train, n):
    gen = torch.Generator().manual_seed(1000 + n)
    worst = {}
    for scaling, li, lr, n_reg, extra_sizes, offset, equal in _loss_cases(n, gen):
        target = mixed(n, gen).reshape(-1, 1)
        coarse = target.clone() if equal else mixed(n, gen).reshape(-1, 1)
        fine = target.clone() if equal else mixed(n, gen).reshape(-1, 1)
        reg = mixed(n_reg, gen, signed=True, lo=-8.0, hi=2.0) if n_reg else None
        extras = []
        for j, m in enumerate(extra_sizes):
            e = torch.rand(m, generator=gen)
            if j % 2 == 0:
                e[(j * 13) % m] = float('nan') if j % 4 == 0 else float('inf')
            extras.append(placed(e, offset))
        c = coarse.cuda().requires_grad_(True)
        f = fine.cuda().requires_grad_(True)
        r = placed(reg, offset) if reg is not None else None
        loss, stats = train.training_loss(c, f, target.cuda(), r, li, lr, asinh_scaling=scaling, finite_check=extras)
        loss.backward()
        s = stats.cpu().double()
        ref = ur.loss64(coarse, fine, target, reg, li, lr, scaling, finite_check=extras)
        most = max([n, n_reg] + extra_sizes)
        b = ur.loss_bounds(ref, ur.reduction_threads(most))
        assert s[5].item() == ref['non_finite'] and s[6].item() == 0 and s[7].item() == 0
        for i, key in enumerate(('loss', 'coarse', 'fine', 'regularization')):
            _check(key, s[i], ref[key], b[key], worst)
        assert equal == (ref['fine'] == 0)
        if equal:
            assert s[2].item() == 0 and s[4].item() == math.inf           # MSE 0 -> PSNR +inf, as torch gives it
        else:
            _check('psnr', s[4], ref['psnr'], b['psnr'], worst)
        _check('d loss / d image', c.grad, ref['g_coarse'], b['g_coarse'], worst)
        _check('d loss / d image', f.grad, ref['g_fine'], b['g_fine'], worst)
    _report(f'loss n={n}', worst)


def _fill_grads(bucket_view, gen):
    g = mixed(bucket_view.numel(), gen, lo=-20.0, hi=6.0)
    bucket_view.copy_(g)
    return g


def _adam_step_vs_float64(train, opt, p_before, gen, max_norm_for, worst, skip=False, expected_step=None):
    """One ClipAdam.step on fresh mixed gradients, checked element by element against clip64 + adam64 from the fp32 state
    before the step.  ``max_norm_for(total64)`` picks the clip threshold."""
    g32 = _fill_grads(opt.flat_grads, gen)
    m0, v0 = opt.exp_avg.cpu().clone(), opt.exp_avg_sq.cpu().clone()
    total, _ = ur.clip64(g32, 1.0, 0.0)
    max_norm = max_norm_for(total)
    opt.max_norm = max_norm
    flag = torch.tensor([1.0 if skip else 0.0], device='cuda')
    opt.step(skip_if_positive=flag)
    norm = opt.norm.cpu().double()
    p_after = opt.flat_params.cpu()
    if skip:
        assert norm[2].item() == 1.0
        assert torch.equal(p_after, p_before) and torch.equal(opt.exp_avg.cpu(), m0) and torch.equal(opt.exp_avg_sq.cpu(), v0)
        return p_after
    assert norm[2].item() == 0.0 and opt.step_count == expected_step
    total, coef = ur.clip64(g32, 1.0, max_norm)
    e_total, e_coef = ur.clip_bounds(g32.numel(), total, coef, max_norm)
    _check('norm', norm[0], total, e_total, worst)
    _check('coefficient', norm[1], coef, max(e_coef, 1e-300), worst)
    if e_coef == 0.0:
        assert norm[1].item() == 1.0
    ref = ur.adam64(p_before, g32, m0, v0, expected_step, opt.param_groups[0]['lr'], opt.param_groups[0]['betas'],
                    opt.param_groups[0]['eps'], 1.0, coef)
    b = ur.adam_bounds(ref, coef, e_coef, p_after.double())
    _check('written-back gradient', opt.flat_grads, ref['g'], b['g'], worst)
    _check('m', opt.exp_avg, ref['m'], b['m'], worst)
    _check('v', opt.exp_avg_sq, ref['v'], b['v'], worst)
    _check('Delta p', p_after.double() - p_before.double(), ref['dp'], b['dp'], worst)
    return p_after


# max_norm per applied step: clipping off, coefficient exactly 1, just below 1, far below 1
CLIPS = (lambda t: 0.0, lambda t: 2.0 * t, lambda t: t * (1.0 - 2.0 ** -10), lambda t: 1e-4 * t)


def _four_steps_with_a_skip(train, opt, gen, worst):
    p = opt.flat_params.cpu()
    applied = 0
    for call in range(5):
        skip = call == 2
        if not skip:
            applied += 1
        p = _adam_step_vs_float64(train, opt, p, gen, CLIPS[applied - 1] if not skip else CLIPS[0], worst, skip=skip,
                                  expected_step=applied)
    assert opt.step_count == 4


@pytest.mark.parametrize('n', SIZES)
def test_clip_adam_vs_float64(train, n):
    """Four applied steps of ClipAdam (clip off, coefficient 1, just below 1, far below 1) with a skipped step after the
    second: the skipped step changes nothing, and the bias correction of the next step uses step 3, not 4."""
    gen = torch.Generator().manual_seed(2000 + n)
    p = torch.nn.Parameter((torch.randn(n, generator=gen) * 0.05).cuda())
    opt = train.ClipAdam([p], lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    worst = {}
    _four_steps_with_a_skip(train, opt, gen, worst)
    _report(f'ClipAdam n={n}', worst)


@pytest.mark.parametrize('n', SIZES)
def test_clip_adam_call_grad_scale_and_layout_vs_float64(train, n):
    """sunerf_clip_adam_step with the averaging factor of 1, 2 and 8 ranks and 1/3 (inexact in fp32), on buffers at storage
    offsets 0..3 floats (the norm pass's scalar path), with the device step counter."""
    from sunerf_hip import lib as _l
    from sunerf_hip.ops import _ptr, _stream
    gen = torch.Generator().manual_seed(3000 + n)
    worst = {}
    dev = torch.device('cuda', torch.cuda.current_device())
    ws = train._workspace(dev)
    lr, betas, eps = 3e-4, (0.8, 0.99), 1e-7
    for i, gs in enumerate(GRAD_SCALES):
        offset = i
        p0 = torch.randn(n, generator=gen) * 0.05
        m0 = mixed(n, gen, lo=-12.0, hi=2.0)
        v0 = mixed(n, gen, signed=False, lo=-20.0, hi=4.0)
        g32 = mixed(n, gen)
        params, grads, m, v = (placed(x, offset) for x in (p0, g32, m0, v0))
        steps = torch.tensor([i], dtype=torch.int64, device='cuda')         # i updates applied before this one
        norm = torch.zeros(4, device='cuda')
        total, _ = ur.clip64(g32, gs, 0.0)
        max_norm = CLIPS[i](total)
        _l.call(dev, 'sunerf_clip_adam_step', _ptr(params), _ptr(grads), _ptr(m), _ptr(v), n, lr, betas[0], betas[1], eps,
                max_norm, gs, 0, None, _ptr(norm), _ptr(ws), ws.numel(), _ptr(steps), _stream(dev))
        nrm = norm.cpu().double()
        assert nrm[2].item() == 0.0 and steps.item() == i + 1
        total, coef = ur.clip64(g32, gs, max_norm)
        e_total, e_coef = ur.clip_bounds(n, total, coef, max_norm)
        _check('norm', nrm[0], total, e_total, worst)
        _check('coefficient', nrm[1], coef, max(e_coef, 1e-300), worst)
        ref = ur.adam64(p0, g32, m0, v0, i + 1, lr, betas, eps, gs, coef)
        p_after = params.cpu().double()
        b = ur.adam_bounds(ref, coef, e_coef, p_after)
        _check('written-back gradient', grads, ref['g'], b['g'], worst)
        _check('m', m, ref['m'], b['m'], worst)
        _check('v', v, ref['v'], b['v'], worst)
        _check('Delta p', p_after - p0.double(), ref['dp'], b['dp'], worst)
    _report(f'sunerf_clip_adam_step n={n}', worst)


def test_clip_adam_d512_layout_vs_float64(train):
    """The reference's default width: coarse + fine NeRF(d_filter=512) in one ClipAdam, 36 tensors in one flat bucket --
    3.77 M elements, so the Adam kernel's 4096-workgroup grid strides (the d256 benchmark's 0.97 M never does)."""
    from sunerf.rendering.emission import EmissionRadiativeTransfer
    torch.manual_seed(0)
    rendering = EmissionRadiativeTransfer(Rs_per_ds=1.0, model_config={'d_filter': 512}).cuda()
    opt = train.ClipAdam(rendering.parameters(), lr=1e-4)
    assert opt.n_params == D512_PARAMS and len(opt._params) == 36
    worst = {}
    _four_steps_with_a_skip(train, opt, torch.Generator().manual_seed(4000), worst)
    off = 0
    for p in opt._params:                          # the views still cover the flat buffer that was updated
        assert p.data_ptr() == opt.flat_params[off:].data_ptr()
        off += p.numel()
    _report('ClipAdam d512', worst)
