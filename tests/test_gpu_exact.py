"""The fp32 backward for small batches (csrc/bwd_exact.hip, sunerf_mlp_backward_exact) against the oracle's autograd, the
policy that selects it (sunerf_hip/ops.py:_backward_path), and a fixed slice of the randomised parity sweep
(tests/tools/fuzz_parity.py) with every gradient tensor -- biases included -- at SURVEY 8d's 1e-3."""
import os
import sys

import pytest
import torch

import sunerf_oracle as orc
from conftest import fp16_chain_bias_bounds

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available()
    from sunerf_hip import ops as _ops
    return _ops


@pytest.fixture(autouse=True)
def _default_policy(monkeypatch, ops):
    monkeypatch.setattr(ops, '_backward_forced', None)
    monkeypatch.delenv('SUNERF_BACKWARD', raising=False)
    monkeypatch.delenv('SUNERF_EXACT_BACKWARD_SAMPLES', raising=False)


def _case(d_filter, n_layers, n_rays, S, seed=0, hidden=1.0):
    torch.manual_seed(seed)
    params = orc.init_params(d_filter=d_filter, n_layers=n_layers, seed=11 + seed)
    params = [(W * hidden, b) if 0 < i < len(params) - 1 else (W, b) for i, (W, b) in enumerate(params)]
    W, b = params[-1]
    params[-1] = (W * 4, b)
    side = int(n_rays ** 0.5) + 1
    o, d = orc.synthetic_rays(side)
    o, d = o[:n_rays].contiguous(), d[:n_rays].contiguous()
    d = d * (0.9 + 0.2 * torch.rand(n_rays, 1))
    t = torch.rand(n_rays, 1) * 5.
    z = orc.stratified_z(o, d, orc.linspace_t_vals(S), torch.tensor(1.3), torch.tensor(1.0))
    return params, o, d, t, z


def _oracle(params, o, d, t, z, g_image, g_reg_const):
    leaves = [(W.clone().requires_grad_(True), b.clone().requires_grad_(True)) for W, b in params]
    out = orc.render_pass(leaves, o, d, t, z)
    out['raw'].retain_grad()
    reg = torch.relu(out['points'].pow(2).sum(-1).pow(0.5) - 1.2) * (1 - out['regularizing_quantity'])
    ((out['image'][:, 0] * g_image).sum() + g_reg_const * reg.sum()).backward()
    return [(W.grad, b.grad) for W, b in leaves], out['raw'].grad


def _oracle64(params, o, d, t, z, g_image, g_reg_const):
    """The same gradients in float64 (orc.render_pass_f64): the yardstick both fp32 evaluations are measured against."""
    leaves = [(W.double().requires_grad_(True), b.double().requires_grad_(True)) for W, b in params]
    out = orc.render_pass_f64(leaves, o, d, t, z, 1.2)
    ((out['image'][:, 0] * g_image.double()).sum() + g_reg_const * out['regularization'].sum()).backward()
    return [(W.grad, b.grad) for W, b in leaves]


def _hip(ops, params, o, d, t, z, g_image, g_reg_const, times=True, accumulate_twice=False):
    dev = torch.device('cuda')
    Ws, bs = [W.to(dev) for W, _ in params], [b.to(dev) for _, b in params]
    packed = ops.PackedMLP(Ws, bs, precision=ops.PRECISION_EXACT)
    fwd = ops.emission_render_fwd(packed, o.to(dev), d.to(dev), t.to(dev), z.to(dev), reg_radius=1.2, training=True)
    gW, gb = [torch.full_like(W, float('nan')) for W in Ws], [torch.full_like(b, float('nan')) for b in bs]
    args = (packed, o.to(dev), d.to(dev), z.to(dev), fwd['raw'], fwd['stash'], g_image.to(dev), None, g_reg_const, 1.2, gW, gb)
    ops.emission_render_bwd(*args, times=t.to(dev) if times else None)
    if accumulate_twice:
        ops.emission_render_bwd(*args, accumulate=True, times=t.to(dev) if times else None)
    torch.cuda.synchronize()
    return [(W.cpu(), b.cpu()) for W, b in zip(gW, gb)]


def _worst(got, ref):
    return max(max(((W.double() - rW).norm() / rW.norm()).item(), ((b.double() - rb).norm() / rb.norm()).item())
               for (W, b), (rW, rb) in zip(got, ref))


@pytest.mark.parametrize('d_filter,n_layers,n_rays,S', [(256, 8, 17, 128), (256, 8, 17, 2), (64, 3, 33, 33), (128, 7, 17, 2), (64, 4, 33, 3),
                                                        (512, 3, 5, 65), (64, 1, 1, 2), (256, 2, 100, 31), (128, 8, 3, 200)])
def test_fp32_backward_matches_the_oracle_autograd(ops, d_filter, n_layers, n_rays, S):
    """Every tensor of every shape -- the three shapes the randomised sweep of round 3 found outside the gate included (d 64 / 128,
    34 ... 1100 samples) -- within 1e-4 of torch.autograd on the fp32 oracle (measured 4e-7 ... 5e-5: printed) and within 1e-4 of
    float64 autograd (orc.render_pass_f64); the fp16 kernels on the same inputs, for comparison, against the bound their arithmetic
    allows (conftest.fp16_chain_bias_bounds).  The kernel-vs-fp32-oracle difference is the sum of two fp32 evaluations' rounding
    errors; the float64 reference splits it (printed side by side) and puts it on the KERNEL's side: the fp32 oracle is <= 1.8e-6
    from float64 in every case, the kernel up to 4.5e-5 (2 x 256, 100 rays x 31: the 4.7e-5 seen against the fp32 oracle).  The
    kernel is not the more accurate side, so the bound stays 1e-4 against both."""
    params, o, d, t, z = _case(d_filter, n_layers, n_rays, S, seed=S)
    assert n_rays * S <= ops.exact_backward_limit()
    g_image = torch.randn(n_rays) * 1e-3
    ref, ref_graw = _oracle(params, o, d, t, z, g_image, 2e-5)
    got = _hip(ops, params, o, d, t, z, g_image, 2e-5)
    worst = _worst(got, ref)
    ref64 = _oracle64(params, o, d, t, z, g_image, 2e-5)
    worst64, oracle64 = _worst(got, ref64), _worst(ref, ref64)
    fp16 = _hip(ops, params, o, d, t, z, g_image, 2e-5, times=False)          # no query -> the fp16 kernels, as before
    model = fp16_chain_bias_bounds(params, o, d, t, z, ref_graw)
    eb16 = [((b - rb).norm() / rb.norm()).item() for (_, b), (_, rb) in zip(fp16, ref)]
    ew16 = max(((W - rW).norm() / rW.norm()).item() for (W, _), (rW, _) in zip(fp16, ref))
    print(f'{n_layers} x {d_filter}, {n_rays} rays x {S}: fp32 backward worst tensor {worst:.1e} vs the fp32 oracle; vs float64: kernel '
          f'{worst64:.1e}, fp32 oracle {oracle64:.1e}; fp16 kernels: weights {ew16:.1e}, biases '
          + ' '.join(f'{e:.1e} (kappa {k:.1f}, bound {bd:.1e})' for e, (k, bd) in zip(eb16, model)))
    assert worst < 1e-4
    assert worst64 < 1e-4
    for l, (e, (_, bound)) in enumerate(zip(eb16, model)):
        assert e <= bound, (l, e, bound)


def test_fp32_backward_accumulates_and_handles_padded_models(ops):
    params, o, d, t, z = _case(64, 3, 9, 40)
    g_image = torch.randn(9) * 1e-3
    ref, _ = _oracle(params, o, d, t, z, g_image, 0.0)
    twice = _hip(ops, params, o, d, t, z, g_image, 0.0, accumulate_twice=True)
    for (W, b), (rW, rb) in zip(twice, ref):
        assert ((W - 2 * rW).norm() / rW.norm()).item() < 4e-5 and ((b - 2 * rb).norm() / rb.norm()).item() < 4e-5
    # a width that runs zero-padded (100 -> 128) and a first layer without positional encoding, through the module API
    from sunerf.model.model import NeRF
    torch.manual_seed(3)
    for kw in ({'d_filter': 100}, {'d_filter': 48, 'encoding': None}):
        net = NeRF(d_input=4, d_output=2, n_layers=3, **kw).cuda()
        x = torch.randn(300, 4, device='cuda')
        probe = torch.randn(300, 2, device='cuda')
        (net(x)['inferences'] * probe).sum().backward()
        lin = net.linears()
        leaves = [(l.weight.detach().cpu().clone().requires_grad_(True), l.bias.detach().cpu().clone().requires_grad_(True)) for l in lin]
        (orc.mlp_forward(leaves, x.cpu(), encoding=kw.get('encoding', 'positional') is not None) * probe.cpu()).sum().backward()
        for (W, b), layer in zip(leaves, lin):
            assert ((layer.weight.grad.cpu() - W.grad).norm() / W.grad.norm()).item() < 2e-5
            assert ((layer.bias.grad.cpu() - b.grad).norm() / b.grad.norm()).item() < 2e-5


def test_policy_small_batches_fp32_large_batches_and_named_kernels_fp16(ops, monkeypatch):
    from sunerf_hip import lib as _l
    calls = []
    real = _l.call

    def spy(device, name, *a):
        calls.append(name)
        return real(device, name, *a)
    monkeypatch.setattr(_l, 'call', spy)
    monkeypatch.setattr(ops._l, 'call', spy)
    params, o, d, t, z = _case(256, 8, 17, 128)
    g_image = torch.randn(17) * 1e-3

    def kernels(**kw):
        calls.clear()
        _hip(ops, params, o, d, t, z, g_image, 0.0, **kw)
        return [c for c in calls if 'backward' in c or 'dgrad' in c or 'wgrad' in c]
    assert kernels() == ['sunerf_mlp_backward_exact']                          # 2176 samples: the default
    assert kernels(times=False) == ['sunerf_mlp_backward_pipe']                # no query points: only the stash can serve
    monkeypatch.setenv('SUNERF_EXACT_BACKWARD_SAMPLES', '2000')
    assert kernels() == ['sunerf_mlp_backward_pipe']                           # above the limit
    monkeypatch.setenv('SUNERF_EXACT_BACKWARD_SAMPLES', '0')
    assert kernels() == ['sunerf_mlp_backward_pipe']                           # switched off
    monkeypatch.delenv('SUNERF_EXACT_BACKWARD_SAMPLES')
    monkeypatch.setenv('SUNERF_BACKWARD', 'classic')
    assert kernels() == ['sunerf_mlp_dgrad', 'sunerf_mlp_wgrad']               # a kernel asked for by name is honoured
    monkeypatch.delenv('SUNERF_BACKWARD')
    monkeypatch.setattr(ops, '_backward_forced', 'pipe')
    assert kernels() == ['sunerf_mlp_backward_pipe']
    monkeypatch.setattr(ops, '_backward_forced', None)
    ops.pipe_status(raise_on_failure=False)


def test_fixed_slice_of_the_randomised_parity_sweep(ops):
    """24 cases of tests/tools/fuzz_parity.py (seed 1: widths 64 ... 512, 1 ... 8 layers, 1 ... 300 rays, 2 ... 200 samples incl. every
    ragged size, hidden x 0.25 ... 2, both forward arithmetics) through the product's default path: forward inside its gates and
    EVERY gradient tensor within 1e-3 of the oracle.  Case 23 (33 rays x 33 samples, layer-1 bias 2.0e-3 under the fp16 kernels) is
    in the slice; the full sweep with cases 37 and 57: python tests/tools/fuzz_parity.py 60 1."""
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'tools'))
    import fuzz_parity
    bad = fuzz_parity.sweep(24, 1, grad_gate=1e-3, verbose=print)
    assert bad == [], bad
