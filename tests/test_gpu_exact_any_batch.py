"""The fp32 backward at any batch size (csrc/bwd_exact.hip: sunerf_mlp_backward_exact_chunked, SUNERF_BACKWARD_PRECISION=exact):
selection, the oracle's autograd at training-batch sizes, agreement with the small-batch fp32 kernel, chunk seams and
determinism, every training path end to end, and the fast default backward measured against it at size.  Gradient errors are
test_gpu_exact._worst: per tensor ||got - ref|| / ||ref||, weights and biases separately."""
import pytest
import torch

import sunerf_oracle as orc
from test_gpu_exact import _case, _hip, _oracle, _worst

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available()
    from sunerf_hip import ops as _ops
    return _ops


@pytest.fixture(autouse=True)
def _default_policy(monkeypatch, ops):
    monkeypatch.setattr(ops, '_backward_forced', None)
    for k in ('SUNERF_BACKWARD', 'SUNERF_EXACT_BACKWARD_SAMPLES', 'SUNERF_BACKWARD_PRECISION', 'SUNERF_FORWARD_PRECISION'):
        monkeypatch.delenv(k, raising=False)


@pytest.fixture
def spy(monkeypatch, ops):
    from sunerf_hip import lib as _l
    calls = []
    real = _l.call

    def call(device, name, *a):
        calls.append(name)
        return real(device, name, *a)
    monkeypatch.setattr(_l, 'call', call)
    monkeypatch.setattr(ops._l, 'call', call)
    return calls


def _backward_kernels(calls):
    return [c for c in calls if 'backward' in c or 'dgrad' in c or 'wgrad' in c]


def _kernel(ops, packed, g_raw, query, chunked, accumulate=False, into=None):
    """One direct call of either fp32 kernel on the kernel shapes of an unpadded model."""
    f32 = dict(dtype=torch.float32, device='cuda')
    if into is None:
        into = ([torch.full(w, float('nan'), **f32) for w, _ in packed.kernel_shapes()],
                [torch.full(b, float('nan'), **f32) for _, b in packed.kernel_shapes()])
    ops._mlp_backward_exact(packed, g_raw, query, into[0], into[1], accumulate, chunked=chunked)
    torch.cuda.synchronize()
    return into


def _cpu(grads):
    return [(W.cpu(), b.cpu()) for W, b in zip(*grads)]


def test_exact_switch_selects_the_chunked_kernel_and_skips_the_stash(ops, spy, monkeypatch):
    """8192 rays x 128: under SUNERF_BACKWARD_PRECISION=exact the emission backward is the any-size fp32 kernel and nothing else, the
    training forward writes no stash (its raw output is unchanged), a backward without query points refuses; unset, the kernel
    list is today's."""
    params, o, d, t, z = _case(256, 8, 8192, 128, seed=1)
    dev = torch.device('cuda')
    Ws, bs = [W.to(dev) for W, _ in params], [b.to(dev) for _, b in params]
    packed = ops.PackedMLP(Ws, bs, precision=ops.PRECISION_EXACT)
    o, d, t, z = o.to(dev), d.to(dev), t.to(dev), z.to(dev)
    g_image = torch.randn(8192, device=dev) * 1e-3
    gW, gb = [torch.empty_like(W) for W in Ws], [torch.empty_like(b) for b in bs]

    def step():
        spy.clear()
        fwd = ops.emission_render_fwd(packed, o, d, t, z, reg_radius=1.2, training=True)
        ops.emission_render_bwd(packed, o, d, z, fwd['raw'], fwd['stash'], g_image, None, 0.0, 1.2, gW, gb, times=t)
        torch.cuda.synchronize()
        return fwd, _backward_kernels(spy)
    fwd_default, default_kernels = step()
    assert fwd_default['stash'] is not None
    assert set(default_kernels) == {'sunerf_mlp_backward_pipe'}      # today's: the layer-pipelined fp16 kernel (+ its W^T probe)
    monkeypatch.setenv('SUNERF_BACKWARD_PRECISION', 'exact')
    assert ops.backward_precision() == 'exact'
    fwd, kernels = step()
    assert kernels == ['sunerf_mlp_backward_exact_chunked']
    assert fwd['stash'] is None
    assert torch.equal(fwd['raw'], fwd_default['raw'])
    assert all(bool(torch.isfinite(g).all()) for g in gW + gb)
    # the other entry points of a training forward: free-standing points
    pts = torch.randn(1000, 4, device=dev)
    assert ops.mlp_points_fwd(packed, pts, training=True)['stash'] is None
    # no query points: a clear error, never the fp16 kernels in its place
    spy.clear()
    with pytest.raises(RuntimeError, match='SUNERF_BACKWARD_PRECISION=exact'):
        ops.emission_render_bwd(packed, o, d, z, fwd['raw'], None, g_image, None, 0.0, 1.2, gW, gb)
    assert _backward_kernels(spy) == []
    # a kernel forced by name does not override the switch
    monkeypatch.setattr(ops, '_backward_forced', 'classic')
    monkeypatch.setenv('SUNERF_BACKWARD', 'classic')
    assert step()[1] == ['sunerf_mlp_backward_exact_chunked']
    monkeypatch.setattr(ops, '_backward_forced', None)
    monkeypatch.delenv('SUNERF_BACKWARD')
    monkeypatch.setenv('SUNERF_BACKWARD_PRECISION', 'fp64')
    with pytest.raises(ValueError):
        ops.emission_render_fwd(packed, o, d, t, z, reg_radius=1.2, training=True)
    monkeypatch.delenv('SUNERF_BACKWARD_PRECISION')
    assert set(step()[1]) == set(default_kernels)


@pytest.mark.parametrize('d_filter,n_layers,n_rays,S', [(256, 8, 2048, 128), (512, 3, 1024, 65)])
def test_matches_the_oracle_autograd_at_training_batch_size(ops, monkeypatch, d_filter, n_layers, n_rays, S):
    """262 144 (8 x 256) and 66 560 (3 x 512) samples, exact forward, against torch.autograd on the fp32 oracle: every tensor
    within 1e-4 (measured worst printed)."""
    params, o, d, t, z = _case(d_filter, n_layers, n_rays, S, seed=S)
    g_image = torch.randn(n_rays) * 1e-3
    ref, _ = _oracle(params, o, d, t, z, g_image, 2e-5)
    monkeypatch.setenv('SUNERF_BACKWARD_PRECISION', 'exact')
    got = _hip(ops, params, o, d, t, z, g_image, 2e-5)
    worst = _worst(got, ref)
    print(f'{n_layers} x {d_filter}, {n_rays} rays x {S}: any-size fp32 backward worst tensor {worst:.2e} (bound 1e-4)')
    assert worst <= 1e-4


@pytest.mark.parametrize('d_filter,n_layers,n_rays,S', [(256, 8, 17, 128), (256, 8, 17, 2), (64, 3, 33, 33), (128, 7, 17, 2), (64, 4, 33, 3),
                                                        (512, 3, 5, 65), (64, 1, 1, 2), (256, 2, 100, 31), (128, 8, 3, 200)])
def test_equals_the_small_batch_kernel(ops, d_filter, n_layers, n_rays, S):
    """The shapes of test_gpu_exact's oracle test (one chunk each): the any-size kernel and sunerf_mlp_backward_exact agree to 1e-6
    (same forward and data-gradient chains; the weight gradients' long sums are split differently)."""
    params, o, d, t, z = _case(d_filter, n_layers, n_rays, S, seed=S)
    dev = torch.device('cuda')
    packed = ops.PackedMLP([W.to(dev) for W, _ in params], [b.to(dev) for _, b in params], precision=ops.PRECISION_EXACT)
    g_raw = torch.randn(n_rays, S, 2, device=dev)
    query = ('rays', o.to(dev), d.to(dev), t.to(dev), z.to(dev))
    small = _cpu(_kernel(ops, packed, g_raw, query, chunked=False))
    anysize = _cpu(_kernel(ops, packed, g_raw, query, chunked=True))
    worst = _worst(anysize, small)
    print(f'{n_layers} x {d_filter}, {n_rays} x {S}: any-size vs small-batch kernel {worst:.1e}')
    assert worst <= 1e-6


@pytest.mark.parametrize('width,encoding', [(48, 'positional'), (100, 'positional'), (320, 'positional'), (48, None)])
def test_padded_widths_and_raw_coordinates_equal_the_small_batch_kernel(ops, monkeypatch, width, encoding):
    """Zero-padded widths and a first layer without positional encoding, through mlp_backward on free-standing points (the
    small-batch fp32 kernel by default at 1000 samples, the any-size one under the switch): within 1e-6."""
    from sunerf.model.model import NeRF
    torch.manual_seed(width)
    net = NeRF(d_input=4, d_output=2, n_layers=3, d_filter=width, encoding=encoding).cuda()
    packed = net.packed()
    assert packed.padded
    pts = torch.randn(1000, 4, device='cuda')
    g_raw = torch.randn(1000, 1, 2, device='cuda')
    absmax = g_raw.abs().max().reshape(1).view(torch.int32)

    def grads():
        gW = [torch.full_like(l.weight, float('nan')) for l in net.linears()]
        gb = [torch.full_like(l.bias, float('nan')) for l in net.linears()]
        ops.mlp_backward(packed, g_raw, absmax, None, gW, gb, query=('points', pts))
        torch.cuda.synchronize()
        return [(W.cpu(), b.cpu()) for W, b in zip(gW, gb)]
    small = grads()
    monkeypatch.setenv('SUNERF_BACKWARD_PRECISION', 'exact')
    anysize = grads()
    worst = _worst(anysize, small)
    print(f'width {width}, encoding {encoding}: any-size vs small-batch kernel {worst:.1e}')
    assert worst <= 1e-6


def test_chunk_seams_accumulation_and_determinism(ops):
    """2 chunks + 37 samples in one call == the same samples in two accumulate calls split off the chunk grid (within fp32
    rounding of the final casts), and a rerun is bit-identical."""
    params, _, _, _, _ = _case(64, 3, 1, 2)
    dev = torch.device('cuda')
    packed = ops.PackedMLP([W.to(dev) for W, _ in params], [b.to(dev) for _, b in params], precision=ops.PRECISION_EXACT)
    n = 2 * 32768 + 37
    torch.manual_seed(4)
    pts = torch.randn(n, 4, device=dev)
    g_raw = torch.randn(n, 1, 2, device=dev)
    whole = _kernel(ops, packed, g_raw, ('points', pts), chunked=True)
    again = _kernel(ops, packed, g_raw, ('points', pts), chunked=True)
    assert all(torch.equal(a, b) for a, b in zip(whole[0] + whole[1], again[0] + again[1]))
    cut = 40000
    halves = _kernel(ops, packed, g_raw[:cut], ('points', pts[:cut].contiguous()), chunked=True)
    _kernel(ops, packed, g_raw[cut:], ('points', pts[cut:].contiguous()), chunked=True, accumulate=True, into=halves)
    worst = _worst(_cpu(halves), _cpu(whole))
    print(f'{n} samples, one call vs two accumulated halves: {worst:.1e}')
    assert worst <= 1e-6


def test_emission_module_training_step_end_to_end(ops, monkeypatch, spy):
    """EmissionSuNeRFModule.training_step with SUNERF_FORWARD_PRECISION=exact + SUNERF_BACKWARD_PRECISION=exact, 1024 rays x (64 + 128)
    samples: every parameter gradient within 1e-4 of the oracle's render_emission autograd; through ClipAdam's flat bucket the
    gradients are those of the step without it."""
    from sunerf.model.sunerf import EmissionSuNeRFModule
    monkeypatch.setenv('SUNERF_FORWARD_PRECISION', 'exact')
    monkeypatch.setenv('SUNERF_BACKWARD_PRECISION', 'exact')

    def config():       # fresh dicts: the module pops their 'type' keys (base_tracing.py, like the reference)
        return dict(Rs_per_ds=1.0, seconds_per_dt=1.0, image_scaling_config={'vmax': 1, 'a': 0.005},
                    sampling_config={'type': 'stratified', 'n_samples': 64, 'perturb': False},
                    hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 128}, model_config={'d_filter': 128})
    torch.manual_seed(21)
    lm = EmissionSuNeRFModule(**config())
    sd = {k: v.clone() for k, v in lm.rendering.state_dict().items()}
    side = 33
    o, d = orc.synthetic_rays(side)
    o, d = o[:1024].contiguous(), d[:1024].contiguous()
    t = torch.rand(1024, 1)
    target = torch.rand(1024, 1) * 0.1
    batch = {'tracing': {'rays': torch.stack([o, d], 1).cuda(), 'time': t.cuda(), 'target_image': target.cuda()}}

    def hip_step(flat):
        m = EmissionSuNeRFModule(**config())
        m.rendering.load_state_dict(sd, strict=True)
        m = m.cuda()
        if flat:
            (opt,), _ = m.configure_optimizers()
            opt.zero_grad()
        spy.clear()
        loss = m.training_step(batch, 0)
        loss.backward()
        torch.cuda.synchronize()
        assert 'sunerf_mlp_backward_exact_chunked' in spy and not any(k in spy for k in (
            'sunerf_mlp_backward_pipe', 'sunerf_mlp_dgrad', 'sunerf_mlp_wgrad', 'sunerf_mlp_backward_exact'))
        return loss.item(), m
    loss, m = hip_step(False)
    leaves = {}
    for part in ('coarse', 'fine'):
        leaves[part] = [(W.clone().requires_grad_(True), b.clone().requires_grad_(True))
                        for W, b in orc.params_from_state_dict(sd, f'{part}_model.')]
    out = orc.render_emission(leaves['coarse'], leaves['fine'], o, d, t, n_coarse=64, n_fine=128, t_vals=sd['sampler.t_vals'])
    ref_loss = orc.emission_training_loss(out, target, vmax=1, a=0.005)['loss']
    ref_loss.backward()
    assert abs(loss - ref_loss.item()) <= 2e-4 * abs(ref_loss.item())
    worst = {}
    for part in ('coarse', 'fine'):
        got = [(l.weight.grad.cpu(), l.bias.grad.cpu()) for l in getattr(m.rendering, f'{part}_model').linears()]
        worst[part] = _worst(got, [(W.grad, b.grad) for W, b in leaves[part]])
    print(f"exact + exact training step, 1024 rays x (64 + 128): worst coarse tensor {worst['coarse']:.2e}, fine {worst['fine']:.2e} (bound 1e-4)")
    assert max(worst.values()) <= 1e-4
    _, mf = hip_step(True)
    for a, b in zip(m.rendering.parameters(), mf.rendering.parameters()):
        assert ((a.grad - b.grad).norm() / a.grad.norm()).item() <= 1e-6


def test_generic_ray_and_point_paths(ops, monkeypatch, spy):
    """_MlpOnRays (the generic plug-in path) and _MlpOnPoints (free-standing points) under the switch: the any-size kernel, with
    the gradients of the small-batch fp32 kernel the default picks at this size."""
    from sunerf.model.model import NeRF
    from sunerf.rendering.functional import _MlpOnRays, mlp_points
    torch.manual_seed(8)
    net = NeRF(d_input=4, d_output=2, n_layers=4, d_filter=128).cuda()
    params, o, d, t, z = _case(128, 4, 20, 50)
    o, d, t, z = o.cuda(), d.cuda(), t.cuda(), z.cuda()
    pts = torch.randn(777, 4, device='cuda')
    probe_r, probe_p = torch.randn(20, 50, 2, device='cuda'), torch.randn(777, 2, device='cuda')
    flat = []
    for lin in net.linears():
        flat += [lin.weight, lin.bias]

    def grads(which):
        net.zero_grad(set_to_none=True)
        spy.clear()
        if which == 'rays':
            loss = (_MlpOnRays.apply(net, o, d, t, z, *flat) * probe_r).sum()
        else:
            loss = (mlp_points(net, pts) * probe_p).sum()
        loss.backward()
        torch.cuda.synchronize()
        return [(l.weight.grad.cpu(), l.bias.grad.cpu()) for l in net.linears()], _backward_kernels(spy)
    for which in ('rays', 'points'):
        small, k0 = grads(which)
        monkeypatch.setenv('SUNERF_BACKWARD_PRECISION', 'exact')
        anysize, k1 = grads(which)
        monkeypatch.delenv('SUNERF_BACKWARD_PRECISION')
        assert k0 == ['sunerf_mlp_backward_exact'] and k1 == ['sunerf_mlp_backward_exact_chunked'], (which, k0, k1)
        assert _worst(anysize, small) <= 1e-6, which


@pytest.mark.parametrize('flat_bucket', [False, True])
def test_dt_training_step_exact(ops, monkeypatch, spy, flat_bucket):
    """The DT fused pass (NeRF_DT, golden g6) with both switches exact: every gradient within test_gpu_dt's gate, through the
    any-size kernel."""
    import test_gpu_dt
    monkeypatch.setenv('SUNERF_FORWARD_PRECISION', 'exact')
    monkeypatch.setenv('SUNERF_BACKWARD_PRECISION', 'exact')
    test_gpu_dt.test_dt_training_step_gradients(flat_bucket)
    kernels = _backward_kernels(spy)
    assert kernels and set(kernels) == {'sunerf_mlp_backward_exact_chunked'}, kernels


def test_default_backward_against_the_exact_one_at_size(ops, monkeypatch):
    """Yardstick for the fast path: 8192 rays x 128, default weights and policies (pipelined backward, measured W^T image): every
    tensor within 1e-3 of the any-size fp32 backward on the same batch (a hand-run comparison once measured 5.98e-4)."""
    from sunerf.model.model import NeRF
    torch.manual_seed(0)
    net = NeRF(d_input=4, d_output=2, n_layers=8, d_filter=256).cuda()
    packed = net.packed()
    _, o, d, t, z = _case(256, 8, 8192, 128, seed=3)
    o, d, t, z = o.cuda(), d.cuda(), t.cuda(), z.cuda()
    fwd = ops.emission_render_fwd(packed, o, d, t, z, reg_radius=1.2, training=True)
    g_image = torch.randn(8192, device='cuda') * 1e-3

    def grads():
        gW = [torch.full_like(l.weight, float('nan')) for l in net.linears()]
        gb = [torch.full_like(l.bias, float('nan')) for l in net.linears()]
        ops.emission_render_bwd(packed, o, d, z, fwd['raw'], fwd['stash'], g_image, None, 2e-5, 1.2, gW, gb, times=t)
        torch.cuda.synchronize()
        return [(W.cpu(), b.cpu()) for W, b in zip(gW, gb)]
    fast = grads()
    monkeypatch.setenv('SUNERF_BACKWARD_PRECISION', 'exact')
    exact = grads()
    worst = _worst(fast, exact)
    print(f'8192 x 128, 8 x 256: default backward vs the fp32 one, worst tensor {worst:.2e} (hand-run before: 5.98e-4; bound 1e-3)')
    assert worst <= 1e-3
