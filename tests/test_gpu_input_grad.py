"""Gradients w.r.t. the query of the MLP (csrc/bwd_exact.hip: sunerf_mlp_input_grad_exact, through _MlpOnPoints / _MlpOnRays):
``NeRF(points)`` w.r.t. the points and ``mlp_on_rays`` w.r.t. rays_o / rays_d / times / z_vals, against torch.autograd of the oracle in
float64.  Gate, per point (per ray for the ray sums, per ray row for g_z): e = ||g - g64||_inf / ||g64||_inf must stay within
max(1e-4, 4 e_cpu32), e_cpu32 the same oracle's float32 CPU autograd error on that point (phases up to 256 |x| make some points
ill-conditioned in any fp32 evaluation).  Parameter gradients taken alongside are test_gpu_exact._worst within 1e-4 of the oracle
and bit-identical to the chunked fp32 parameter backward.
Measured worst e_gpu / max(1e-4, 4 e_cpu32), MI355X: points 0.10 (e_gpu 1.03e-5; all widths, both encodings, up to 70 001 points),
rays 0.62 (g_t at S = 2, where the fp32 rounding of o + d z sets the error for the CPU too), generic render path 0.27; parameter
gradients alongside 1.3e-6."""
import pytest
import torch

import sunerf_oracle as orc
from test_gpu_exact import _worst

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


def _net(d_filter, n_layers, encoding, seed, cls=None):
    from sunerf.model.model import NeRF
    torch.manual_seed(seed)
    net = (cls or NeRF)(d_input=4, d_output=2, n_layers=n_layers, d_filter=d_filter, encoding=encoding)
    return net.cuda()


def _params(net, dtype):
    return [(l.weight.detach().cpu().to(dtype), l.bias.detach().cpu().to(dtype)) for l in net.linears()]


def _rowwise(g, ref):
    """Per row: ||g - ref||_inf / ||ref||_inf (rows: the leading dimension)."""
    g, ref = g.detach().cpu().double().reshape(ref.shape[0], -1), ref.double().reshape(ref.shape[0], -1)
    return (g - ref).abs().amax(1) / ref.abs().amax(1).clamp_min(1e-300)


def _gate(name, got, g64, g32):
    """Worst ratio e_gpu / max(1e-4, 4 e_cpu32) over the rows; <= 1 passes."""
    e_gpu, e_cpu = _rowwise(got, g64), _rowwise(g32, g64)
    ratio = (e_gpu / torch.clamp(4 * e_cpu, min=1e-4)).max().item()
    print(f'  {name}: worst e_gpu {e_gpu.max().item():.2e}, worst ratio to the gate {ratio:.3f}')
    return ratio


def _oracle_points(params, x, g_raw, encoding, dtype, offsets=None):
    x = x.detach().to(dtype).clone().requires_grad_(True)      # (a copy: .to() of the same dtype returns the tensor itself)
    leaves = [tuple(v.detach().to(dtype).clone().requires_grad_(True) for v in p) for p in params]
    raw = orc.mlp_forward(leaves, x, encoding=encoding)
    if offsets is not None:
        raw = raw + raw.new_tensor(offsets)
    (raw * g_raw.to(dtype)).sum().backward()
    return x.grad, [(W.grad, b.grad) for W, b in leaves]


def _oracle_rays(params, o, d, t, z, loss, dtype):
    """float64 / float32 CPU autograd of ``loss(raw (N, S, 2))`` w.r.t. rays_o, rays_d, times (N, 1), z_vals."""
    o, d, t, z = (v.detach().to(dtype).clone().requires_grad_(True) for v in (o, d, t, z))
    pts = orc.points_on_rays(o, d, z)
    x = torch.cat([pts, t[:, None, :].expand(-1, z.shape[1], 1)], -1)
    raw = orc.mlp_forward([(W.to(dtype), b.to(dtype)) for W, b in params], x.reshape(-1, 4)).reshape(*z.shape, -1)
    loss(raw).backward()
    return o.grad, d.grad, t.grad, z.grad


_POINT_CASES = [(d, enc, m) for d in (64, 100, 256, 512) for enc in ('positional', None) for m in (1, 31, 33, 4097)]
_POINT_CASES += [(256, 'positional', 70001), (256, None, 70001)]


@pytest.mark.parametrize('trainable', [False, True], ids=['frozen', 'trainable'])
@pytest.mark.parametrize('d_filter,encoding,m', _POINT_CASES)
def test_point_gradients_against_the_fp64_oracle(ops, d_filter, encoding, m, trainable):
    """NeRF(points)['inferences'] with a random upstream gradient: points.grad against fp64 autograd of orc.mlp_forward.  Frozen:
    the output still has a grad_fn (it had none before: the node was taken for trainable parameters only).  Trainable: the
    parameter gradients come from the same call, within 1e-4 of the oracle.  70 001 points cross the 32 768-sample chunk seam twice."""
    n_layers = 4
    net = _net(d_filter, n_layers, encoding, seed=d_filter + m)
    for p in net.parameters():
        p.requires_grad_(trainable)
    torch.manual_seed(m)
    x = (torch.rand(m, 4) * 4 - 2)
    g_raw = torch.randn(m, 2)
    xg = x.cuda().requires_grad_(True)
    out = net(xg)['inferences']
    assert out.grad_fn is not None
    (out * g_raw.cuda()).sum().backward()
    assert xg.grad is not None and xg.grad.shape == (m, 4)
    params = _params(net, torch.float32)
    use_enc = encoding == 'positional'
    g64, p64 = _oracle_points(params, x, g_raw, use_enc, torch.float64)
    g32, _ = _oracle_points(params, x, g_raw, use_enc, torch.float32)
    print(f'{d_filter} {encoding} M={m} {"trainable" if trainable else "frozen"}:')
    assert _gate('points', xg.grad, g64, g32) <= 1
    if trainable:
        got = [(l.weight.grad.cpu(), l.bias.grad.cpu()) for l in net.linears()]
        worst = _worst(got, p64)
        print(f'  parameters: worst tensor {worst:.1e}')
        assert worst <= 1e-4
    else:
        assert all(p.grad is None for p in net.parameters())


def _ray_case(n_rays, S, seed):
    torch.manual_seed(seed)
    side = int(n_rays ** 0.5) + 1
    o, d = orc.synthetic_rays(side)
    o, d = o[:n_rays].contiguous(), d[:n_rays].contiguous()
    d = d * (0.9 + 0.2 * torch.rand(n_rays, 1))
    t = torch.rand(n_rays, 1)
    z = orc.stratified_z(o, d, orc.linspace_t_vals(S), torch.tensor(1.3), torch.tensor(1.0))
    return o, d, t, z


@pytest.mark.parametrize('S,n_rays', [(2, 16500), (97, 400), (128, 300)])
def test_ray_gradients_against_the_fp64_oracle(ops, S, n_rays):
    """mlp_on_rays with rays_o, rays_d, times and z_vals as leaves; N * S > 32 768 (two chunks); at S = 97 ray 337 straddles the
    chunk seam and its sums are carried into the second chunk."""
    from sunerf.rendering.functional import mlp_on_rays
    net = _net(256, 4, 'positional', seed=S)
    for p in net.parameters():
        p.requires_grad_(False)
    o, d, t, z = _ray_case(n_rays, S, seed=S)
    g_raw = torch.randn(n_rays, S, 2)
    leaves = [v.cuda().requires_grad_(True) for v in (o, d, t, z)]
    raw = mlp_on_rays(net, *leaves)
    (raw * g_raw.cuda()).sum().backward()
    params = _params(net, torch.float32)
    loss = lambda r: (r * g_raw.to(r.dtype)).sum()
    ref64 = _oracle_rays(params, o, d, t, z, loss, torch.float64)
    ref32 = _oracle_rays(params, o, d, t, z, loss, torch.float32)
    print(f'rays {n_rays} x {S}:')
    for name, got, g64, g32 in zip(('g_o', 'g_d', 'g_t', 'g_z'), leaves, ref64, ref32):
        assert got.grad is not None and got.grad.shape == got.shape
        assert _gate(name, got.grad, g64, g32) <= 1, name
    # the kernel's own error, without the fp32 rounding of o + d z that dominates the gate above: fp64 autograd at the points as fp32
    # forms them; each ray's error against the scale of what was summed -- the per-point gradients' magnitudes ||g_x||_inf (the
    # per-point gate's norm; a single component such as g_t can be far smaller than its point's gradient)
    pts = orc.points_on_rays(o, d, z)
    x = torch.cat([pts, t[:, None, :].expand(-1, S, 1)], -1).double().reshape(-1, 4).requires_grad_(True)
    raw = orc.mlp_forward([(W.double(), b.double()) for W, b in params], x).reshape(n_rays, S, -1)
    (raw * g_raw.double()).sum().backward()
    gx = x.grad.reshape(n_rays, S, 4)
    zd, dd = z.double(), d.double()
    gn = gx.abs().amax(-1)                                                          # (N, S)
    refs = {'g_o': (gx[..., :3].sum(1), gn.sum(1)), 'g_d': ((zd[..., None] * gx[..., :3]).sum(1), (zd.abs() * gn).sum(1)),
            'g_t': (gx[..., 3:].sum(1), gn.sum(1)), 'g_z': ((dd[:, None, :] * gx[..., :3]).sum(-1), dd.abs().sum(-1)[:, None] * gn)}
    for name, got in zip(('g_o', 'g_d', 'g_t', 'g_z'), leaves):
        ref, scale = refs[name]
        err = (got.grad.detach().cpu().double().reshape(ref.shape) - ref).abs()
        e = (err.reshape(n_rays, -1) / scale.reshape(n_rays, -1)).max().item()
        print(f'  {name} at the fp32 points: worst error / summed ||g_x||_inf {e:.1e}')
        assert e <= 1e-4, name


def test_parameter_gradients_alongside_are_bit_identical_to_the_chunked_kernel(ops):
    """Points and parameters both need gradients: one call gives both; the parameter gradients equal
    ops._mlp_backward_exact(..., chunked=True) bit for bit on the same query (two chunks) and are within 1e-4 of the oracle."""
    m = 40000
    net = _net(256, 4, 'positional', seed=5)
    torch.manual_seed(6)
    x = torch.rand(m, 4) * 4 - 2
    g_raw = torch.randn(m, 2)
    xg = x.cuda().requires_grad_(True)
    (net(xg)['inferences'] * g_raw.cuda()).sum().backward()
    got = [(l.weight.grad.clone(), l.bias.grad.clone()) for l in net.linears()]
    packed = net.packed()
    assert not packed.padded
    gW = [torch.full_like(W, float('nan')) for W, _ in got]
    gb = [torch.full_like(b, float('nan')) for _, b in got]
    ops._mlp_backward_exact(packed, g_raw.cuda().reshape(m, 1, 2), ('points', x.cuda()), gW, gb, False, chunked=True)
    torch.cuda.synchronize()
    for (W, b), w2, b2 in zip(got, gW, gb):
        assert torch.equal(W, w2) and torch.equal(b, b2)
    _, p64 = _oracle_points(_params(net, torch.float32), x, g_raw, True, torch.float64)
    worst = _worst([(W.cpu(), b.cpu()) for W, b in got], p64)
    print(f'parameters alongside point gradients: worst tensor {worst:.1e}')
    assert worst <= 1e-4
    # accumulate into existing .grad (the flat-bucket form of the same call adds into the buffers)
    (net(xg)['inferences'] * g_raw.cuda()).sum().backward()
    for (W, b), l in zip(got, net.linears()):
        assert torch.allclose(l.weight.grad, 2 * W, rtol=1e-6, atol=0) and torch.allclose(l.bias.grad, 2 * b, rtol=1e-6, atol=0)


def test_nerf_dt_forward_point_gradients(ops):
    """NeRF_DT.forward: the base offsets are constants, so the point gradient is the MLP's."""
    from sunerf.model.model import NeRF_DT
    net = _net(128, 3, 'positional', seed=8, cls=NeRF_DT)
    m = 2000
    torch.manual_seed(9)
    x = torch.rand(m, 4) * 4 - 2
    g_raw = torch.randn(m, 2)
    xg = x.cuda().requires_grad_(True)
    (g,) = torch.autograd.grad((net(xg)['inferences'] * g_raw.cuda()).sum(), xg)
    params = _params(net, torch.float32)
    off = [net.base_log_density, net.base_log_temperature]
    g64, _ = _oracle_points(params, x, g_raw, True, torch.float64, off)
    g32, _ = _oracle_points(params, x, g_raw, True, torch.float32, off)
    print('NeRF_DT.forward:')
    assert _gate('points', g, g64, g32) <= 1


def test_generic_render_path_reaches_the_rays(ops):
    """A SuNeRFRendering subclass whose raw2outputs loss reaches the rays through field_on_query_points (the generic _render of
    base_tracing.py): g_o, g_d, g_t, g_z against the oracle."""
    from sunerf.rendering.base_tracing import SuNeRFRendering, ray_query_points

    def raw2outputs(raw, z_vals):
        w = torch.softmax(raw[..., 0], -1)
        return {'image': (w * raw[..., 1] * z_vals).sum(-1, keepdim=True), 'weights': w,
                'regularizing_quantity': torch.sigmoid(raw[..., 0])}

    class Toy(SuNeRFRendering):
        def raw2outputs(self, raw, z_vals, rays_d, rays_o, query_points):
            return raw2outputs(raw, z_vals)

    torch.manual_seed(10)
    mod = Toy(Rs_per_ds=1.0, model_config={'d_filter': 64, 'n_layers': 3}).cuda()
    o, d, t, z = _ray_case(300, 40, seed=11)
    leaves = [v.cuda().requires_grad_(True) for v in (o, d, t, z)]
    lo, ld, lt, lz = leaves
    out = mod._render(mod.fine_model, ray_query_points(lo, ld, lt, lz), ld, lo, lz)
    g_img = torch.randn(300, 1)
    (out['image'] * g_img.cuda()).sum().backward()
    params = _params(mod.fine_model, torch.float32)
    ref = {}
    for dtype in (torch.float64, torch.float32):
        def loss(r, dtype=dtype):
            return (raw2outputs(r, z.to(dtype).requires_grad_(False))['image'] * g_img.to(dtype)).sum()
        ref[dtype] = _oracle_rays(params, o, d, t, z, loss, dtype)
    print('generic render path:')
    for i, name in enumerate(('g_o', 'g_d', 'g_t')):
        assert _gate(name, leaves[i].grad, ref[torch.float64][i], ref[torch.float32][i]) <= 1, name


def test_z_gradient_through_the_generic_render_path(ops):
    """The same with the loss's own use of z_vals left out, so that g_z is the MLP's alone (d . g_xyz)."""
    from sunerf.rendering.base_tracing import SuNeRFRendering, ray_query_points

    class Toy(SuNeRFRendering):
        def raw2outputs(self, raw, z_vals, rays_d, rays_o, query_points):
            return {'image': raw[..., :1].sum(1), 'weights': raw[..., 0], 'regularizing_quantity': raw[..., 1]}

    torch.manual_seed(12)
    mod = Toy(Rs_per_ds=1.0, model_config={'d_filter': 64, 'n_layers': 3}).cuda()
    o, d, t, z = _ray_case(200, 33, seed=13)
    leaves = [v.cuda().requires_grad_(True) for v in (o, d, t, z)]
    lo, ld, lt, lz = leaves
    out = mod._render(mod.fine_model, ray_query_points(lo, ld, lt, lz), ld, lo, lz)
    (out['image'] * 3.0).sum().backward()
    params = _params(mod.fine_model, torch.float32)
    loss = lambda r: (r[..., 0] * 3.0).sum()
    ref64 = _oracle_rays(params, o, d, t, z, loss, torch.float64)
    ref32 = _oracle_rays(params, o, d, t, z, loss, torch.float32)
    print('generic render path, z only through the MLP:')
    for name, got, g64, g32 in zip(('g_o', 'g_d', 'g_t', 'g_z'), leaves, ref64, ref32):
        assert _gate(name, got.grad, g64, g32) <= 1, name


def test_determinism(ops):
    """Two backward calls give bit-identical input gradients (points over two chunks; rays with a ray across the seam)."""
    from sunerf.rendering.functional import mlp_on_rays
    net = _net(128, 4, 'positional', seed=14)
    torch.manual_seed(15)
    x = (torch.rand(40000, 4, device='cuda') * 4 - 2).requires_grad_(True)
    g = torch.randn(40000, 2, device='cuda')
    a = torch.autograd.grad((net(x)['inferences'] * g).sum(), x)[0]
    b = torch.autograd.grad((net(x)['inferences'] * g).sum(), x)[0]
    assert torch.equal(a, b)
    o, d, t, z = (v.cuda().requires_grad_(True) for v in _ray_case(400, 97, seed=16))
    gr = torch.randn(400, 97, 2, device='cuda')
    first = torch.autograd.grad((mlp_on_rays(net, o, d, t, z) * gr).sum(), (o, d, t, z))
    second = torch.autograd.grad((mlp_on_rays(net, o, d, t, z) * gr).sum(), (o, d, t, z))
    assert all(torch.equal(u, v) for u, v in zip(first, second))


def test_second_order_raises(ops):
    """create_graph=True on the input-gradient path raises instead of returning gradients that carry no graph."""
    from sunerf.rendering.functional import mlp_on_rays
    net = _net(64, 3, 'positional', seed=17)
    x = torch.rand(100, 4, device='cuda').requires_grad_(True)
    with pytest.raises(RuntimeError, match='second derivatives'):
        torch.autograd.grad(net(x)['inferences'].sum(), x, create_graph=True)
    o, d, t, z = (v.cuda() for v in _ray_case(10, 8, seed=18))
    o.requires_grad_(True)
    with pytest.raises(RuntimeError, match='second derivatives'):
        torch.autograd.grad(mlp_on_rays(net, o, d, t, z).sum(), o, create_graph=True)
