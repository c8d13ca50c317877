"""The headline training batch at full size against the float64 oracle (oracle/sunerf_oracle.py:render_pass_f64).

bench.py's step is 32768 rays x 128 samples on the 8 x 256 network, on the default policy: the AUTO forward, the 16-bit phase
stash (18 GB), the layer-pipelined backward (csrc/bwd_pipe.hip) with the W^T arithmetic its 64-ray probe picks.  Every other
oracle comparison of the default backwards runs at <= 289 rays, where the stash stays below 2^31 bytes and each pipeline gets a
few chunks.  Here, at the sizes that run:

  headline   256 x 8, 32768 x 128   pipelined backward, 16 pipelines of 8192 chunks
  uneven     256 x 5, 32768 x 128   pipelined backward, 24 pipelines of 5462 chunks: boundaries mid-ray, the last one short
  ref-width  512 x 8,  8192 x 128   two-kernel backward (dgrad + wgrad, split 7), fp16 stash past 16 GiB, dz stash past 4 GiB

(a) the forward of every ray at the north-star gate (tests/conftest.py:gate_units) against float64;
(b) backwards whose upstream gradients are non-zero on ONE region of 64 rays only.  Zero rows add exactly zero to every kernel
    sum, so each call's gradients must equal float64 autograd over those 64 rays alone -- a fault confined to a few chunks of the
    131072 is ~1e-5 of a batch-summed gradient, but all of a region's.  Regions: the first rays (the W^T probe reads them), the
    rays whose stash byte offsets cross 2^31 ... 2^34, the first / a middle / the last pipeline (wgrad split) boundary, the last
    rays of the batch;
(c) bench.py's unmasked training step (NeRF + emission_pass + training_loss + backward + ClipAdam) against float64 autograd.

The float64 reference runs on the GPU (rocBLAS, none of the project's kernels) in chunks of REF_CHUNK rays; a 64-ray slice of it
is checked against the CPU."""
import time

import pytest
import torch

import sunerf_oracle as orc
from conftest import fp16_chain_bounds, gate_units

REF_CHUNK = 1024
GRAD_GATE = 1e-3            # every gradient tensor, relative norm
REG_RADIUS = 1.2


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available()
    from sunerf_hip import ops as _ops
    return _ops


@pytest.fixture
def default_policy(monkeypatch, ops):
    """The product's defaults: no SUNERF_* override, no forced backward."""
    for k in ('SUNERF_FORWARD_PRECISION', 'SUNERF_BACKWARD', 'SUNERF_BACKWARD_PRECISION', 'SUNERF_PIPE_HI_ONLY', 'SUNERF_STASH',
              'SUNERF_EXACT_BACKWARD_SAMPLES', 'SUNERF_GRID_CAP_WGRAD'):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(ops, '_backward_forced', None)
    ops.pipe_status(raise_on_failure=False)
    return monkeypatch


def _rel(got, ref):
    return ((got.double() - ref).norm() / ref.norm()).item()


def _rays(n_rays, S):
    """``n_rays`` rays of whole rows through the disk of a 1024 x 1024 frame (observer_rays), random times, stratified z."""
    from sunerf_hip.rays import observer_rays
    from sunerf_hip import ops
    rows = n_rays // 1024
    r0 = 512 - rows // 2
    o, d = observer_rays(1024, row_start=r0, row_end=r0 + rows, device='cuda')
    gen = torch.Generator().manual_seed(n_rays + S)
    t = (torch.rand(n_rays, 1, generator=gen) * 5.).cuda()
    z = ops.sample_z(ops.SAMPLER_STRATIFIED, o, d, torch.linspace(0, 1, S).cuda(), 1.3, 1.0)
    return o, d, t, z


# ---- the float64 reference --------------------------------------------------------------------------------------------

def test_f64_reference_restates_the_fp32_oracle():
    """render_pass_f64 (CPU) is render_pass with float64 arithmetic: same points, the fp32 oracle's outputs to fp32 rounding."""
    params = orc.init_params(d_filter=64, n_layers=3, seed=7)
    params[-1] = (params[-1][0] * 4, params[-1][1])
    o, d = orc.synthetic_rays(4)
    t = torch.rand(o.shape[0], 1, generator=torch.Generator().manual_seed(0))
    z = orc.stratified_z(o, d, orc.linspace_t_vals(40), torch.tensor(1.3), torch.tensor(1.0))
    f32 = orc.render_pass(params, o, d, t, z)
    f64 = orc.render_pass_f64(params, o, d, t, z, REG_RADIUS)
    assert f64['image'].dtype == torch.float64 and torch.equal(f64['points'], f32['points'].double())
    for k in ('raw', 'image', 'weights', 'regularizing_quantity'):
        assert ((f64[k] - f32[k].double()).abs().max() / f32[k].abs().max()).item() < 2e-6, k
    dist = f32['points'].pow(2).sum(-1).pow(0.5)
    reg = torch.relu(dist - REG_RADIUS) * (1 - f32['regularizing_quantity'])
    assert ((f64['regularization'] - reg.double()).abs().max() / reg.abs().max()).item() < 1e-5
    assert ((f64['height_map'] - (f32['weights'] * dist).sum(-1).double()).abs().max() / f64['height_map'].abs().max()).item() < 1e-6


@pytest.mark.gpu
def test_f64_reference_on_the_gpu_equals_the_cpu():
    """render_pass_f64 is plain torch: on the GPU (rocBLAS fp64) it must agree with the CPU to float64 rounding."""
    params = orc.init_params(d_filter=256, n_layers=8, seed=7)
    params[-1] = (params[-1][0] * 4, params[-1][1])
    o, d, t, z = _rays(1024, 128)
    sl = slice(480, 544)
    cpu = orc.render_pass_f64(params, o[sl].cpu(), d[sl].cpu(), t[sl].cpu(), z[sl].cpu())
    gpu = orc.render_pass_f64([(W.cuda(), b.cuda()) for W, b in params], o[sl], d[sl], t[sl], z[sl])
    worst = 0.0
    for k in ('image', 'weights', 'regularizing_quantity', 'height_map', 'absorption_map', 'regularization', 'raw'):
        assert gpu[k].dtype == torch.float64
        e = ((gpu[k].cpu() - cpu[k]).abs().max() / cpu[k].abs().max()).item()
        worst = max(worst, e)
        assert e <= 1e-12, (k, e)
    print(f'float64 reference, GPU vs CPU on 64 rays: {worst:.1e} of each tensor\'s maximum')


def _reference_outputs(params, o, d, t, z):
    """Forward outputs of render_pass_f64 for every ray, in chunks, on the GPU (no graph)."""
    p64 = [(W.cuda().double(), b.cuda().double()) for W, b in params]
    keys = ('image', 'weights', 'regularizing_quantity', 'height_map', 'absorption_map', 'regularization')
    parts = {k: [] for k in keys}
    with torch.no_grad():
        for b in range(0, o.shape[0], REF_CHUNK):
            sl = slice(b, b + REF_CHUNK)
            out = orc.render_pass_f64(p64, o[sl], d[sl], t[sl], z[sl], REG_RADIUS)
            for k in keys:
                parts[k].append(out[k])
    return {k: torch.cat(v) for k, v in parts.items()}


def _reference_grads(params, o, d, t, z, g_image, g_reg):
    """float64 autograd of  sum(image * g_image) + sum(regularization * g_reg)  over the given rays (one graph), and the bound
    per tensor: SURVEY 8d's 1e-3, or what single-fp16-operand arithmetic can deliver where the region's sums cancel
    (conftest.fp16_chain_bounds: 64 rays of random-signed g_image can; the headline's region at ray 3912 has kappa up to 3)."""
    leaves = [(W.cuda().double().requires_grad_(True), b.cuda().double().requires_grad_(True)) for W, b in params]
    out = orc.render_pass_f64(leaves, o, d, t, z, REG_RADIUS)
    out['raw'].retain_grad()
    ((out['image'][:, 0] * g_image.double()).sum() + (out['regularization'] * g_reg.double()).sum()).backward()
    bw, bb = fp16_chain_bounds([(W.cuda(), b.cuda()) for W, b in params], o, d, t, z, out['raw'].grad)
    return [(W.grad, b.grad) for W, b in leaves], [(max(GRAD_GATE, w[1]), b[1]) for w, b in zip(bw, bb)], max(k for k, _ in bb + bw)


# ---- the cases --------------------------------------------------------------------------------------------------------

CASES = {
    'headline': dict(d_filter=256, n_layers=8, n_rays=32768, S=128),
    'uneven': dict(d_filter=256, n_layers=5, n_rays=32768, S=128),
    'ref-width': dict(d_filter=512, n_layers=8, n_rays=8192, S=128),
}


def _pipelines(n_linear, cus=256):
    """Number of pipelines of the layer-pipelined backward (csrc/bwd_pipe.hip, PipeLayout): 8 XCD classes x as many whole
    pipelines of 2 (n_linear - 1) workgroups as fit a class's cus / 8."""
    return 8 * ((cus // 8) // (2 * (n_linear - 1)))


def _regions(ops, packed, n_rays, S):
    """{name: first ray} of 64-ray regions; every boundary is derived from the library's own size functions."""
    lib = ops._l.load()
    D, nl = packed.d_filter, packed.n_linear
    chunks_per_ray = (S + 31) // 32
    n_chunks = n_rays * chunks_per_ray
    last = n_rays - 64
    at = lambda ray: min(max(int(ray) - 32, 0), last)       # noqa: E731  a region centred on a ray
    regions = {'first rays': 0}
    pipe = ops.backward_mode() == 'pipe' and lib.sunerf_bwd_pipe_workspace_bytes(n_rays, S, D, nl) > 0
    fmt = ops.STASH_PHASE if pipe else ops.STASH_FP16
    # bytes per ray of the stashes (ray-major, whole 32-sample chunks; the sizes include one spare chunk)
    act_ray = (lib.sunerf_act_stash_bytes(2, S, D, nl, fmt) - lib.sunerf_act_stash_bytes(1, S, D, nl, fmt))
    stashes = [('stash', act_ray)]
    if not pipe:
        stashes.append(('dz stash', lib.sunerf_dz_stash_bytes(2, S, D, nl) - lib.sunerf_dz_stash_bytes(1, S, D, nl)))
    for name, per_ray in stashes:
        for k in (31, 32, 33, 34):
            ray = (1 << k) // per_ray          # the ray whose bytes contain offset 2^k
            if ray < n_rays:
                regions[f'{name} 2^{k} (ray {ray})'] = at(ray)
    if pipe:
        parts, what = _pipelines(nl), 'pipeline'
    else:
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        parts, what = ops.wgrad_split(nl, cus, D), 'wgrad split'
    per = -(-n_chunks // parts)
    for p in (1, parts // 2, parts - 1):
        chunk = p * per
        if chunk < n_chunks:
            regions[f'{what} {p}/{parts} (chunk {chunk}, ray {chunk // chunks_per_ray}' + ('' if chunk % chunks_per_ray == 0
                                                                                              else ' mid-ray') + ')'] = at(chunk // chunks_per_ray)
    regions['last rays'] = last
    return regions


def _params(d_filter, n_layers):
    params = orc.init_params(d_filter=d_filter, n_layers=n_layers, seed=7)
    params[-1] = (params[-1][0] * 4, params[-1][1])          # absorption active (as test_gpu_pipe._case)
    return params


@pytest.mark.gpu
@pytest.mark.parametrize('case', list(CASES))
def test_training_batch_forward_and_masked_backward(ops, default_policy, case):
    """(a) every ray of the training forward at the gate; (b) one backward per 64-ray region (x the three W^T settings of the
    pipelined backward at width 256), each against float64 autograd over that region alone."""
    monkeypatch = default_policy
    cfg = CASES[case]
    t0 = time.perf_counter()
    params = _params(cfg['d_filter'], cfg['n_layers'])
    o, d, t, z = _rays(cfg['n_rays'], cfg['S'])
    N, S = z.shape
    Ws, bs = [W.cuda() for W, _ in params], [b.cuda() for _, b in params]
    packed = ops.PackedMLP(Ws, bs)
    assert packed.auto
    fwd = ops.emission_render_fwd(packed, o, d, t, z, REG_RADIUS, want_epilogues=True, training=True)
    torch.cuda.synchronize()
    arith = ops.PRECISION_NAMES[packed.precision]
    ref = _reference_outputs(params, o, d, t, z)

    # ---- (a) ----
    units = {'image': gate_units(fwd['image'], ref['image'].cpu()),
             'height_map': gate_units(fwd['height_map'], ref['height_map'].cpu()),
             'absorption_map': gate_units(fwd['absorption_map'], ref['absorption_map'].cpu(), floor=S * 6e-8)}
    per_ray = ((fwd['image'].double() - ref['image']).abs() / (1e-4 * ref['image'].abs())).reshape(-1)
    worst_rays = torch.topk(per_ray, 3)
    rel = lambda a, r: ((a.double() - r).abs().max() / r.abs().max()).item()       # noqa: E731  (test_gpu_stages.rel_err)
    e_w, e_a = rel(fwd['weights'], ref['weights']), rel(fwd['absorption'], ref['regularizing_quantity'])
    e_reg = rel(fwd['regularization'], ref['regularization'])
    reg_tol = 1e-4 if arith == 'exact' else 4e-4
    print(f'\n[{case}] {N} rays x {S}, {cfg["n_layers"]} x {cfg["d_filter"]}: AUTO forward chose {arith} (probe {packed.last_probe:.2f}'
          f' gate units, limit {ops.PROBE_LIMIT})')
    print(f'  (a) gate units vs float64, all rays: ' + ', '.join(f'{k} {v:.3f}' for k, v in units.items())
          + f'; worst image rays {worst_rays.indices.tolist()} at {[round(v, 3) for v in worst_rays.values.tolist()]}')
    print(f'      of the maximum: weights {e_w:.1e}, absorption {e_a:.1e}, regularization {e_reg:.1e} (bound {reg_tol:.0e})')
    del ref
    for k, v in units.items():
        assert v <= 1.0, (k, v)
    assert e_w < 1e-4 and e_a < 1e-4, (e_w, e_a)
    assert e_reg <= reg_tol, e_reg

    # ---- (b) ----
    regions = _regions(ops, packed, N, S)
    gen = torch.Generator().manual_seed(17)
    masks = {}
    for name, r0 in regions.items():
        sl = slice(r0, r0 + 64)
        g_image = torch.zeros(N, device='cuda')
        g_image[sl] = (torch.randn(64, generator=gen) * 1e-3).cuda()
        g_reg = torch.zeros(N, S, device='cuda')
        g_reg[sl] = (2e-5 * (0.5 + torch.rand(64, 1, generator=gen))).cuda().expand(64, S)
        masks[name] = (sl, g_image, g_reg, _reference_grads(params, o[sl], d[sl], t[sl], z[sl], g_image[sl], g_reg[sl]))
    pipe = ops.stash_format_of(fwd['stash'], N, S, packed) == ops.STASH_PHASE
    settings = ('auto', '1', '0') if pipe else ('default',)
    worst, failures, probe = {}, [], None
    for setting in settings:
        if setting in ('1', '0'):
            monkeypatch.setenv('SUNERF_PIPE_HI_ONLY', setting)
        for name, (sl, g_image, g_reg, (want, gates, kappa)) in masks.items():
            gW = [torch.full_like(W, float('nan')) for W in Ws]
            gb = [torch.full_like(b, float('nan')) for b in bs]
            ops.emission_render_bwd(packed, o, d, z, fwd['raw'], fwd['stash'], g_image, g_reg, 0.0, REG_RADIUS, gW, gb, times=t)
            if setting == 'auto' and probe is None:
                # the W^T probe ran in this first call, on the first 64 rays: the non-zero region
                ops._pipe_w_apply(packed, block=True)
                probe = (packed.pipe_w_probe, packed.pipe_hi_only)
            errs = []
            for i, (gw, gbias, (rW, rb), (gate_w, gate_b)) in enumerate(zip(gW, gb, want, gates)):
                for kind, g, r, gate in (('W', gw, rW, gate_w), ('b', gbias, rb, gate_b)):
                    e = _rel(g, r) if torch.isfinite(g).all() else float('inf')
                    errs.append((e / gate, e, gate, f'{kind}{i}'))
                    if e > gate:
                        failures.append((setting, name, f'{kind}{i}', e, gate))
            worst[(setting, name)] = max(errs)
        torch.cuda.synchronize()
        if pipe:
            assert ops.pipe_status(raise_on_failure=False) == 0
    kind = 'pipelined' if pipe else f'two-kernel (wgrad split {ops.wgrad_split(packed.n_linear, 256, packed.d_filter)})'
    print(f'  (b) {len(regions)} regions of 64 rays, {kind} backward: worst gradient tensor vs float64 over the region, relative to its'
          f' gate ({GRAD_GATE:.0e}, or the fp16 chain bound where the region\'s sums cancel, conftest.fp16_chain_bounds):')
    if probe is not None:
        print(f'      W^T probe on rays 0-63: {probe[0]:.2e} (limit {ops.PIPE_W_LIMIT:.0e}) -> single fp16 W^T: {probe[1]}')
    for name in regions:
        print(f'      {name:48s} ' + '  '.join(f'{s}: {worst[(s, name)][1]:.2e} ({worst[(s, name)][3]}, gate {worst[(s, name)][2]:.1e})'
                                               for s in settings) + f'  [kappa {masks[name][3][2]:.2f}]')
    print(f'  case time {time.perf_counter() - t0:.1f} s')
    if probe is not None:
        assert probe[0] == probe[0] and probe[0] != float('inf'), probe
    assert not failures, failures


@pytest.mark.gpu
def test_bench_training_step_against_float64(ops, default_policy):
    """(c) bench.py's train step at the headline size, unmasked: loss within 2e-4, every gradient of the flat bucket within 1e-3,
    and ClipAdam's gradient norm within 1e-3 of float64 autograd (accumulated over ray chunks: the loss is a sum over rays)."""
    from sunerf.model.model import NeRF
    from sunerf.rendering.functional import emission_pass
    from sunerf_hip.train import ClipAdam, training_loss
    t0 = time.perf_counter()
    N, S = 32768, 128
    o, d, t, _ = _rays(N, S)
    t = t.reshape(-1)
    target = torch.rand(N, 1, generator=torch.Generator().manual_seed(1)).cuda()
    torch.manual_seed(7)
    model = NeRF(d_input=4, d_output=2, n_layers=8, d_filter=256).cuda()
    lins = model.linears()
    leaves = [(l.weight.detach().double().clone().requires_grad_(True), l.bias.detach().double().clone().requires_grad_(True))
              for l in lins]
    opt = ClipAdam(model.parameters(), lr=1e-4, max_norm=0.5)
    opt.zero_grad()
    z = ops.sample_z(ops.SAMPLER_STRATIFIED, o, d, torch.linspace(0., 1., S, device='cuda'), 1.3, 1.0)
    out = emission_pass(model, o, d, t, z, REG_RADIUS, want_epilogues=True)
    loss, stats = training_loss(out['image'], out['image'], target, out['regularization'], 0.5, 1.0, asinh_scaling=(1.0, 0.005),
                                finite_check=[out['height_map'], out['absorption_map']])
    loss.backward()
    grads = [(l.weight.grad.clone(), l.bias.grad.clone()) for l in lins]
    opt.step(skip_if_positive=stats[5:6])
    torch.cuda.synchronize()
    assert ops.pipe_status(raise_on_failure=False) == 0
    norm = opt.norm[0].item()
    arith = ops.PRECISION_NAMES[model.packed().precision]

    # float64: loss = 0.5 (mse + mse) + mean(reg) = sum over rays of (s(img) - s(tgt))^2 / N + reg / (N S)
    s_tgt = orc.asinh_scaling(target.double(), 1.0, 0.005)
    loss64 = 0.0
    for b in range(0, N, REF_CHUNK):
        sl = slice(b, b + REF_CHUNK)
        r = orc.render_pass_f64(leaves, o[sl], d[sl], t[sl, None], z[sl], REG_RADIUS)
        part = ((orc.asinh_scaling(r['image'], 1.0, 0.005) - s_tgt[sl]) ** 2).sum() / N + r['regularization'].sum() / (N * S)
        part.backward()
        loss64 += part.item()
    e_loss = abs(loss.item() - loss64) / abs(loss64)
    errs = []
    for i, ((gw, gbias), (W, b)) in enumerate(zip(grads, leaves)):
        errs += [(_rel(gw, W.grad), f'W{i}'), (_rel(gbias, b.grad), f'b{i}')]
    norm64 = torch.sqrt(sum((W.grad ** 2).sum() + (b.grad ** 2).sum() for W, b in leaves)).item()
    e_norm = abs(norm - norm64) / norm64
    w_probe = model.packed().pipe_w_probe            # None: no W^T probe ran (not the pipelined backward, or its arithmetic was forced)
    print(f'\n(c) bench step, {N} rays x {S}, AUTO forward {arith}, W^T single fp16: {model.packed().pipe_hi_only}'
          f' (probe {float("nan") if w_probe is None else w_probe:.2e})')
    print(f'    loss {loss.item():.6e} vs float64 {loss64:.6e}: {e_loss:.1e} (bound 2e-4); gradient norm {norm:.6e} vs {norm64:.6e}: '
          f'{e_norm:.1e} (bound 1e-3)')
    print('    gradient tensors vs float64: ' + ' '.join(f'{w} {e:.1e}' for e, w in errs) + f'; worst {max(errs)[0]:.2e}')
    print(f'    time {time.perf_counter() - t0:.1f} s')
    assert e_loss < 2e-4, e_loss
    for e, which in errs:
        assert e < GRAD_GATE, (which, e)
    assert e_norm < 1e-3, e_norm
