"""The pipelined backward's data-gradient waves decode the NEXT chunk's phases behind the matrix instructions of their k-steps
(csrc/bwd_pipe.hip, the order of an iteration in hidden_stage): the cases in which that order can go wrong -- no main-loop iteration at all, a single
one (chunk 0 is decoded in the prologue iterations and nothing behind it), the wrap of the five staging buffers, ragged last
chunks, every layer count -- on BOTH builds of the kernel: W^T as fp16 head + remainder (SUNERF_PIPE_HI_ONLY=0, what
test_gpu_pipe.py forces) and the single fp16 W^T that the benchmark runs (=1).  Bounds: those of test_gpu_pipe.py for the same
comparisons (1e-3 relative L2 per tensor against the oracle's autograd and against the two-kernel backward)."""
import pytest
import torch

import sunerf_oracle as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available()
    from sunerf_hip import ops as _ops
    return _ops


def _pipeline_counts(n_rays, S, n_layers):
    """The launcher's partition of the chunks over the pipelines (bwd_pipe.hip: PipeLayout, bwd_pipe_kernel): eight classes of
    CUs, 2 n_act workgroups per pipeline, ceil(chunks / pipelines) consecutive chunks each."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n_pipes = 8 * ((cus // 8) // (2 * n_layers))
    total = n_rays * ((S + 31) // 32)
    per = (total + n_pipes - 1) // n_pipes
    return sorted({max(0, min(per, total - p * per)) for p in range(n_pipes)})


def _case(n_rays, S, n_layers, hidden_scale=1.0):
    torch.manual_seed(0)
    params = orc.init_params(d_filter=256, n_layers=n_layers, seed=3)
    params = [(W * hidden_scale, b) if 0 < i < len(params) - 1 else (W, b) for i, (W, b) in enumerate(params)]
    W, b = params[-1]
    params[-1] = (W * 4, b)          # absorption active on about half of the samples
    n_side = 1
    while n_side * n_side < n_rays:
        n_side += 1
    o, d = orc.synthetic_rays(n_side)
    o, d = o[:n_rays].contiguous(), d[:n_rays].contiguous()
    d = d * (0.9 + 0.2 * torch.rand(d.shape[0], 1))
    t = torch.rand(o.shape[0], 1) * 5.
    z = orc.stratified_z(o, d, orc.linspace_t_vals(S), torch.tensor(1.3), torch.tensor(1.0))
    g_image = torch.randn(o.shape[0]) * 1e-3
    return params, o, d, t, z, g_image


def _oracle_grads(params, o, d, t, z, g_image, g_reg_const):
    leaves = [(W.clone().requires_grad_(True), b.clone().requires_grad_(True)) for W, b in params]
    out = orc.render_pass(leaves, o, d, t, z)
    dist_pts = out['points'].pow(2).sum(-1).pow(0.5)
    reg = torch.relu(dist_pts - 1.2) * (1 - out['regularizing_quantity'])
    ((out['image'][:, 0] * g_image).sum() + g_reg_const * reg.sum()).backward()
    return [(W.grad, b.grad) for W, b in leaves]


def _hip_grads(ops, mode, params, o, d, t, z, g_image, g_reg_const, launches=1):
    """Gradients of every launch (same stash, same workspace) and the status word."""
    dev = torch.device('cuda')
    Ws, bs = [W.to(dev) for W, _ in params], [b.to(dev) for _, b in params]
    packed = ops.PackedMLP(Ws, bs, precision=ops.PRECISION_EXACT)
    prev = ops._backward_forced
    ops._backward_forced = mode          # (before the forward: it leaves the stash in the format this backward reads)
    runs = []
    try:
        fwd = ops.emission_render_fwd(packed, o.to(dev), d.to(dev), t.to(dev), z.to(dev), reg_radius=1.2, training=True)
        for _ in range(launches):
            gW = [torch.full_like(W, float('nan')) for W in Ws]
            gb = [torch.full_like(b, float('nan')) for b in bs]
            ops.emission_render_bwd(packed, o.to(dev), d.to(dev), z.to(dev), fwd['raw'], fwd['stash'], g_image.to(dev), None,
                                    g_reg_const, 1.2, gW, gb)
            runs.append([(W.cpu(), b.cpu()) for W, b in zip(gW, gb)])
        torch.cuda.synchronize()
        status = ops.pipe_status(raise_on_failure=False)
    finally:
        ops._backward_forced = prev
    return runs, status


# (rays, samples per ray, layers) -> the chunk counts per pipeline that the case is there for (256 CUs: 16 / 24 / 40 pipelines of
# 8 / 5 / 3 layers); S = 17, 33, 40 end in a ragged chunk
CASES = [
    (1, 33, 8, (0, 1)),        #   2 chunks: two pipelines with one main-loop iteration, fourteen with none
    (9, 17, 8, (0, 1)),        #   9 chunks
    (9, 40, 8, (0, 2)),        #  18 chunks: nine pipelines with 2
    (95, 32, 8, (5, 6)),       #  95 chunks: fifteen pipelines with 6, one with 5 -- the five staging buffers wrap
    (83, 40, 8, (1, 11)),      # 166 chunks: fifteen pipelines with 11, one with 1
    (49, 33, 3, (0, 2, 3)),    #  98 chunks over 40 pipelines
    (25, 17, 5, (0, 1, 2)),    #  25 chunks over 24 pipelines
]
_reference = {}      # case -> (inputs, oracle gradients, two-kernel gradients): computed once, shared by both builds, never changed


def _reference_of(ops, case):
    if case not in _reference:
        n_rays, S, n_layers, _ = case
        inputs = _case(n_rays, S, n_layers)
        classic, _ = _hip_grads(ops, 'classic', *inputs, 2e-5)
        _reference[case] = (inputs, _oracle_grads(*inputs, 2e-5), classic[0])
    return _reference[case]


@pytest.mark.parametrize('hi_only', ['0', '1'])
@pytest.mark.parametrize('case', CASES, ids=lambda c: f'{c[0]}x{c[1]}-L{c[2]}')
def test_chunk_counts_ragged_chunks_and_layer_counts(ops, monkeypatch, case, hi_only):
    n_rays, S, n_layers, wanted = case
    counts = _pipeline_counts(n_rays, S, n_layers)
    print(f'{n_rays} rays x {S}, {n_layers} layers, SUNERF_PIPE_HI_ONLY={hi_only}: chunks per pipeline {counts}')
    assert set(wanted) <= set(counts), (wanted, counts)
    inputs, ref, classic = _reference_of(ops, case)
    monkeypatch.setenv('SUNERF_PIPE_HI_ONLY', hi_only)
    (pipe,), status = _hip_grads(ops, 'pipe', *inputs, 2e-5)
    assert status == 0
    worst_ref = worst_classic = 0.0
    for i, ((rW, rb), (cW, cb), (pW, pb)) in enumerate(zip(ref, classic, pipe)):
        assert torch.isfinite(pW).all() and torch.isfinite(pb).all(), i
        for name, r, c, p in (('weight', rW, cW, pW), ('bias', rb, cb, pb)):
            e_ref = ((p - r).norm() / r.norm()).item()
            e_cls = ((p - c).norm() / c.norm()).item()
            worst_ref, worst_classic = max(worst_ref, e_ref), max(worst_classic, e_cls)
    print(f'   pipelined vs oracle {worst_ref:.2e}, vs two-kernel {worst_classic:.2e}')
    for i, ((rW, rb), (cW, cb), (pW, pb)) in enumerate(zip(ref, classic, pipe)):
        for name, r, c, p in (('weight', rW, cW, pW), ('bias', rb, cb, pb)):
            assert ((p - r).norm() / r.norm()).item() < 1e-3, (i, name, 'vs oracle')
            assert ((p - c).norm() / c.norm()).item() < 1e-3, (i, name, 'vs two-kernel backward')


@pytest.mark.parametrize('hi_only', ['0', '1'])
def test_two_launches_on_one_stash_and_workspace_give_the_same_bits(ops, monkeypatch, hi_only):
    """The second launch finds the staging buffers, rings and counters of the first.  The parent of this change (decoder behind the
    epilogue) is bit-identical from launch to launch on both builds (fixed chunk -> pipeline assignment, fixed summation order;
    measured with this very test), so bit-identity is what is asserted."""
    inputs = _case(95, 40, 8)            # 190 chunks: 12 per pipeline, one with 10
    monkeypatch.setenv('SUNERF_PIPE_HI_ONLY', hi_only)
    runs, status = _hip_grads(ops, 'pipe', *inputs, 0.0, launches=3)
    assert status == 0
    for later in runs[1:]:
        for (aW, ab), (bW, bb) in zip(runs[0], later):
            assert torch.isfinite(aW).all() and torch.isfinite(ab).all()
            assert torch.equal(aW, bW) and torch.equal(ab, bb)


def test_single_fp16_build_saturates_instead_of_overflowing(ops, monkeypatch):
    """The condition of test_gpu_backward.py::test_backward_saturates_instead_of_overflowing (hidden weights x 16: dZ outgrows
    fp16 and clamps at +-65504 through MODE.FP16_OVFL, which the decoder's fp16 sines now share a k-step loop with) on the single
    fp16 W^T build of the pipelined kernel."""
    params, o, d, t, z, _ = _case(16, 32, 8, hidden_scale=16.0)
    monkeypatch.setenv('SUNERF_PIPE_HI_ONLY', '1')
    (grads,), status = _hip_grads(ops, 'pipe', params, o, d, t, z, torch.ones(o.shape[0]), 0.0)
    assert status == 0
    assert all(torch.isfinite(W).all() and torch.isfinite(b).all() for W, b in grads)
    assert grads[1][0].abs().max().item() > 0
