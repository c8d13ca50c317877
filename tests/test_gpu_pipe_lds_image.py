"""The LDS image of the pipelined backward's hidden stages (csrc/bwd_pipe.hip, "LDS IMAGE": fragments 1088 bytes apart, the
pair skew) at the smallest shapes where a wrong row, a wrong fragment base or a wrapped staging buffer shows: the
pipelined backward against the fp64 oracle and against the two-kernel backward, helpers and the 1e-3 per-tensor bound of
test_gpu_pipe.py.  A row or a fragment taken from the wrong place pairs a dZ with another sample's or another feature's
activation: the sums then differ from the oracle's by their own size, not by 1e-3."""
import pytest
import torch

import test_gpu_pipe as tp
from test_gpu_pipe import _split_weights, ops  # noqa: F401  (fixtures: the module's library handle, W^T as head + remainder)

pytestmark = pytest.mark.gpu


def _compare(ops, params, o, d, t, z, what):
    g_image = torch.randn(o.shape[0]) * 1e-3
    ref = tp._oracle_grads(params, o, d, t, z, g_image, 2e-5)
    classic, _ = tp._hip_grads(ops, 'classic', params, o, d, t, z, g_image, 2e-5)
    pipe, status = tp._hip_grads(ops, 'pipe', params, o, d, t, z, g_image, 2e-5)
    assert status == 0
    worst_ref = worst_classic = 0.0
    for i, ((rW, rb), (cW, cb), (pW, pb)) in enumerate(zip(ref, classic, pipe)):
        assert torch.isfinite(pW).all() and torch.isfinite(pb).all(), i
        for name, r, c, p in (('weight', rW, cW, pW), ('bias', rb, cb, pb)):
            e_ref = ((p - r).norm() / r.norm()).item()
            e_cls = ((p - c).norm() / c.norm()).item()
            worst_ref, worst_classic = max(worst_ref, e_ref), max(worst_classic, e_cls)
            assert e_ref < 1e-3, (i, name, 'vs oracle', e_ref)
            assert e_cls < 1e-3, (i, name, 'vs two-kernel backward', e_cls)
    print(f'{what}: pipelined vs oracle {worst_ref:.2e}, vs two-kernel {worst_classic:.2e}')


# (1, 33, 8): one ray, a full and a ragged chunk, most pipelines empty; (5, 128, 8): 100 chunks, 6 - 7 per pipeline -- every one of
# the five staging buffers is reused; (9, 128, 3): the shortest network (one hidden stage: the top stage feeds the in-layer stage)
@pytest.mark.parametrize('n_side,S,n_layers', [(1, 33, 8), (5, 128, 8), (9, 128, 3)])
def test_lds_image_matches_oracle_and_two_kernel_backward(ops, n_side, S, n_layers):
    params, o, d, t, z = tp._case(n_side, S, n_layers)
    _compare(ops, params, o, d, t, z, f'{o.shape[0]} rays x {S}, {n_layers} layers')


def test_lds_image_with_distinct_amplifying_feature_scales(ops):
    """Hidden weights amplify as in test_pipelined_backward_with_amplifying_hidden_weights (x 2 on average), but every output
    feature j of a hidden layer by its own factor 1.5 + j / 256: rows of dZ and of the activations differ in size feature by
    feature, so two swapped rows or fragments move a weight gradient by tens of per cent of its norm."""
    params, o, d, t, z = tp._case(5, 128, 8)
    scale = (1.5 + torch.arange(256, dtype=torch.float32) / 256.)[:, None]
    params = [(W * scale, b) if 0 < i < len(params) - 1 else (W, b) for i, (W, b) in enumerate(params)]
    _compare(ops, params, o, d, t, z, 'per-feature scales 1.5 .. 2.5')
