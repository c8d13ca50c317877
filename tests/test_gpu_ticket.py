"""The last-workgroup ticket (csrc/ordered_sum.h) under the use it is made for: launches of different grids queued
on ONE workspace and one stream with no synchronisation between them.  Each of the four kernels that draw a ticket -- the training
loss, the clip norm in front of Adam, the likelihood and the SSIM loss -- runs small, large, small; the first and the third call
must agree word for word, and every call must agree word for word with the same call on a fresh, zeroed workspace.  A ticket that
is not back at zero when the next launch starts, a last workgroup that reads a partial before it is visible, or one that reads a
stale partial of the launch before, all show here; the rerun tests of the kernels' own files use a workspace per call size or per
stream and would not see the first.

Sizes at the seams of the last stage: 1, 256, 257 and 128 * 256 + 1 elements are one workgroup, one, two, and the cap of 128
workgroups with a second sweep; the likelihood crosses them with 1 and 2 table rows (grids of 1, 2 and 128 against the last
workgroup's groups of 8); the SSIM loss takes 1, 256 and 257 patches of 8 x 8 at window 7, where the last workgroup's run length
goes from 1 to 2."""
import ctypes

import numpy as np
import pytest
import torch

import likelihood_reference as lr

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SIZES = (1, 256, 257, 128 * 256 + 1)


def _words(out):
    return [t.detach().contiguous().view(torch.uint8) for t in out]


def _small_large_small(run, small, large, nbytes):
    """``run(case, workspace)`` queues one call and returns its output tensors without synchronising."""
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    queued = [run(small, ws), run(large, ws), run(small, ws)]
    torch.cuda.synchronize()
    assert int(ws[:4].view(torch.int32).item()) == 0, 'the ticket is back at zero'
    fresh = [run(case, torch.zeros(nbytes, dtype=torch.uint8, device=DEV)) for case in (small, large, small)]
    torch.cuda.synchronize()
    for i, (got, want) in enumerate(zip(queued, fresh)):
        for k, (a, b) in enumerate(zip(_words(got), _words(want))):
            assert torch.equal(a, b), f'call {i}, output {k}: differs from the same call on a fresh workspace'
    for k, (a, b) in enumerate(zip(_words(queued[0]), _words(queued[2]))):
        assert torch.equal(a, b), f'output {k}: the first and the third call differ'


def _other(n):
    return SIZES[-1] if n != SIZES[-1] else 257


def _lib():
    from sunerf_hip import lib
    return lib


def _images(n, seed):
    gen = torch.Generator().manual_seed(seed)
    return [(torch.rand(n, generator=gen) * 3.0).to(DEV) for _ in range(4)]          # coarse, fine, target, regularization


@pytest.mark.parametrize('scaling', (0, 1), ids=('mse', 'asinh'))
@pytest.mark.parametrize('n', SIZES)
def test_training_loss_small_large_small_on_one_workspace(n, scaling):
    from sunerf_hip._ffi import _ptr, _stream
    lib = _lib()
    dev = torch.device(DEV, torch.cuda.current_device())
    none = (ctypes.c_void_p * 1)()
    sizes = (ctypes.c_int64 * 1)()

    def run(case, ws):
        coarse, fine, target, reg = case
        g_coarse, g_fine, stats = torch.empty_like(coarse), torch.empty_like(fine), torch.empty(8, device=DEV)
        lib.call(dev, 'sunerf_training_loss', _ptr(coarse), _ptr(fine), _ptr(target), coarse.numel(), _ptr(reg), reg.numel(), none, sizes, 0,
                 scaling, 2.0, 0.005, 1.0, 0.5, _ptr(g_coarse), _ptr(g_fine), _ptr(stats), _ptr(ws), ws.numel(), _stream(dev))
        return stats, g_coarse, g_fine
    _small_large_small(run, _images(n, n), _images(_other(n), n + 1), lib.load().sunerf_train_workspace_bytes())


@pytest.mark.parametrize('n', SIZES)
def test_clip_norm_small_large_small_on_one_workspace(n):
    from sunerf_hip._ffi import _ptr, _stream
    lib = _lib()
    dev = torch.device(DEV, torch.cuda.current_device())

    def run(case, ws):
        params, grads, m, v = (t.clone() for t in case)          # the step writes all four
        norm, steps = torch.zeros(4, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
        lib.call(dev, 'sunerf_clip_adam_step', _ptr(params), _ptr(grads), _ptr(m), _ptr(v), params.numel(), 3e-4, 0.9, 0.999, 1e-8, 0.5, 1.0, 0,
                 None, _ptr(norm), _ptr(ws), ws.numel(), _ptr(steps), _stream(dev))
        return norm, params, grads, m, v, steps

    def case(size, seed):
        params, grads, m, v = _images(size, seed)
        return params - 1.5, grads - 1.5, m - 1.5, v
    _small_large_small(run, case(n, 10 + n), case(_other(n), 11 + n), lib.load().sunerf_train_workspace_bytes())


@pytest.mark.parametrize('mode', (lr.OBSERVED, lr.MODEL), ids=('observed', 'model'))
@pytest.mark.parametrize('rows', (1, 2))
@pytest.mark.parametrize('n', SIZES)
def test_likelihood_small_large_small_on_one_workspace(n, rows, mode):
    from sunerf_hip.likelihood import launch

    def case(size, seed):
        c = lr.make_case(size, 1, rows, seed)
        c['reg'] = c['reg'][:size]          # as many as slots: the grid is the slots'
        return {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in c.items()}

    def run(d, ws):
        return launch(d['coarse'], d['fine'], d['target'], d['codes'], d['row_codes'], d['noise'], d['log_gain'], mode, d['reg'], [], 0.75,
                      0.5, workspace=ws)
    _small_large_small(run, case(n, 0), case(_other(n), 1), _lib().load().sunerf_likelihood_workspace_bytes(rows))


@pytest.mark.parametrize('n', (1, 256, 257))
def test_ssim_loss_small_large_small_on_one_workspace(n):
    from sunerf_hip.ssim_loss import launch
    P, window = 8, 7
    other = 257 if n != 257 else 256

    def case(patches, seed):
        gen = torch.Generator().manual_seed(seed)
        target = torch.rand(patches * P * P, 1, generator=gen)
        return [(target + 0.1 * torch.rand(target.shape, generator=gen)).to(DEV) for _ in range(2)] + [target.to(DEV), patches]

    def run(c, ws):
        coarse, fine, target, patches = c
        return launch(coarse, fine, target, patches, P, 1.0, window, workspace=ws)
    _small_large_small(run, case(n, n), case(other, n + 1), _lib().load().sunerf_ssim_loss_workspace_bytes(257, 1))
