"""Every kernel entry point of the C ABI stays inside its buffers (include/sunerf_hip.h; cases: tests/abi_cases.py, the guarded
arena: tests/abi_arena.py).

Per (entry point, shape) the entry point is called directly through ``lib.call`` semantics on arena buffers whose extents are
the ones the header states:

1. run A -- guards, outputs and workspaces hold the finite sentinel: the call returns 0, no guard word of any buffer (inputs
   included) has changed, every input is bit-for-bit what it was, every output equals the project's own wrapper on the same
   inputs by bits and holds no sentinel where the header says it is written;
2. run B -- the same call with NaN / 0xFF in guards, outputs and workspaces: guards untouched, outputs bit-identical to run A
   (a read outside an input, a workspace taken to be zero, an output accumulated into without being INOUT would differ);
3. the workspace bound -- the size the ``*_workspace_bytes()`` function returns is what runs 1 and 2 were given; one byte less
   returns SUNERF_E_WORKSPACE and leaves every buffer untouched;
4. the empty call -- the count the header documents as "nothing to do" returns 0 and leaves every buffer untouched (or has
   exactly the documented effect).

5. documented rejections -- a count the header refuses (``n_rays == 0`` of the fp32 backward, ...) returns that status and
   leaves every buffer untouched.

Bit equality is the rule.  A case is ``reproducible=False`` only for a reason that stands in the kernel source (float atomics,
named in the case): the outputs those atomics add up are then always held to the tolerance of the kernel's own test file
(imported from there), every other output of the case to its bits; whether a rerun of the wrapper differs is printed, and
decides nothing.  Opaque outputs (a layout the header does not give) must be written, equal the wrapper path's bytes where
written, and agree between the runs.  Guards are always compared by bits.  Every check prints one line per buffer."""
import pytest
import torch

import abi_cases as ac
from abi_arena import IN, INOUT, OUT, WORKSPACE, pattern_bytes

pytestmark = pytest.mark.gpu

E_WORKSPACE = -3
PAIRS = [(name, shape) for name, (_, shapes) in ac.CASES.items() for shape in shapes]
_FAULT = []          # a HIP error ends the session: nothing more is launched on a device that has faulted


def _bytes_of(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


def _call(case, dev, overrides=None):
    """The raw status of the entry point (``lib.call`` raises on a non-zero one; the workspace check wants to see -3)."""
    from sunerf_hip import lib, ops
    fn = getattr(lib.load(), case.name)
    with torch.cuda.device(dev):
        status = fn(*case.ctypes_args(ops._stream(dev), overrides))
    try:
        torch.cuda.synchronize(dev)
    except RuntimeError as e:          # an illegal access surfaces here
        _FAULT.append(f'{case.name} {case.shape}: {e}')
        raise
    if status > 0:
        _FAULT.append(f'{case.name} {case.shape}: HIP error {status}')
    return status


def _check_guards(case, what):
    ok, report = case.arena.guards_intact()
    print(f'{case.name} {ac.shape_id(case.shape)} {what}:')
    print('\n'.join(case.arena.lines(report)))
    assert ok, f'{what}: guard words were written: ' + '; '.join(
        f'{name} front {r["front"]} back {r["back"]}' for name, r in report.items() if r['front'][0] or r['back'][0])


def _run(case, dev, pattern, initial):
    arena = case.arena
    for b in arena.tagged(INOUT):
        b.bytes.copy_(initial[b.name])
    arena.fill_guards(pattern)
    arena.fill_payload(pattern, (OUT, WORKSPACE))
    status = _call(case, dev)
    assert status == 0, f'run {pattern}: status {status}'
    _check_guards(case, f'run {pattern}')
    for b in arena.tagged(IN):
        assert torch.equal(b.bytes, initial[b.name]), f'run {pattern}: input {b.name} was written'
    return arena.payload_bits(OUT, INOUT)


def _untouched(case, before, what, but=()):
    for b in case.arena.buffers:
        if b.name not in but:
            assert torch.equal(b.bytes, before[b.name]), f'{what}: {b.name} was written'


@pytest.mark.parametrize('name,shape', PAIRS, ids=[f'{n[7:]}-{ac.shape_id(s)}' for n, s in PAIRS])
def test_entry_point_stays_inside_its_buffers(name, shape):
    check_entry_point(ac.CASES[name][0], name, shape)


def check_entry_point(builder, name, shape):
    """The checks of this file's docstring on the case ``builder(shape, device)`` builds for the entry point ``name``; the tables
    beside the core one (tests/test_gpu_*_abi.py) call it with the builders of their own case tables."""
    if _FAULT:
        pytest.exit(f'a GPU fault ended the session: {_FAULT[0]}', returncode=3)
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    dev = torch.device('cuda', torch.cuda.current_device())
    case = builder(shape, dev)
    assert case.name == name
    arena = case.arena
    initial = arena.payload_bits(IN, INOUT)

    if case.expect_status is not None:          # a documented rejection: that status, and nothing written
        arena.fill_guards('A')
        arena.fill_payload('A', (OUT, WORKSPACE))
        before = arena.payload_bits()
        status = _call(case, dev)
        assert status == case.expect_status, f'status {status}, the header documents {case.expect_status}'
        _check_guards(case, 'refused call')
        _untouched(case, before, 'refused call')
        return

    # ---- run A ---------------------------------------------------------------------------------------------------------------
    got_a = _run(case, dev, 'A', initial)
    for b in arena.tagged(OUT):
        # (a byte buffer holds the sentinel byte by chance once in 256 bytes: it is held to the wrapper's bits instead)
        if b.name not in case.opaque and b.dtype != torch.uint8:
            left = b.holds_pattern('A')
            assert left == 0, f'{left} of {b.numel} elements of {b.name} still hold the sentinel'
    want = case.expected()
    torch.cuda.synchronize(dev)
    compared = [b for b in arena.tagged(OUT, INOUT) if b.name not in case.opaque]
    assert set(want) - case.opaque == {b.name for b in compared}, (sorted(want), sorted(b.name for b in compared))
    # reproducible=False is decided by the kernel source (the case names the atomic adds), never by a run: the outputs it names
    # are always held to the imported tolerance.  Whether a rerun of the wrapper happens to differ is printed, nothing more.
    exempt = not case.reproducible
    if exempt:
        again = case.expected()
        differs = any(not torch.equal(_bytes_of(want[k]), _bytes_of(again[k])) for k in want)
        print(f'reproducible=False: a rerun of the wrapper {"differs" if differs else "agrees"} by bits')
    for b in arena.tagged(OUT):
        if b.name in case.opaque:
            # layout not in the header: the call must have written something, and where it wrote, what the wrapper's path wrote
            word_a = torch.tensor(list(pattern_bytes('A', b.dtype)), dtype=torch.uint8, device=dev).repeat(b.numel)
            written = got_a[b.name] != word_a
            assert int(written.sum()) > 0, f'{b.name}: nothing was written'
            if b.name in want:
                w = _bytes_of(want[b.name]).to(dev)
                assert w.numel() == b.nbytes, (b.name, w.numel(), b.nbytes)
                bad = written & (got_a[b.name] != w)
                assert not bool(bad.any()), f'{b.name}: {int(bad.sum())} written bytes differ from the wrapper, first at ' \
                                            f'{int(torch.nonzero(bad)[0, 0])}'
    for b in compared:
        w = want[b.name]
        assert w.dtype == b.dtype and w.numel() == b.numel, (b.name, w.dtype, tuple(w.shape), b.numel)
        if exempt:
            case.tolerance(b.name, got_a[b.name].view(b.dtype), w.to(dev))
        else:
            differ = (got_a[b.name] != _bytes_of(w).to(dev)).view(b.numel, b.itemsize).any(1)
            assert not bool(differ.any()), f'{b.name}: {int(differ.sum())} of {b.numel} elements differ from the wrapper by bits, ' \
                                           f'first at {int(torch.nonzero(differ)[0, 0])}'

    # ---- run B ---------------------------------------------------------------------------------------------------------------
    got_b = _run(case, dev, 'B', initial)
    for b in arena.tagged(OUT, INOUT):
        a_bits, b_bits = got_a[b.name], got_b[b.name]
        if b.name in case.opaque:
            # the layout is not the header's: what run A wrote, run B wrote with the same bits, and nothing else -- per byte
            # either the two runs agree, or both still hold their own pattern
            word_a = torch.tensor(list(pattern_bytes('A', b.dtype)), dtype=torch.uint8, device=dev).repeat(b.numel)
            word_b = torch.tensor(list(pattern_bytes('B', b.dtype)), dtype=torch.uint8, device=dev).repeat(b.numel)
            ok = (a_bits == b_bits) | ((a_bits == word_a) & (b_bits == word_b))
            assert bool(ok.all()), f'{b.name}: {int((~ok).sum())} of {b.nbytes} bytes differ between the runs, first at ' \
                                   f'{int(torch.nonzero(~ok)[0, 0])}'
            print(f'  {b.name}: {int((a_bits != word_a).sum())} of {b.nbytes} bytes written')
        elif not exempt:
            differ = (a_bits != b_bits).view(b.numel, b.itemsize).any(1)
            assert not bool(differ.any()), f'{b.name}: {int(differ.sum())} of {b.numel} elements depend on what the guards, outputs ' \
                                           f'or workspaces held before the call, first at {int(torch.nonzero(differ)[0, 0])}'
        else:
            case.tolerance(b.name, b_bits.view(b.dtype), want[b.name].to(dev))

    # ---- the workspace bound ---------------------------------------------------------------------------------------------------
    if case.ws_index is not None:
        nbytes = case.args[case.ws_index]
        assert nbytes > 0
        for b in arena.tagged(INOUT):
            b.bytes.copy_(initial[b.name])
        arena.fill_guards('A')
        arena.fill_payload('A', (OUT, WORKSPACE))
        before = arena.payload_bits()
        status = _call(case, dev, {case.ws_index: nbytes - 1})
        assert status == E_WORKSPACE, f'a workspace of {nbytes - 1} bytes (one short): status {status}'
        _check_guards(case, 'workspace one byte short')
        _untouched(case, before, 'workspace one byte short')

    # ---- documented rejections -------------------------------------------------------------------------------------------------
    for overrides, expect in case.rejections:
        for b in arena.tagged(INOUT):
            b.bytes.copy_(initial[b.name])
        arena.fill_guards('A')
        arena.fill_payload('A', (OUT, WORKSPACE))
        before = arena.payload_bits()
        status = _call(case, dev, overrides)
        assert status == expect, f'arguments {overrides}: status {status}, the header documents {expect}'
        _check_guards(case, f'refused call {overrides}')
        _untouched(case, before, f'refused call {overrides}')

    # ---- the empty call --------------------------------------------------------------------------------------------------------
    if case.empty is not None:
        for b in arena.tagged(INOUT):
            b.bytes.copy_(initial[b.name])
        arena.fill_guards('A')
        arena.fill_payload('A', (OUT, WORKSPACE))
        before = arena.payload_bits()
        status = _call(case, dev, case.empty)
        assert status == 0, f'empty call: status {status}'
        _check_guards(case, 'empty call')
        effect = case.empty_effect() if case.empty_effect else {}
        _untouched(case, before, 'empty call', but=effect)
        for k, w in effect.items():
            assert torch.equal(arena[k].bytes, _bytes_of(w).to(dev)), f'empty call: {k} does not hold the documented effect'
