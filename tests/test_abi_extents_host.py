"""The case table of tests/test_gpu_abi_extents.py and its guarded arena, checked without a GPU: every exported symbol has a
case (or a stated reason to have none), every case builds on the CPU with tagged, sized pointer arguments in the order of the
binding's signature, and the arena reports writes outside a payload where they happen."""
import ctypes

import pytest
import torch

import abi_arena as aa
import abi_cases as ac
from sunerf_hip import lib

PAIRS = [(name, shape) for name, (_, shapes) in ac.CASES.items() for shape in shapes]
POINTER = ctypes.c_void_p
INTEGERS = (ctypes.c_int, ctypes.c_int64, ctypes.c_uint64, ctypes.c_size_t)
FLOATS = (ctypes.c_float, ctypes.c_double)


def test_every_exported_symbol_has_a_case_or_a_reason():
    cases, none = set(ac.CASES), set(ac.NO_DEVICE_ACCESS)
    assert not cases & none, sorted(cases & none)
    exported = set(lib.symbols('core'))
    assert cases | none == exported, (sorted(exported - cases - none), sorted((cases | none) - exported))
    assert all(isinstance(r, str) and r for r in ac.NO_DEVICE_ACCESS.values())
    assert all(ac.TILES[name] for name in cases)
    assert all(len(shapes) == len(set(shapes)) and shapes for _, shapes in ac.CASES.values())


@pytest.mark.parametrize('name', sorted(ac.CASES))
def test_cases_build_on_the_cpu_with_tagged_sized_arguments(name):
    builder, shapes = ac.CASES[name]
    argtypes = lib.signature(name)[1]
    for shape in shapes:
        case = builder(shape, 'cpu')
        assert case.name == name and len(case.args) == len(argtypes), (shape, len(case.args), len(argtypes))
        assert case.args[-1] == ac.STREAM
        seen = set()
        for i, (arg, ctype) in enumerate(zip(case.args[:-1], argtypes[:-1])):
            where = f'{name} {shape} argument {i}'
            if isinstance(arg, (aa.Buffer, aa.Absent)):
                assert ctype is POINTER, where
                assert arg.tag in aa.TAGS, where
                assert arg.name not in seen, where
                seen.add(arg.name)
                if isinstance(arg, aa.Buffer):
                    assert arg.numel > 0, f'{where}: {arg.name} has no elements (an absent optional argument is Absent)'
                    assert arg in case.arena.buffers, where
            elif isinstance(arg, ac.HostPtrs):
                assert ctype is ctypes.POINTER(ctypes.c_void_p), where
                assert all(isinstance(b, aa.Buffer) and b.numel > 0 and b in case.arena.buffers for b in arg.buffers), where
            elif isinstance(arg, ac.HostValue):
                assert ctype not in INTEGERS + FLOATS, where
            elif arg is None:
                assert ctype is ctypes.POINTER(ctypes.c_void_p), f'{where}: a NULL device pointer is an Absent with a tag'
            elif ctype in INTEGERS:
                assert isinstance(arg, int) and not isinstance(arg, bool), (where, arg)
            else:
                assert ctype in FLOATS and isinstance(arg, (int, float)), (where, arg, ctype)
        assert len(case.ctypes_args(None)) == len(argtypes)
        for b in case.arena.buffers:
            assert b.guard_bytes >= aa.MIN_GUARD_BYTES
        if case.ws_index is not None:
            assert argtypes[case.ws_index] is ctypes.c_size_t and case.args[case.ws_index] > 0, (name, shape)
            assert isinstance(case.args[case.ws_index - 1], aa.Buffer) and case.args[case.ws_index - 1].tag == aa.WORKSPACE
            assert case.args[case.ws_index - 1].numel == case.args[case.ws_index], 'the workspace is exactly the size its query returns'
        for i in (case.empty or {}):
            assert argtypes[i] in INTEGERS
        assert case.opaque <= {b.name for b in case.arena.tagged(aa.OUT)}
        for overrides, status in case.rejections:
            assert status < 0 and all(argtypes[i] in INTEGERS for i in overrides)


# ---- the arena itself -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8])
@pytest.mark.parametrize('offset', [0, 1, 3])
def test_arena_reports_writes_on_either_side_of_a_payload(dtype, offset):
    arena = aa.Arena('cpu')
    other = arena.alloc('other', aa.IN, torch.float32, 5, data=torch.arange(5.))
    buf = arena.alloc('buf', aa.OUT, dtype, 37, offset=offset)
    item = buf.itemsize
    assert buf.guard_bytes >= 1 << 20 and buf.front.numel() == buf.back.numel() == buf.guard_bytes
    assert (buf.t.data_ptr() - offset * item) % aa.ALIGN == 0 and buf.ptr.value == buf.t.data_ptr()
    assert buf.front.data_ptr() + buf.guard_bytes == buf.t.data_ptr() and buf.back.data_ptr() == buf.t.data_ptr() + 37 * item
    for pattern in aa.PATTERNS:
        arena.fill_guards(pattern)
        arena.fill_payload(pattern)
        ok, report = arena.guards_intact()
        assert ok and report['buf'] == {'front': (0, None), 'back': (0, None)}
        assert buf.holds_pattern(pattern) == 37 and bytes(buf.payload_bits()[:item].tolist()) == aa.pattern_bytes(pattern, dtype)
        assert torch.equal(other.t, torch.arange(5.)), 'fill_payload leaves inputs alone'
        if dtype.is_floating_point:
            assert bool(torch.isnan(buf.t).all()) if pattern == 'B' else bool((buf.t == -12345.0).all())
        # payload index -1: the last word of the front guard
        whole = buf._storage[buf._start - item:buf._start]
        saved = whole.clone()
        whole[0] ^= 0x01
        ok, report = arena.guards_intact()
        assert not ok and report['buf'] == {'front': (1, -1), 'back': (0, None)} and report['other']['front'] == (0, None)
        whole.copy_(saved)
        # payload index numel (+ 2): words of the back guard
        end = buf._start + 37 * item
        buf._storage[end + item - 1] ^= 0x80
        buf._storage[end + 2 * item] ^= 0x10
        ok, report = arena.guards_intact()
        assert not ok and report['buf'] == {'front': (0, None), 'back': (2, 37)}
        assert any('buf' in line and 'touched 0 / 2' in line and 'first at 37' in line for line in arena.lines(report))
        arena.fill_guards(pattern)
        assert arena.guards_intact()[0]
        # a write inside the payload is no guard hit, and shows in payload_bits
        before = buf.payload_bits()
        buf.t[36] = 1
        assert arena.guards_intact()[0] and not torch.equal(before, buf.payload_bits()) and buf.holds_pattern(pattern) == 36


def test_arena_payload_bits_is_a_copy_and_inputs_keep_their_data():
    arena = aa.Arena('cpu')
    data = torch.tensor([1.5, float('nan'), -0.0, float('inf')])
    buf = arena.alloc('x', aa.INOUT, torch.float32, 4, data=data)
    bits = buf.payload_bits()
    assert bits.dtype == torch.uint8 and bits.numel() == 16 and torch.equal(bits.view(torch.float32)[[0, 3]], data[[0, 3]])
    buf.t[0] = 2.0
    assert bits.view(torch.float32)[0] == 1.5
    arena.fill_payload('B')                        # OUT and WORKSPACE only
    assert buf.t[0] == 2.0
    ws = arena.alloc('ws', aa.WORKSPACE, torch.uint8, 300, init='zero')
    head = arena.alloc('head', aa.WORKSPACE, torch.uint8, 300, init='zero_head:256')
    arena.fill_payload('A')
    assert not ws.bytes.any() and not head.bytes[:256].any() and bool((head.bytes[256:] == 0x5a).all())
    assert torch.equal(buf.plain(2, 2).reshape(-1)[2:], buf.t[2:]) and buf.plain().data_ptr() != buf.t.data_ptr()
    absent = aa.Absent('optional', aa.OUT)
    assert absent.ptr is None and absent.numel == 0
    with pytest.raises(AssertionError):
        arena.alloc('x', aa.IN, torch.float32, 1)
