"""A guarded arena for calls through the C ABI (include/sunerf_hip.h): every buffer an entry point is handed sits in the middle
of an allocation of its own, between a front guard and a back guard that hold a known pattern.  A kernel that writes outside
the extent the header states shows up as changed guard words; a kernel that reads outside it, or that depends on what an
output or a workspace held before the call, shows up as a difference between two runs whose guards and outputs held different
patterns.  Plain torch: every ``device`` works, 'cpu' included (tests/test_abi_extents_host.py exercises the arena there).

Patterns (per element type, so that a guard word reads as one element of the buffer's own type):

* ``'A'``: a finite sentinel no kernel produces -- the float -12345.0 (bits 0xC640E400; as fp64 for fp64 buffers, the fp32 word
  twice for int64, once for int32) and 0x5A bytes for byte buffers;
* ``'B'``: quiet NaNs for the float types (0x7FC00000, 0x7FF8000000000000), 0xFF bytes for everything else.
"""
import ctypes
import struct

import torch

IN, OUT, INOUT, WORKSPACE = 'IN', 'OUT', 'INOUT', 'WORKSPACE'
TAGS = (IN, OUT, INOUT, WORKSPACE)
MIN_GUARD_BYTES = 1 << 20        # per side
ALIGN = 256                      # the caching allocator's alignment: the default start of a payload

_F32_A = struct.pack('<f', -12345.0)
_PATTERN_BYTES = {
    'A': {torch.float32: _F32_A, torch.float64: struct.pack('<d', -12345.0), torch.int32: _F32_A, torch.int64: _F32_A * 2,
          torch.uint8: b'\x5a'},
    'B': {torch.float32: struct.pack('<I', 0x7FC00000), torch.float64: struct.pack('<Q', 0x7FF8000000000000),
          torch.int32: b'\xff' * 4, torch.int64: b'\xff' * 8, torch.uint8: b'\xff'},
}
PATTERNS = tuple(_PATTERN_BYTES)


def pattern_bytes(pattern: str, dtype) -> bytes:
    """The bytes of one element of ``dtype`` in ``pattern``."""
    return _PATTERN_BYTES[pattern][dtype]


def _round_up(x: int, m: int) -> int:
    return -(-x // m) * m


class Buffer:
    """One argument of a call: ``numel`` elements of ``dtype`` (the payload, ``.t``) with ``guard_bytes`` on either side."""

    def __init__(self, device, name, tag, dtype, numel, guard_bytes=None, offset=0, init=None):
        assert tag in TAGS, tag
        assert numel >= 0 and offset >= 0
        self.name, self.tag, self.dtype, self.numel, self.offset = name, tag, dtype, int(numel), int(offset)
        self.itemsize = torch.empty(0, dtype=dtype).element_size()
        # 'zero': a workspace the header wants zeroed by the caller (never given a pattern); 'zero_head:N': its first N bytes only
        self.init = init
        self.guard_bytes = _round_up(max(MIN_GUARD_BYTES, int(guard_bytes or 0)), ALIGN)
        self.nbytes = self.numel * self.itemsize
        skew = self.offset * self.itemsize
        self._storage = torch.empty(self.guard_bytes + skew + self.nbytes + self.guard_bytes + ALIGN, dtype=torch.uint8, device=device)
        base = self._storage.data_ptr()
        start = _round_up(base + self.guard_bytes, ALIGN) - base + skew          # byte offset of the payload
        self._start = start
        self.front = self._storage[start - self.guard_bytes:start]
        self.back = self._storage[start + self.nbytes:start + self.nbytes + self.guard_bytes]
        self.bytes = self._storage[start:start + self.nbytes]
        # a payload that is offset by an odd number of elements may be misaligned for its own type only when the offset in bytes
        # is no multiple of the item size, which cannot happen: the typed view below is always legal
        self.t = self.bytes.view(dtype) if self.numel else torch.empty(0, dtype=dtype, device=device)
        assert self.t.numel() == self.numel
        assert self.numel == 0 or (self.t.data_ptr() - skew) % ALIGN == 0

    @property
    def ptr(self):
        return ctypes.c_void_p(self.bytes.data_ptr() if self.numel else self._storage.data_ptr() + self._start)

    def set(self, data) -> 'Buffer':
        """Copies ``data`` (a tensor or array of ``numel`` elements of the buffer's type) into the payload."""
        data = torch.as_tensor(data)
        assert data.numel() == self.numel, (self.name, data.numel(), self.numel)
        assert data.dtype == self.dtype, (self.name, data.dtype, self.dtype)
        self.t.copy_(data.reshape(-1))
        return self

    def plain(self, *shape):
        """An ordinary tensor (a fresh allocation) holding the payload, reshaped."""
        t = self.t.clone()
        return t.reshape(*shape) if shape else t

    def _tile(self, pattern, nbytes):
        word = pattern_bytes(pattern, self.dtype)
        assert nbytes % len(word) == 0
        return torch.tensor(list(word), dtype=torch.uint8, device=self._storage.device).repeat(nbytes // len(word))

    def fill_guards(self, pattern):
        tile = self._tile(pattern, self.guard_bytes)
        self.front.copy_(tile)
        self.back.copy_(tile)
        self._guard_pattern = pattern

    def fill_payload(self, pattern):
        if self.init == 'zero':
            self.bytes.zero_()
        elif self.numel:
            self.bytes.copy_(self._tile(pattern, self.nbytes))
            if self.init and self.init.startswith('zero_head:'):
                self.bytes[:int(self.init.split(':')[1])].zero_()

    def payload_bits(self):
        """A copy of the payload as bytes: what bit-for-bit comparisons are made on."""
        return self.bytes.clone()

    def holds_pattern(self, pattern):
        """Number of whole elements of the payload that hold ``pattern``'s element."""
        if not self.numel:
            return 0
        same = (self.bytes == self._tile(pattern, self.nbytes)).view(self.numel, self.itemsize).all(1)
        return int(same.sum())

    def guard_hits(self):
        """``dict(front=(words, first), back=(words, first))``: the number of guard words (elements of the buffer's type) that
        no longer hold the pattern, and the payload index of the first of them (negative in the front guard, >= numel in the
        back guard; None when there is none)."""
        tile = self._tile(self._guard_pattern, self.guard_bytes)
        report = {}
        for side, guard in (('front', self.front), ('back', self.back)):
            bad = (guard != tile).view(-1, self.itemsize).any(1)
            count = int(bad.sum())
            first = None
            if count:
                word = int(torch.nonzero(bad)[0, 0])
                first = word - self.guard_bytes // self.itemsize if side == 'front' else self.numel + word
            report[side] = (count, first)
        return report


class Absent:
    """An optional pointer argument that this case passes as NULL."""
    numel = 0

    def __init__(self, name, tag):
        assert tag in TAGS
        self.name, self.tag = name, tag
    ptr = None


class Arena:
    def __init__(self, device):
        self.device = torch.device(device)
        self.buffers = []

    def alloc(self, name, tag, dtype, numel, data=None, guard_bytes=None, offset=0, init=None) -> Buffer:
        assert all(b.name != name for b in self.buffers), f'two buffers called {name}'
        buf = Buffer(self.device, name, tag, dtype, numel, guard_bytes, offset, init)
        self.buffers.append(buf)
        if data is not None:
            buf.set(data)
        elif tag in (IN, INOUT):
            buf.bytes.zero_()
        return buf

    def __getitem__(self, name) -> Buffer:
        return next(b for b in self.buffers if b.name == name)

    def tagged(self, *tags):
        return [b for b in self.buffers if b.tag in tags]

    def fill_guards(self, pattern):
        for b in self.buffers:
            b.fill_guards(pattern)

    def fill_payload(self, pattern, tags=(OUT, WORKSPACE)):
        for b in self.tagged(*tags):
            b.fill_payload(pattern)

    def guards_intact(self):
        """``(ok, report)``: report[name] = ``Buffer.guard_hits()`` of every buffer, compared by bits on the device."""
        report = {b.name: b.guard_hits() for b in self.buffers}
        ok = all(count == 0 for r in report.values() for count, _ in r.values())
        return ok, report

    def payload_bits(self, *tags):
        return {b.name: b.payload_bits() for b in (self.tagged(*tags) if tags else self.buffers)}

    def lines(self, report):
        """One line per buffer: name, tag, elements, guard words touched (front / back)."""
        out = []
        for b in self.buffers:
            (f, f0), (k, k0) = report[b.name]['front'], report[b.name]['back']
            where = '' if not (f or k) else f'  first at {f0 if f else k0}'
            out.append(f'  {b.name:<24s} {b.tag:<9s} {b.numel:>10d} x {str(b.dtype)[6:]:<8s} guard {b.guard_bytes >> 10} KiB  touched {f} / {k}{where}')
        return out
