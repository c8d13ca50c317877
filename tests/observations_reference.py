"""Numpy restatement of the training-set builder (``csrc/observations.hip``, ``include/sunerf_hip.h``): the keyed permutation,
the pixel decode, the block mean and the channel fill, integer for integer and bit for bit.  numpy only; not a test module."""
import numpy as np

_M32 = np.uint64(0xffffffff)


def fmix32(h):
    """murmur3 finaliser on uint32 values carried in uint64 arrays."""
    h = np.asarray(h, dtype=np.uint64) & _M32
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85ebca6b)) & _M32
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xc2b2ae35)) & _M32
    return h ^ (h >> np.uint64(16))


def round_keys(seed: int, epoch: int):
    seed, epoch = int(seed) & (2 ** 64 - 1), int(epoch) & (2 ** 64 - 1)
    s = (seed & 0xffffffff) ^ int(fmix32(((seed >> 32) + 0x9e3779b9) & 0xffffffff))
    e = (epoch & 0xffffffff) ^ int(fmix32(((epoch >> 32) + 0x9e3779b9) & 0xffffffff))
    keys = []
    for r in range(4):
        inner = int(fmix32((e + 0x85ebca6b * (r + 1)) & 0xffffffff))
        keys.append(int(fmix32(((s + 0x9e3779b9 * (r + 1)) & 0xffffffff) ^ inner)))
    return keys


def half_bits(n_valid: int) -> int:
    return (int(n_valid - 1).bit_length() + 1) // 2


def permutation(slots, n_valid: int, seed: int, epoch: int, max_rounds: int = 100000):
    """pi(slots): cycle-walking over a 4-round balanced Feistel network on 2 b bits."""
    assert 1 <= n_valid < 2 ** 40
    b = np.uint64(half_bits(n_valid))
    mask = np.uint64((1 << int(b)) - 1)
    keys = [np.uint64(k) for k in round_keys(seed, epoch)]
    x = np.array(slots, dtype=np.uint64, copy=True).reshape(-1)
    assert x.size == 0 or int(x.max()) < n_valid
    todo = np.arange(x.size)
    rounds = 0
    while todo.size:
        v = x[todo]
        left, right = v >> b, v & mask
        for k in keys:
            left, right = right, left ^ (fmix32((right + k) & _M32) & mask)
        v = (left << b) | right
        x[todo] = v
        todo = todo[v >= np.uint64(n_valid)]
        rounds += 1
        assert rounds < max_rounds
    return x.astype(np.int64)


def shard_range(n_items: int, rank: int, world: int):
    base, rem = divmod(n_items, world)
    begin = rank * base + min(rank, rem)
    return begin, begin + base + (1 if rank < rem else 0)


def decode(pixels, shapes):
    """Global pixel numbers -> (view, row, col) for views of ``shapes`` [(H, W), ...] concatenated in order, row-major."""
    pixels = np.asarray(pixels, dtype=np.int64)
    sizes = np.array([h * w for h, w in shapes], dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(sizes)])
    view = np.searchsorted(offsets, pixels, side='right') - 1
    local = pixels - offsets[view]
    widths = np.array([w for _, w in shapes], dtype=np.int64)[view]
    return view, local // widths, local % widths


def block_mean(plane: np.ndarray, f: int) -> np.ndarray:
    """Mean of the f x f blocks of a (H, W) fp32 plane: fp64 sum in row-major order, / (f f), rounded to fp32 once."""
    plane = np.asarray(plane, dtype=np.float32)
    if f == 1:
        return plane.copy()
    assert plane.shape[0] % f == 0 and plane.shape[1] % f == 0
    total = np.zeros((plane.shape[0] // f, plane.shape[1] // f), dtype=np.float64)
    for y in range(f):
        for x in range(f):
            total = total + plane[y::f, x::f].astype(np.float64)
    return (total / np.float64(f * f)).astype(np.float32)


def channel_fill(planes: np.ndarray, wavelengths, f: int):
    """(target (n, C), wavelength (n, C), valid (n,)) of one view: ``planes`` (C_present, H, W) are the non-zero entries of
    ``wavelengths`` in order; absent channels are target 0 / wavelength 0; valid = every present block mean finite."""
    wl = np.asarray(wavelengths, dtype=np.float32).reshape(-1)
    reduced = [block_mean(p, f) for p in planes]
    n = reduced[0].size
    target = np.zeros((n, wl.size), dtype=np.float32)
    k = 0
    for c in range(wl.size):
        if wl[c] != 0:
            target[:, c] = reduced[k].reshape(-1)
            k += 1
    assert k == len(reduced)
    valid = np.all([np.isfinite(r.reshape(-1)) for r in reduced], axis=0)
    return target, np.broadcast_to(wl, (n, wl.size)).copy(), valid


def assemble(views, n_slots_range, seed: int, epoch: int, drop_nonfinite: bool = True, permute: bool = True):
    """The pool arrays of slots ``n_slots_range`` = (begin, end) or None (all).  ``views``: dicts with ``planes``
    (C_present, H f, W f), ``wavelengths`` (C,), ``downscale``, ``time``, ``rays_o`` / ``rays_d`` (H W, 3) in pixel order."""
    rays, time, target, wavelength, valid = [], [], [], [], []
    for v in views:
        t, w, ok = channel_fill(v['planes'], v['wavelengths'], v['downscale'])
        n = t.shape[0]
        assert v['rays_o'].shape == (n, 3) and v['rays_d'].shape == (n, 3)
        rays.append(np.stack([v['rays_o'], v['rays_d']], 1).astype(np.float32))
        time.append(np.full((n, 1), np.float32(v['time']), dtype=np.float32))
        target.append(t), wavelength.append(w), valid.append(ok)
    rays, time, target, wavelength = (np.concatenate(a) for a in (rays, time, target, wavelength))
    valid = np.concatenate(valid)
    index = np.nonzero(valid)[0] if drop_nonfinite and not valid.all() else np.arange(valid.size)
    begin, end = (0, index.size) if n_slots_range is None else n_slots_range
    slots = np.arange(begin, end)
    q = permutation(slots, index.size, seed, epoch) if permute else slots
    p = index[q]
    return {'rays': rays[p], 'time': time[p], 'target_image': target[p], 'wavelength': wavelength[p], 'pixels': p,
            'n_valid': index.size}
