"""fp64 NumPy restatement of include/sunerf_hip_patch.h's adjoint, exactly as the header words it (the order of every operation
included; NumPy never fuses a multiply with an add), of the extended sub-pixel axes and of the patch lattice of
sunerf_hip/patch.py, for tests/test_patch_host.py and the GPU tests of the patch table.

The adjoint is written in the scatter form -- for every tap (i, j) in the header's order, ``np.add.at`` of ``K[i, j] * g_out`` onto
the clamped (NEAREST) or masked (ZERO) indices, the index arrays flattened in C order -- so that an input pixel receives its terms
i ascending, inside it j ascending, inside it R ascending, inside it C ascending: ``np.add.at`` adds unbuffered, element by element,
in the order of its index arrays.  The kernel is written in the gather form; the two agree by bits or one of them is wrong."""
import numpy as np

# (planes, H, W, kh, kw, bin, anchor, per-plane K): the cases of the issue, every one for both boundaries
ADJOINT_CASES = [
    (1, 5, 7, 1, 1, 1, (0, 0), False),
    (2, 9, 11, 3, 5, 1, (1, 2), True),
    (1, 9, 11, 4, 2, 2, (0, 0), False),
    (1, 9, 11, 4, 2, 2, (3, 1), False),
    (3, 13, 10, 5, 5, 3, (2, 2), True),
    (1, 2, 3, 7, 7, 1, (3, 3), False),          # the plane is smaller than the kernel: every tap clamps
    (1, 70, 67, 9, 9, 2, (4, 4), False),
    (1, 40, 40, 96, 96, 8, (48, 48), False),
    (2, 67, 35, 6, 6, 2, (2, 2), False),
]
# tile seams of the adjoint kernel (SUNERF_PATCH_TILE = 32 input pixels): exactly one tile; a partial last tile in both axes
SEAM_CASES = [
    (1, 32, 32, 5, 5, 2, (2, 2), False),
    (2, 45, 71, 7, 5, 3, (3, 1), True),
]
BOUNDARIES = ('zero', 'nearest')


def case_data(case, seed=0):
    """(K [1 or P, kh, kw] fp64, x [P, H, W] fp32, g [P, H // b, W // b] fp32) of a case: values of both signs and of several
    magnitudes, so that a wrong order of the sum shows in the last bits."""
    planes, h, w, kh, kw, b, _, per_plane = case
    rng = np.random.default_rng([seed, planes, h, w, kh, kw, b])
    K = rng.uniform(-1.0, 1.0, size=(planes if per_plane else 1, kh, kw)) * 10.0 ** rng.integers(-2, 2, size=(1, kh, kw))
    x = (rng.uniform(-1.0, 1.0, size=(planes, h, w)) * 10.0 ** rng.integers(-2, 3, size=(planes, h, w))).astype(np.float32)
    g = (rng.uniform(-1.0, 1.0, size=(planes, h // b, w // b)) * 10.0 ** rng.integers(-2, 3, size=(planes, h // b, w // b))).astype(np.float32)
    return K, x, g


def correlate_bin_adjoint(g_out, K, height, width, bin_factor, anchor, scale=1.0, boundary='zero'):
    """The header's sunerf_patch_correlate_bin_adjoint: (g_in [P, height, width] fp32, the fp64 sum before scale)."""
    g = np.asarray(g_out, dtype=np.float32).astype(np.float64)
    K = np.asarray(K, dtype=np.float64)
    K = K[None] if K.ndim == 2 else K
    p_, oh, ow = g.shape
    b = int(bin_factor)
    assert (oh, ow) == (height // b, width // b)
    kh, kw = K.shape[1:]
    ay, ax = anchor
    rows = np.arange(oh) * b - ay
    cols = np.arange(ow) * b - ax
    acc = np.zeros((p_, height, width))
    with np.errstate(all='ignore'):
        for i in range(kh):
            y = rows + i
            for j in range(kw):
                xx = cols + j
                yy, xg = np.meshgrid(y, xx, indexing='ij')          # [oh, ow]: C order is R ascending, inside it C ascending
                if boundary == 'nearest':
                    keep = np.ones(yy.shape, dtype=bool)
                    yy, xg = np.clip(yy, 0, height - 1), np.clip(xg, 0, width - 1)
                else:
                    keep = (yy >= 0) & (yy < height) & (xg >= 0) & (xg < width)
                keep = keep.reshape(-1)
                iy, ix = yy.reshape(-1)[keep], xg.reshape(-1)[keep]
                for p in range(p_):
                    wgt = K[p if K.shape[0] > 1 else 0, i, j]
                    np.add.at(acc[p], (iy, ix), (wgt * g[p]).reshape(-1)[keep])
        return (scale * acc).astype(np.float32), acc


def extended_axis(axis, bin_factor, k_eff, anchor):
    """Entry m: the angle of sub-pixel m - anchor of the frame, fp64, rounded to fp32 once."""
    axis = np.asarray(axis, dtype=np.float64)
    n = axis.shape[0]
    t0 = axis[0]
    delta = (axis[-1] - axis[0]) / (n - 1)
    out = np.empty((n - 1) * bin_factor + k_eff, dtype=np.float32)
    for m in range(out.shape[0]):
        q = m - anchor
        c = q // bin_factor          # floor: c may be negative
        s = q - c * bin_factor
        out[m] = np.float32(t0 + (float(c) + (float(s) + 0.5) / bin_factor - 0.5) * delta)
    return out


def lattice(n, patch):
    starts = [k * patch for k in range(n // patch)]
    if n % patch:
        starts.append(n - patch)
    return starts
