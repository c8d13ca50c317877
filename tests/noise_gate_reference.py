"""NumPy fp64 restatement of noise gating, written from include/sunerf_hip_noise_gate.h: explicit blocks, ``np.fft.fftn`` on each,
the factors, the inverse and the overlap-add -- block by block in plain Python: this is the specification, not a fast path.

Beside the result it reports what the comparison with the fp32 kernel needs ("the bound"): per block the sum
``A = sum |W I|``, per coefficient the clearance ``| |F_k|^2 - T_k |`` against the error a forward fp32 transform can make there,
and per output sample the bound on the difference."""
import numpy as np

GATE, WIENER = 0, 1
FILL_INVALID = 1
BLOCK = 16
BLOCK_T = (1, 4, 8, 16)
U = 2.0 ** -24          # unit roundoff of fp32
# Roundings a coefficient passes on the way forward, each as a relative perturbation of at most c u of everything that flows into
# it: the window and the fill 3; x: three butterfly levels 3, one level of twiddle products 3.24, the split of the
# real line 5.24; y and t: four butterfly levels 4 and two levels of twiddle products 6.48 each -- 35.4, rounded up.
C_FORWARD = 40.0
# ... and back: t and y 10.48 each, x 11.48, the factor 4, the window and the scale 3 -- 39.4, rounded up.
C_INVERSE = 44.0


def window(n):
    return np.ones(1) if n == 1 else np.sin(np.pi * (np.arange(n) + 0.5) / n) ** 2


def stride(n):
    return 1 if n == 1 else n // 4


def origins(n, size):
    """Where the blocks of ``size`` samples begin along an axis of ``n`` samples."""
    s = stride(size)
    return list(range(-(size - s), n, s))


def fold(i, n):
    """NumPy's ``symmetric`` padding as an index map, for any integer ``i`` and ``n >= 1``."""
    m = np.mod(i, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def canonical(bt):
    """For every coefficient (k_t, k_y, k_x) of a ``bt x 16 x 16`` block the flat index of the one whose power and spectrum
    decide its factor: itself at 0 < k_x < 8, -k at k_x > 8, and at k_x = 0 or 8 whichever of k and -k has the smaller
    (k_t, k_y) in row-major order."""
    kt, ky, kx = np.meshgrid(np.arange(bt), np.arange(16), np.arange(16), indexing='ij')
    mt, my, mx = (-kt) % bt, (-ky) % 16, (-kx) % 16
    own, other = (kt * 16 + ky) * 16 + kx, (mt * 16 + my) * 16 + mx
    swap = (kx > 8) | (((kx == 0) | (kx == 8)) & (mt * 16 + my < kt * 16 + ky))
    return np.where(swap, other, own).reshape(-1)


def noise_gate(frames, bad=None, params=None, spectrum=None, bt=8, mode=GATE, gamma=None, flags=0, detail=False):
    """``frames`` [T, C, H, W] (float32 values), ``bad`` of that shape or None, ``params`` [C, 4] = a, b, 0, 0, ``spectrum``
    [C, bt, 16, 16] or None.  Returns ``(out, state)``: fp64 [T, C, H, W] and int64 [C, 4]; with ``detail`` a dict as third item:
    ``bound`` (per sample, on |fp32 kernel - out|), ``excluded`` (bool per sample: inside a block that holds an undecidable
    coefficient), ``undecidable`` (per plane, the number of such coefficients), ``min_clearance`` (the smallest clearance relative
    to the error allowed there, over all non-DC coefficients), ``blocks``, and for the statistics of the rule ``interior_blocks``
    (the blocks that read no folded sample) with ``interior_kept``, their coefficients with k != -k and a factor above 0."""
    assert bt in BLOCK_T and mode in (GATE, WIENER)
    gamma = (3.0 if mode == GATE else 1.0) if gamma is None else float(gamma)
    x = np.asarray(frames, dtype=np.float64)
    n_t, n_c, n_h, n_w = x.shape
    valid_all = np.isfinite(x) if bad is None else np.isfinite(x) & (np.asarray(bad) == 0)
    params = np.zeros((n_c, 4)) if params is None else np.asarray(params, dtype=np.float64)
    wt, wy = window(bt), window(BLOCK)
    w = wt[:, None, None] * wy[None, :, None] * wy[None, None, :]
    axes = 3 if bt > 1 else 2
    norm = 1.5 ** axes
    n_coef = bt * BLOCK * BLOCK
    canon = canonical(bt)
    g2 = gamma * gamma
    out = np.zeros(x.shape)
    state = np.zeros((n_c, 4), dtype=np.int64)
    bound = np.zeros(x.shape)
    absum = np.zeros(x.shape)
    excluded = np.zeros(x.shape, dtype=bool)
    undecidable = np.zeros(n_c, dtype=np.int64)
    min_clearance = np.inf
    n_blocks = 0
    lipschitz = 1.0 if mode == GATE else 2.0
    paired = canonical(bt) != np.arange(n_coef)          # k > -k ...
    paired[canon[paired]] = True                         # ... and its partner: every k != -k
    interior_blocks = interior_kept = 0
    for c in range(n_c):
        state[c, 0] = int((~valid_all[:, c]).sum())
        s_c = np.ones(n_coef) if spectrum is None else np.asarray(spectrum, dtype=np.float64)[c].reshape(-1)[canon]
        a, b = params[c, 0], params[c, 1]
        for t0 in origins(n_t, bt):
            pt = t0 + np.arange(bt)
            for y0 in origins(n_h, BLOCK):
                py = y0 + np.arange(BLOCK)
                for x0 in origins(n_w, BLOCK):
                    px = x0 + np.arange(BLOCK)
                    n_blocks += 1
                    idx = np.ix_(fold(pt, n_t), [c], fold(py, n_h), fold(px, n_w))
                    block, valid = x[idx][:, 0], valid_all[idx][:, 0]
                    if not valid.any():
                        continue
                    mean = np.float64(np.float32(block[valid].mean()))
                    filled = np.where(valid, block, mean)
                    spec = np.fft.fftn(w * filled)
                    power = float(np.sum((w * w * (a + b * np.maximum(filled, 0.0)))[valid]))
                    thr = (g2 * power) * s_c
                    mag = (np.abs(spec) ** 2).reshape(-1)[canon]
                    if mode == GATE:
                        factor = (mag >= thr).astype(np.float64)
                    else:
                        with np.errstate(divide='ignore', invalid='ignore'):
                            factor = np.where(mag > 0, np.maximum(0.0, 1.0 - thr / mag), 0.0)
                    factor[0] = 1.0
                    gated = factor.reshape(spec.shape) * spec
                    part = w * np.fft.ifftn(gated).real / norm
                    state[c, 1] += 1
                    state[c, 2] += int((factor[1:] > 0).sum())
                    state[c, 3] += n_coef - 1
                    inside = np.ix_((pt >= 0) & (pt < n_t), (py >= 0) & (py < n_h), (px >= 0) & (px < n_w))
                    where = np.ix_(pt[(pt >= 0) & (pt < n_t)], [c], py[(py >= 0) & (py < n_h)], px[(px >= 0) & (px < n_w)])
                    out[where] += part[inside][:, None]
                    if detail:
                        if t0 >= 0 and t0 + bt <= n_t and y0 >= 0 and y0 + BLOCK <= n_h and x0 >= 0 and x0 + BLOCK <= n_w:
                            interior_blocks += 1
                            interior_kept += int((factor[paired] > 0).sum())
                        total = float(np.abs(w * filled).sum())
                        e_f = C_FORWARD * U * total
                        allowed = 2.0 * np.sqrt(mag) * e_f + e_f * e_f + 1e-12 * thr
                        if mode == GATE:          # |F|^2 >= 0 holds whatever the error
                            allowed = np.where(thr > 0, allowed, 0.0)
                        clear = np.abs(mag - thr)
                        with np.errstate(divide='ignore', invalid='ignore'):
                            ratio = np.where(allowed[1:] > 0, clear[1:] / allowed[1:], np.inf)
                        min_clearance = min(min_clearance, float(ratio.min()))
                        n_bad = int((clear[1:] < allowed[1:]).sum())
                        undecidable[c] += n_bad
                        e_b = w / norm * (lipschitz * e_f + C_INVERSE * U * float(np.abs(gated).sum()) / n_coef)
                        bound[where] += e_b[inside][:, None]
                        absum[where] += np.abs(part[inside])[:, None]
                        if n_bad:
                            hit = np.zeros(part.shape, dtype=bool)
                            hit[inside] = True
                            excluded[where] |= hit[inside][:, None]
    result = out.copy()
    if not flags & FILL_INVALID:
        result[~valid_all] = np.nan
    if not detail:
        return result, state
    cover = 4 ** axes
    bound = bound + (cover + 2) * U * absum
    return result, state, dict(bound=bound, excluded=excluded, undecidable=undecidable, min_clearance=min_clearance, blocks=n_blocks,
                               interior_blocks=interior_blocks, interior_kept=interior_kept)
