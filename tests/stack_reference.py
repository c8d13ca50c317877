"""NumPy restatement of the stacking step, written from include/sunerf_hip_stack.h: per pixel, in fp64, the valid samples sorted,
the clipping passes with their medians and MADs taken by rank, and the statistic over the survivors -- the mean as a literal loop
over the sorted survivors.  Pixels are handled one by one in plain Python: this is the specification, not a fast path."""
import numpy as np

REJECTED, INVALID = 1, 2
MEAN, MEDIAN, PERCENTILE, RANK = 0, 1, 2, 3
MODEL, MAD = 0, 1


def middle(s):
    """0.5 * (s[(n - 1) // 2] + s[n // 2]) of an ascending fp64 sequence."""
    n = len(s)
    return 0.5 * (s[(n - 1) // 2] + s[n // 2])


def clip_pixel(s, a=0.0, b=0.0, floor=0.0, mode=MODEL, n_sigma=5.0, iterations=0, clip_min=3, two_sided=False):
    """``s``: the valid samples ascending, fp64.  Returns ``(keep, passes)``: the bool array of the survivors and the number of
    passes that rejected something.  The test is applied to every survivor on its own; that the survivors stay a run is a
    property the tests check, not an assumption made here."""
    keep = np.ones(len(s), dtype=bool)
    passes = 0
    for _ in range(iterations):
        r = s[keep]
        if len(r) < clip_min:
            break
        m = middle(r)
        d = s - m
        if mode == MODEL:
            lim = (n_sigma * n_sigma) * (a + b * (m if m > 0 else 0.0))
            with np.errstate(over='ignore'):
                far = d * d > lim
            fail = (d > 0) & far
            if two_sided:
                fail |= (d < 0) & far
        else:
            scale = 1.4826 * middle(np.sort(np.abs(r - m)))
            scale = scale if scale > floor else floor
            lim = n_sigma * scale
            fail = d > lim
            if two_sided:
                fail |= -d > lim
        fail &= keep
        if not fail.any():
            break
        keep &= ~fail
        passes += 1
    return keep, passes


def statistic(r, method, q=0.0, rank=0):
    """Of the survivors ``r`` ascending, fp64, at least one."""
    n = len(r)
    if method == MEAN:
        total = 0.0
        for x in r:          # ascending, one rounding per addition
            total = total + float(x)
        return total / n
    if method == MEDIAN:
        return middle(r)
    if method == PERCENTILE:
        p = q / 100.0 * (n - 1)
        lo = int(np.floor(p))
        if lo >= n - 1:
            return r[lo]
        return r[lo] + (p - lo) * (r[lo + 1] - r[lo])
    return r[min(rank, n - 1)] if rank >= 0 else r[max(n + rank, 0)]


def combine(frames, bad=None, params=None, method=MEDIAN, q=0.0, rank=0, mode=MODEL, n_sigma=5.0, iterations=0, clip_min=3,
            min_valid=1, two_sided=False):
    """``frames`` [T, C, H, W] float32, ``bad`` of that shape or None, ``params`` [C, 4] = a, b, floor, 0.  Returns ``(image, count,
    mask, state)``: [C, H, W] float32 and uint8, [T, C, H, W] uint8 and [C, 4] int64."""
    frames = np.asarray(frames, dtype=np.float32)
    t, c, h, w = frames.shape
    params = np.zeros((c, 4)) if params is None else np.asarray(params, dtype=np.float64)
    valid = np.isfinite(frames)
    if bad is not None:
        valid &= np.asarray(bad) == 0
    image = np.full((c, h, w), np.nan, dtype=np.float32)
    count = np.zeros((c, h, w), dtype=np.uint8)
    mask = np.where(valid, 0, INVALID).astype(np.uint8)
    state = np.zeros((c, 4), dtype=np.int64)
    for p in range(c):
        a, b, floor = params[p, :3]
        for y in range(h):
            for x in range(w):
                ok = valid[:, p, y, x]
                column = frames[:, p, y, x].astype(np.float64)
                s = np.sort(column[ok])
                keep, passes = clip_pixel(s, a, b, floor, mode, n_sigma, iterations, clip_min, two_sided)
                r = s[keep]
                n = len(r)
                count[p, y, x] = n
                if n >= max(min_valid, 1):
                    with np.errstate(over='ignore'):
                        image[p, y, x] = np.float32(statistic(r, method, q, rank))
                else:
                    state[p, 2] += 1
                # a sample is a survivor when its value is one of the survivors' values: equal values share one fate
                rejected = ok & ~np.isin(column, r)
                mask[rejected, p, y, x] = REJECTED
                state[p, 0] += len(s) - n
                state[p, 1] += t - len(s)
                state[p, 3] = max(state[p, 3], passes)
    return image, count, mask, state


def is_run(s, keep):
    """The survivors of the ascending samples ``s`` are one run of them, and no value is both kept and rejected."""
    idx = np.nonzero(keep)[0]
    contiguous = len(idx) == 0 or idx[-1] - idx[0] + 1 == len(idx)
    return contiguous and not np.isin(s[~keep], s[keep]).any()
