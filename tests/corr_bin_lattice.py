"""A lattice of kernel, bin and anchor for the PSF-and-bin kernels (csrc/corr_bin.h), and a classifier
that says which path of that header a geometry takes.  Plain Python: the host arithmetic of corr_bin.h (``corr_tile``,
``corr_outputs_per_thread``, ``adjoint_lds_bytes``, the slice bounds of ``adjoint_stage_tile``) and of psf_grad.hip
(``psf_grad_plan``) restated, so that tests/test_corr_bin_lattice_host.py can assert that the cases reach every path and
tests/test_gpu_corr_bin_lattice.py can name the path of a geometry that fails.

A case has the shape of ``patch_reference``'s: ``(planes, H, W, kh, kw, bin, (ay, ax), per_plane)``; its data are
``patch_reference.case_data``'s; every case runs under both boundaries."""
import functools

import numpy as np

import instrument_reference as ir
import patch_reference as pr
import psf_grad_reference as pg

MAX_KERNEL, MAX_BIN = 96, 8                      # include/sunerf_hip_instrument.h
TILE = 32                                        # SUNERF_INSTRUMENT_TILE and SUNERF_PATCH_TILE
THREADS = 256
GRAD_CHUNK, GRAD_MAX_RUNS, GRAD_MAX_SC = 1024, 512, 4          # include/sunerf_hip_psf_grad.h; psf_grad.hip
LDS_OPT_IN = 64 * 1024                           # dynamic LDS above this has to be opted in, per kernel instantiation
LDS_LIMIT = 160 * 1024                           # LDS of a workgroup on gfx950
LDS_MAX = 139520                                 # adjoint_lds_bytes at (96, 96, 1), its largest value
BOUNDARIES = pr.BOUNDARIES
BOUNDARY_CODE = {'zero': pg.ZERO, 'nearest': pg.NEAREST}
SCALE = 0.25                                     # a scale other than 1, exact in binary


# ---- corr_bin.h and psf_grad.hip, restated ------------------------------------------------------------------------------------------
def floor_div(a, b):
    return a // b                                # Python's // floors; the header builds it from C's truncation


def ceil_div(a, b):
    return -((-a) // b)


def corr_tile(kh, kw, b):
    return min(TILE, (127 - max(kh, kw)) // b + 1)


def corr_outputs_per_thread(kh, kw, b):
    t = corr_tile(kh, kw, b)
    return (t * t + THREADS - 1) // THREADS


def adjoint_lds_bytes(kh, kw, b):
    sh, sw = (TILE + kh - 2) // b + 1, (TILE + kw - 2) // b + 1
    kwb = (kw + b - 1) // b
    return (kh * b * kwb + kwb) * 8 + (sh * sw + sw) * 4


def adjoint_slice(h, w, kh, kw, b, ay, ax, y0, x0):
    """(r_lo, r_hi, c_lo, c_hi) of the adjoint tile from (y0, x0) on: the detector pixels whose taps reach it."""
    y_last, x_last = min(y0 + TILE, h) - 1, min(x0 + TILE, w) - 1
    r_lo, r_hi = max(0, ceil_div(y0 + ay - (kh - 1), b)), min(h // b - 1, floor_div(y_last + ay, b))
    c_lo, c_hi = max(0, ceil_div(x0 + ax - (kw - 1), b)), min(w // b - 1, floor_div(x_last + ax, b))
    return r_lo, r_hi, c_lo, c_hi


def unreachable_tiles(h, w, kh, kw, b, ay, ax):
    """[(y0, x0)] of the adjoint tiles that no tap reaches: ``adjoint_sum_tile`` returns zeros for them at once."""
    out = []
    for y0 in range(0, h, TILE):
        for x0 in range(0, w, TILE):
            r_lo, r_hi, c_lo, c_hi = adjoint_slice(h, w, kh, kw, b, ay, ax, y0, x0)
            if r_hi - r_lo + 1 <= 0 or c_hi - c_lo + 1 <= 0:
                out.append((y0, x0))
    return out


def psf_grad_plan(planes, h, w, n_kernels, kh, kw, b):
    """dict(nt, group, slices, slice_rows, slice_cols, chunks, chunk_taps, items, n_runs): include/sunerf_hip_psf_grad.h's order."""
    t = corr_tile(kh, kw, b)
    taps = kh * kw
    chunks = (taps + GRAD_CHUNK - 1) // GRAD_CHUNK
    chunk_taps = (taps + chunks - 1) // chunks
    best = None
    for nt in range(1, GRAD_CHUNK // THREADS + 1):
        group = (chunk_taps + nt - 1) // nt
        if group > THREADS:
            continue
        avail = THREADS // group
        rows = min(t, avail)
        cols = max(1, min(GRAD_MAX_SC, t, avail // rows))
        if best is None or nt * best['slices'] <= best['nt'] * rows * cols:          # the smallest nt / slices, the largest such nt
            best = dict(nt=nt, group=group, slices=rows * cols, slice_rows=rows, slice_cols=cols)
    tiles = ((h // b + t - 1) // t) * ((w // b + t - 1) // t)
    items = (planes // n_kernels) * tiles
    best.update(chunks=chunks, chunk_taps=chunk_taps, items=items, n_runs=min(items, max(1, GRAD_MAX_RUNS // n_kernels)))
    return best


def n_kernels_of(case):
    return case[0] if case[7] else 1


def tags(case):
    """The paths of corr_bin.h and psf_grad.hip that the geometry of a case takes, as a frozenset of strings."""
    planes, h, w, kh, kw, b, (ay, ax), _ = case
    plan = psf_grad_plan(planes, h, w, n_kernels_of(case), kh, kw, b)
    lds = adjoint_lds_bytes(kh, kw, b)
    out = {f'T={corr_tile(kh, kw, b)}', f'NM={corr_outputs_per_thread(kh, kw, b)}', f'NT={plan["nt"]}', f'slices={plan["slices"]}'}
    flags = {'bin>kw': b > kw, 'bin>kh': b > kh, 'empty-tile': bool(unreachable_tiles(h, w, kh, kw, b, ay, ax)),
             'lds>64K': lds > LDS_OPT_IN, 'lds-max': lds == LDS_MAX, 'one-wide': w == 1, 'one-high': h == 1, 'H==bin': h == b,
             # an anchor in a corner that is not on the diagonal, where the taps of one axis all lie before the pixel and those
             # of the other all after it; with bin > 1 the clamped pixels of the two axes gather unlike ranges
             'corner-anchor': b > 1 and kh > 1 and kw > 1 and (ay, ax) in ((kh - 1, 0), (0, kw - 1))}
    return frozenset(out | {name for name, on in flags.items() if on})


FLAG_TAGS = ('bin>kw', 'bin>kh', 'empty-tile', 'lds>64K', 'lds-max', 'one-wide', 'one-high', 'H==bin', 'corner-anchor')


def describe(case):
    planes, h, w, kh, kw, b, anchor, per_plane = case
    return f'{planes}x{h}x{w} k{kh}x{kw} bin{b} anchor{anchor} {"per-plane" if per_plane else "shared"} [{" ".join(sorted(tags(case)))}]'


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
SMALL_PLANE = (37, 41)                           # 2 x 2 adjoint tiles, both last tiles partial


def small_anchors(kh, kw):
    out = []
    for anchor in ((0, 0), (kh - 1, kw - 1), (kh // 2, kw // 2), (0, kw - 1)):
        if anchor not in out:
            out.append(anchor)
    return out


def small_cases(b):
    """The geometries of SMALL at one bin: kh, kw in 1 .. 5, four anchors less their duplicates, one shared kernel."""
    return [(1,) + SMALL_PLANE + (kh, kw, b, anchor, False)
            for kh in range(1, 6) for kw in range(1, 6) for anchor in small_anchors(kh, kw)]


SMALL_BINS = tuple(range(1, MAX_BIN + 1))
SMALL = [case for b in SMALL_BINS for case in small_cases(b)]

# two planes with a kernel each: (H, W, kh, kw, bin, anchor)
_LARGE = [
    (34, 33, 96, 96, 1, (47, 48)),               # the LDS maximum, T = 32, NM = 4
    (34, 33, 96, 96, 1, (0, 95)),
    (40, 45, 96, 96, 5, (95, 0)),                # T = 7
    (36, 43, 96, 96, 7, (48, 48)),               # T = 5
    (70, 7, 96, 1, 3, (95, 0)),                  # long thin kernels: the tile is set by one axis, the LDS row by the other
    (7, 70, 1, 96, 6, (0, 10)),
    (66, 41, 65, 33, 4, (32, 16)),               # T = 16
    (71, 70, 3, 3, 8, (2, 2)),                   # five unreachable tiles each
    (71, 70, 1, 1, 8, (0, 0)),
    (8, 8, 2, 3, 8, (1, 2)),                     # H == W == bin
    (2, 64, 5, 5, 2, (2, 2)),
    (65, 3, 7, 7, 3, (3, 3)),
    (1, 1, 3, 3, 1, (1, 1)),
    (1, 40, 9, 9, 1, (4, 4)),                    # one pixel high, one pixel wide: both edges of an axis at once
    (40, 1, 9, 9, 1, (4, 4)),
    # Beyond the issue's list: the classifier showed no unreachable tile below bin 5 in SMALL (37 rows: the taps of the last
    # detector row reach row 32) and only bin 3 here.  At bin 2 the last tile must be the one trailing row that fills no detector
    # pixel, under an anchor on the kernel's last row; at bin 1 there is no such tile (test_corr_bin_lattice_host.py shows it).
    (33, 40, 20, 20, 2, (19, 0)),                # bin 2: row 32 alone is unreachable; a corner anchor
    (35, 38, 6, 3, 4, (3, 1)),                   # bin 4: rows 32 .. 34, and bin > kw
]
LARGE = [(2, h, w, kh, kw, b, anchor, True) for h, w, kh, kw, b, anchor in _LARGE]


def large_id(case):
    return '-'.join(str(v) for v in case[1:6]) + f'-a{case[6][0]}.{case[6][1]}'


# ---- the three restatements on a case ---------------------------------------------------------------------------------------------
def references(case, boundary):
    """dict of the three restatements at ``SCALE``: forward (fp32) and forward_acc (fp64, before scale), adjoint and adjoint_acc,
    taps (fp64) and taps_bound, beside the data K, x, g."""
    planes, h, w, kh, kw, b, anchor, _ = case
    K, x, g = pr.case_data(case)
    nk = n_kernels_of(case)
    fwd, fwd_acc = ir.correlate_bin(x, K, b, anchor, SCALE, boundary)
    adj, adj_acc = pr.correlate_bin_adjoint(g, K, h, w, b, anchor, SCALE, boundary)
    call = (nk, kh, kw, b, anchor[0], anchor[1], SCALE, BOUNDARY_CODE[boundary])
    out = dict(K=K, x=x, g=g, forward=fwd, forward_acc=fwd_acc, adjoint=adj, adjoint_acc=adj_acc,
               taps=pg.tap_gradient(x, g, *call), taps_bound=pg.tap_gradient_bound(x, g, *call))
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def large_references(case, boundary):
    """``references`` of a LARGE case, computed once (the 96 x 96 ones take seconds) and never written to."""
    return references(case, boundary)


def _axis_fan(n, k, b, anchor, boundary):
    """The largest number of (detector index, tap) pairs of one axis that read one input index."""
    idx = (np.arange(n // b) * b - anchor)[:, None] + np.arange(k)[None, :]
    if boundary == 'nearest':
        idx = np.clip(idx, 0, n - 1)
    idx = idx[(idx >= 0) & (idx < n)]
    return int(np.bincount(idx, minlength=n).max()) if idx.size else 0


def identity_check(case, boundary, ref):
    """The three restatements hold one number, the sum of K x g over every (plane, detector pixel, tap), each summed another way:
    ``<A x, g>`` (taps inside, detector pixels outside), ``<x, A^T g>`` (the terms of an input pixel inside, the pixels outside)
    and ``<K, dK> / scale`` (detector pixels inside, taps outside).  Returns (the three values, bound, mass).

    Bound.  The products of two fp32 values are exact in fp64; every addition, and the one product that joins an inner sum to
    its outer factor, rounds once, 2^-53 relative.  A term passes through at most N + 2 roundings, N the additions of the longest
    chain of its path: the inner terms plus the outer terms.  So each value is within (N + 2) 2^-53 mass of the exact sum, with
    mass = sum |K| |x| |g| over the footprint, and two of them differ by at most twice that -- the same form as
    ``psf_grad_reference.tap_gradient_bound``."""
    planes, h, w, kh, kw, b, (ay, ax), _ = case
    nk = n_kernels_of(case)
    oh, ow = h // b, w // b
    x64, g64 = ref['x'].astype(np.float64), ref['g'].astype(np.float64)
    values = (float((ref['forward_acc'] * g64).sum()), float((x64 * ref['adjoint_acc']).sum()),
              float((ref['K'] * ref['taps']).sum() / SCALE))          # K and taps are both [n_kernels, kh, kw]
    fan = _axis_fan(h, kh, b, ay, boundary) * _axis_fan(w, kw, b, ax, boundary)          # the terms of one input pixel at most
    chains = (kh * kw + planes * oh * ow, fan + planes * h * w, (planes // nk) * oh * ow + nk * kh * kw)
    mass = float((np.abs(g64) * pg.correlate_bin(np.abs(x64), np.abs(ref['K']), b, ay, ax, 1.0, BOUNDARY_CODE[boundary])).sum())
    return values, 2.0 * (max(chains) + 2) * 2.0 ** -53 * mass, mass
