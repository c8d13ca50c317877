"""Case builders for the seams of the two voxel-grid fields: constructed layouts of the backward's sorted
inverted index, and points on the seams of a sphere where every decision of ``gf_locate`` is exact in IEEE arithmetic.
Importable without a GPU: tests/test_grid_seams_host.py checks on the CPU that every layout holds the seam it is named for,
tests/test_gpu_grid_seams.py runs them on the device.

A *layout* is a table of sample counts per id of the inverted index, in id order (the static field: the 24 cells of the
'nonuniform' grid of tests/test_gpu_grid_field.py; the field with a time axis: ``interval * 24 + cell``), plus a number of points
outside the grid, which get the sentinel id and sort last.  The backward cuts the sorted positions at the multiples of 64
(one piece per wave); a segment of more than 64 samples is *long* and goes through the piece kernel.

Two value modes.  *exact*: points at quarter fractions of their cell, times at quarter fractions of their interval, integer
``g_raw`` in [-8, 8]: every weight is k / 4, every product and every partial sum a multiple of 1 / 256 far below 2^24, so fp32
adds them without rounding in any order and the gradient must equal the restatement bit for bit.  *random*: uniform positions,
Gaussian ``g_raw``, judged by the bound per node.

The bound per node (derived, not measured).  A term ``w g`` of the static adjoint passes six fp32 roundings (three weights
rounded once from fp64, two products, the product with g), one of the dynamic adjoint eight; summing n terms in any order adds
at most n - 1; two more cover the second-order terms:  |got - want| <= (n + 8) 2^-24 A,  (n + 10) 2^-24 A with a time axis,
A = sum |w||g| over the node's n samples (``node_terms`` of the two reference modules).  A node with n = 0 is exactly 0.
"""
import math

import numpy as np
import torch

import dynamic_grid_reference as dref
import grid_field_reference as sref
import test_gpu_dynamic_grid as dynamic
import test_gpu_grid_field as static

CHUNK = 64                                   # sorted positions per piece: GF_CHUNK of csrc/grid_gather.h
EPS = 2.0 ** -24
STATIC_SLACK, DYNAMIC_SLACK = 8, 10          # the bound per node: (n + slack) 2^-24 A
FILL = static.FILL
MODES = ('exact', 'random')
N_CELLS = 24                                 # the 'nonuniform' grid: 4 x 3 x 2 cells
_F32 = torch.float32


# ---- the bound per node -----------------------------------------------------------------------------------------------------
def node_check(got, want, terms, count, slack):
    """max over nodes and channels of |got - want| / ((n + slack) 2^-24 A); asserts that nodes no sample touches, and nodes
    whose samples all have weight 0, are exactly 0.  ``got`` fp32 from the device, ``want`` / ``terms`` float64, ``count`` long."""
    got, want = got.detach().cpu().double(), want.double()
    assert got.shape == want.shape == terms.shape and count.shape == want.shape[:-1]
    bound = (count[..., None].double() + slack) * EPS * terms
    err = (got - want).abs()
    untouched = (count == 0)[..., None].expand_as(got)
    assert bool((got[untouched] == 0.0).all()), 'a node that no sample touches is not exactly 0'
    assert bool((terms[untouched] == 0.0).all())
    dead = bound == 0
    assert bool((err[dead] == 0.0).all()), 'a node whose samples all weigh 0 is not exactly 0'
    if bool(dead.all()):
        return 0.0
    return (err[~dead] / bound[~dead]).max().item()


def cell_ids(grid, points, Rs_per_ds=1.0, lon_mode='patch'):
    """(M,) long flattened cell id of every point as the forward leaves it for the backward, from the restatement's cells:
    ``(i0 nc1 + i1) nc2 + i2``, the wrap cell counted on an open longitude; outside points get the number of cells."""
    i0, _, _, inside = sref.locate(grid, sref.grid_coordinates(grid, points, Rs_per_ds, lon_mode), lon_mode)
    nc = cells_per_axis(grid, lon_mode)
    ids = (i0[:, 0] * nc[1] + i0[:, 1]) * nc[2] + i0[:, 2]
    return torch.where(inside, ids, torch.full_like(ids, nc[0] * nc[1] * nc[2]))


def cells_per_axis(grid, lon_mode):
    nc = [int(a.shape[0]) - 1 for a in grid.axes]
    if grid.kind == 'spherical' and lon_mode == 'open':
        nc[1] += 1
    return nc


def dynamic_ids(grid, frame_times, points, Rs_per_ds=1.0, lon_mode='patch', time_mode='clamp'):
    """(M,) long ``interval * n_cells + cell`` of points ``(x, y, z, t)``; outside in space or time: ``(T - 1) n_cells``."""
    cells = cell_ids(grid, points, Rs_per_ds, lon_mode)
    n_cells = int(np.prod(cells_per_axis(grid, lon_mode)))
    j, _, inside_t = dref.locate_time(frame_times, points[:, 3], time_mode)
    inside = inside_t & (cells < n_cells)
    return torch.where(inside, j * n_cells + cells, torch.full_like(cells, (len(frame_times) - 1) * n_cells))


# ---- layouts of the inverted index ------------------------------------------------------------------------------------------
def _sparse(n, **at):
    counts = [0] * n
    for k, v in at.items():
        counts[int(k[1:])] = v
    return counts


PROBE = [63, 64, 65, 1, 130, 62, 66, 0, 129, 64, 200, 3] + [0] * 11 + [70]          # 917 samples over the 24 cells

# name: (counts in id order, points outside, the seams the layout is there for -- checked on the CPU against seams())
LAYOUTS = {
    '64': ([64], 0, {'len64', 'total_64k'}),
    '65': ([65], 0, {'len65', 'long_starts_on_a_boundary'}),
    '63_65': ([63, 65], 0, {'len63', 'len65', 'long_starts_inside_a_piece', 'long_ends_on_a_boundary', 'total_64k'}),
    '65_63': ([65, 63], 0, {'len65', 'len63', 'short_after_a_long_in_its_piece', 'total_64k'}),
    '64_64_64': ([64, 64, 64], 0, {'len64', 'total_64k'}),
    '1_200': ([1, 200], 0, {'long_starts_inside_a_piece'}),
    '63_129': ([63, 129], 0, {'len63', 'long_starts_inside_a_piece', 'long_ends_on_a_boundary', 'total_64k'}),
    '128': ([128], 0, {'long_starts_on_a_boundary', 'long_ends_on_a_boundary', 'total_64k'}),
    '10_118': ([10, 118], 0, {'long_starts_inside_a_piece', 'long_ends_on_a_boundary', 'total_64k'}),
    '64_128': ([64, 128], 0, {'len64', 'long_starts_on_a_boundary', 'long_ends_on_a_boundary', 'total_64k'}),
    '100_100': ([100, 100], 0, {'two_long_ids_in_a_piece', 'long_starts_inside_a_piece'}),
    '65_65_65': ([65, 65, 65], 0, {'len65', 'two_long_ids_in_a_piece', 'long_starts_inside_a_piece'}),
    '70_5_70': ([70, 5, 70], 0, {'short_between_two_longs', 'two_long_ids_in_a_piece'}),
    '70_out20': ([70], 20, {'long_shares_its_last_piece_with_the_sentinel'}),
    '3_out200': ([3], 200, {'sentinel_longer_than_a_piece'}),
    '129': ([129], 0, {'long_starts_on_a_boundary', 'last_piece_of_one'}),
    '256': ([256], 0, {'long_ends_on_a_boundary', 'total_64k', 'total_256k'}),
    '257': ([257], 0, {'total_256k_plus_1', 'last_piece_of_one'}),
    'last_cell_out30': (_sparse(N_CELLS, c23=100), 30, {'long_in_the_last_id', 'long_shares_its_last_piece_with_the_sentinel'}),
    'from_cell5': (_sparse(7, c5=70, c6=3), 0, {'first_id_empty', 'long_starts_on_a_boundary'}),
    'probe': (PROBE, 0, {'len63', 'len64', 'len65', 'long_starts_inside_a_piece', 'two_long_ids_in_a_piece',
                         'short_between_two_longs', 'long_in_the_last_id'}),
}


def seams(counts, n_outside):
    """The seams a table of counts really holds, from its cumulative counts alone."""
    found = set()
    inside = sum(counts)
    total = inside + n_outside
    segments, begin = [], 0
    for k, c in enumerate(counts):
        if c:
            segments.append((k, begin, begin + c))
        begin += c
    for k, b, e in segments:
        if e - b in (63, 64, 65):
            found.add(f'len{e - b}')
        if e - b > CHUNK:
            found.add('long_starts_inside_a_piece' if b % CHUNK else 'long_starts_on_a_boundary')
            if e % CHUNK == 0:
                found.add('long_ends_on_a_boundary')
            elif e == inside and n_outside:
                found.add('long_shares_its_last_piece_with_the_sentinel')
            if k == len(counts) - 1:
                found.add('long_in_the_last_id')
    for q in range(-(-total // CHUNK)):
        lo, hi = q * CHUNK, min((q + 1) * CHUNK, total)
        held = [(k, b, e) for k, b, e in segments if b < hi and e > lo]
        is_long = [e - b > CHUNK for _, b, e in held]
        if sum(is_long) == 2:
            found.add('two_long_ids_in_a_piece')
        if len(held) >= 3 and is_long[0] and is_long[-1] and not all(is_long[1:-1]):
            found.add('short_between_two_longs')
        if len(held) >= 2 and is_long[0] and not is_long[1]:
            found.add('short_after_a_long_in_its_piece')
        if hi - lo == 1:
            found.add('last_piece_of_one')
    if total % CHUNK == 0:
        found.add('total_64k')
    if total % 256 == 0:
        found.add('total_256k')
    if total % 256 == 1:
        found.add('total_256k_plus_1')
    if inside and counts[0] == 0:
        found.add('first_id_empty')
    if n_outside > CHUNK:
        found.add('sentinel_longer_than_a_piece')
    return found


def _seed(*key):
    return sum((i + 1) * 7919 * sum(ord(ch) for ch in str(k)) for i, k in enumerate(key)) % (2 ** 31)


def _fractions(gen, shape, mode):
    """Where in its cell (interval) a sample sits, as a fraction in (0, 1): k / 4 (exact), or uniform away from the faces so
    that the rounding to fp32 cannot move it into a neighbour (random)."""
    if mode == 'exact':
        return torch.randint(1, 4, shape, generator=gen).double() / 4
    return 0.05 + 0.9 * torch.rand(shape, generator=gen, dtype=torch.float64)


def _outside(n, width):
    """n points outside the 'nonuniform' grid: beyond the last node of the first axis, and (from the second on) one NaN."""
    p = torch.zeros(n, width, dtype=torch.float64)
    p[:, 0] = 2.0 + 0.25 * (torch.arange(n) % 8)
    p[:, 1:3] = 0.125
    if width == 4:
        p[:, 3] = 0.5
    if n >= 2:
        p[1, 1] = math.nan
    return p


def _g_raw(gen, m, mode):
    if mode == 'exact':
        return torch.randint(-8, 9, (m, 4), generator=gen).float()
    return torch.randn(m, 4, generator=gen).float()


_BUILT = {}


def static_layout(name, mode):
    """Layout ``name`` of the static field on the 'nonuniform' grid, built once and shared: fp32 ``points (M, 3)`` in a fixed
    shuffled order, ``g_raw (M, 4)`` and ``values (5, 4, 3, 4)`` (a test with C channels takes the first C of each), the fp64
    restatement's ``raw``, ``abs_sum``, ``grad``, ``terms`` and ``count`` and the ``ids`` it expects."""
    key = ('static', name, mode)
    if key in _BUILT:
        return _BUILT[key]
    counts, n_outside, _ = LAYOUTS[name]
    grid = static.make_grid('nonuniform')
    gen = torch.Generator().manual_seed(_seed(*key))
    nc = cells_per_axis(grid, 'patch')
    assert nc == [4, 3, 2] and len(counts) <= N_CELLS
    chunks = []
    for cell, k in enumerate(counts):
        i = (cell // (nc[1] * nc[2]), (cell // nc[2]) % nc[1], cell % nc[2])
        lo = torch.stack([grid.axes[a][i[a]] for a in range(3)])
        hi = torch.stack([grid.axes[a][i[a] + 1] for a in range(3)])
        chunks.append(lo + _fractions(gen, (k, 3), mode) * (hi - lo))
    chunks.append(_outside(n_outside, 3))
    p64 = torch.cat(chunks)
    m = p64.shape[0]
    order = torch.randperm(m, generator=gen)
    p64 = p64[order]
    points = p64.float()
    g_raw = _g_raw(gen, m, mode)
    values = torch.randn(*grid.shape, 4, generator=gen).float()
    leaf = values.double().requires_grad_(True)
    raw, abs_sum, inside = sref.field(grid, leaf, points, FILL)
    (raw * g_raw.double()).sum().backward()
    terms, count = sref.node_terms(grid, points, g_raw)
    _BUILT[key] = dict(grid=grid, lon='patch', counts=counts, n_outside=n_outside, mode=mode, points=points, p64=p64, g_raw=g_raw,
                       values=values, raw=raw.detach(), abs_sum=abs_sum, inside=inside, grad=leaf.grad.clone(), terms=terms,
                       count=count, ids=cell_ids(grid, points))
    return _BUILT[key]


def _trimmed(counts):
    n = len(counts)
    while n and counts[n - 1] == 0:
        n -= 1
    return counts[:n]


def dynamic_table(name):
    """``(T, counts over the (T - 1) 24 ids, points outside)`` of a layout of the field with a time axis.

    ``NAME@j``: table NAME of LAYOUTS in interval j of ``FRAME_TIMES[5]``; ``NAME@1+2``: the table in interval 1 and, reversed, in
    interval 2 -- a cell that holds a long segment in one holds a short one in the other, so the node thread of frame 2 adds a
    long segment as the upper frame and a short one as the lower frame, and on the mirrored cell the other way round;
    ``NAME@T2``: the table in the one interval of ``FRAME_TIMES[2]``."""
    base, where = name.split('@')
    counts, n_outside, _ = LAYOUTS[base]
    if where == 'T2':
        return 2, list(counts) + [0] * (N_CELLS - len(counts)), n_outside
    table = [0] * (4 * N_CELLS)
    if where == '1+2':
        trimmed = _trimmed(counts)
        table[N_CELLS:N_CELLS + len(trimmed)] = trimmed
        table[2 * N_CELLS:2 * N_CELLS + len(trimmed)] = trimmed[::-1]
    else:
        j = int(where)
        table[j * N_CELLS:j * N_CELLS + len(counts)] = counts
    return 5, table, n_outside


DYNAMIC_LAYOUTS = tuple([f'{n}@{i % 4}' for i, n in enumerate(LAYOUTS)] + [f'{n}@1+2' for n in LAYOUTS if n != 'probe'] +
                        [f'{n}@T2' for n in ('100_100', '70_5_70', '70_out20')])


def dynamic_layout(name, mode):
    """Layout ``name`` (see :func:`dynamic_table`) of the field with a time axis, built once and shared: as
    :func:`static_layout` with ``points (M, 4)``, ``values (T, 5, 4, 3, 4)`` and ``tau``."""
    key = ('dynamic', name, mode)
    if key in _BUILT:
        return _BUILT[key]
    n_frames, counts, n_outside = dynamic_table(name)
    tau = dynamic.FRAME_TIMES[n_frames]
    grid = static.make_grid('nonuniform')
    gen = torch.Generator().manual_seed(_seed(*key))
    nc = cells_per_axis(grid, 'patch')
    chunks = []
    for ident, k in enumerate(counts):
        j, cell = divmod(ident, N_CELLS)
        i = (cell // (nc[1] * nc[2]), (cell // nc[2]) % nc[1], cell % nc[2])
        lo = torch.stack([grid.axes[a][i[a]] for a in range(3)] + [torch.tensor(tau[j], dtype=torch.float64)])
        hi = torch.stack([grid.axes[a][i[a] + 1] for a in range(3)] + [torch.tensor(tau[j + 1], dtype=torch.float64)])
        chunks.append(lo + _fractions(gen, (k, 4), mode) * (hi - lo))
    chunks.append(_outside(n_outside, 4))
    p64 = torch.cat(chunks)
    m = p64.shape[0]
    order = torch.randperm(m, generator=gen)
    p64 = p64[order]
    points = p64.float()
    g_raw = _g_raw(gen, m, mode)
    values = torch.randn(n_frames, *grid.shape, 4, generator=gen).float()
    leaf = values.double().requires_grad_(True)
    raw, abs_sum, inside = dref.field(grid, tau, leaf, points, FILL)
    (raw * g_raw.double()).sum().backward()
    terms, count = dref.node_terms(grid, tau, points, g_raw)
    _BUILT[key] = dict(grid=grid, lon='patch', tau=tau, time_mode='clamp', counts=counts, n_outside=n_outside, mode=mode,
                       points=points, p64=p64, g_raw=g_raw, values=values, raw=raw.detach(), abs_sum=abs_sum, inside=inside,
                       grad=leaf.grad.clone(), terms=terms, count=count, ids=dynamic_ids(grid, tau, points))
    return _BUILT[key]


# ---- long segments in the wrap cell of an open longitude --------------------------------------------------------------------
WRAP_SEGMENTS = (((2, 1), 65), ((3, 2), 200))          # ((latitude cell, radial cell), samples), longitude cell n1 - 1


def sphere_to_points(lat, lon, r):
    """fp64 Cartesian points of the node map ``X = r (-cos b sin l, cos b cos l, -sin b)``."""
    return torch.stack([-r * torch.cos(lat) * torch.sin(lon), r * torch.cos(lat) * torch.cos(lon), -r * torch.sin(lat)], -1)


def wrap_layout(with_time):
    """65 and 200 samples in two wrap cells of the 'sph_open' grid of tests/test_gpu_grid_field.py (random mode; with a time
    axis: in interval 1 of ``FRAME_TIMES[5]``), and 20 points outside the shells."""
    key = ('wrap', with_time)
    if key in _BUILT:
        return _BUILT[key]
    grid = static.make_grid('sph_open')
    lat, lon, r = grid.axes
    tau = dynamic.FRAME_TIMES[5]
    gen = torch.Generator().manual_seed(_seed(*key))
    chunks = []
    for (i0, i2), k in WRAP_SEGMENTS:
        f = _fractions(gen, (k, 4), 'random')
        chunks.append(torch.cat([sphere_to_points(lat[i0] + f[:, 0] * (lat[i0 + 1] - lat[i0]),
                                                  lon[-1] + f[:, 1] * (lon[0] + sref.TWO_PI - lon[-1]),
                                                  r[i2] + f[:, 2] * (r[i2 + 1] - r[i2])),
                                 (tau[1] + f[:, 3:] * (tau[2] - tau[1]))], -1))
    f = _fractions(gen, (20, 4), 'random')
    chunks.append(torch.cat([sphere_to_points(f[:, 0] * 2 - 1, f[:, 1] * 6 - 3, 2.5 + f[:, 2]), f[:, 3:]], -1))
    p64 = torch.cat(chunks)
    p64 = p64[torch.randperm(p64.shape[0], generator=gen)]
    points = p64.float().contiguous() if with_time else p64[:, :3].float().contiguous()
    m = points.shape[0]
    g_raw = _g_raw(gen, m, 'random')
    if with_time:
        values = torch.randn(5, *grid.shape, 4, generator=gen).float()
        leaf = values.double().requires_grad_(True)
        raw, abs_sum, inside = dref.field(grid, tau, leaf, points, FILL, 1.0, 'open')
        terms, count = dref.node_terms(grid, tau, points, g_raw, 1.0, 'open')
        ids = dynamic_ids(grid, tau, points, 1.0, 'open')
    else:
        values = torch.randn(*grid.shape, 4, generator=gen).float()
        leaf = values.double().requires_grad_(True)
        raw, abs_sum, inside = sref.field(grid, leaf, points, FILL, 1.0, 'open')
        terms, count = sref.node_terms(grid, points, g_raw, 1.0, 'open')
        ids = cell_ids(grid, points, 1.0, 'open')
    (raw * g_raw.double()).sum().backward()
    _BUILT[key] = dict(grid=grid, lon='open', tau=tau, time_mode='clamp', points=points, g_raw=g_raw, values=values,
                       raw=raw.detach(), abs_sum=abs_sum, inside=inside, grad=leaf.grad.clone(), terms=terms, count=count, ids=ids)
    return _BUILT[key]


def wrap_cell_ids(grid, with_time):
    """The ids of WRAP_SEGMENTS on ``grid`` ('sph_open')."""
    nc = cells_per_axis(grid, 'open')
    cells = [(i0 * nc[1] + nc[1] - 1) * nc[2] + i2 for (i0, i2), _ in WRAP_SEGMENTS]
    return [int(np.prod(nc)) + c for c in cells] if with_time else cells


# ---- the seams of a sphere, with exact decisions ----------------------------------------------------------------------------
SPHERES = ('full_closed', 'full_open', 'patch', 'full_open_to_zero')
SPHERE_LON = {'full_closed': 'closed', 'full_open': 'open', 'patch': 'patch', 'full_open_to_zero': 'open'}
PERIODIC = ('full_closed', 'full_open', 'full_open_to_zero')
SPHERE_TAU = (0.0, 0.1, 0.3)
SPHERE_TIMES = torch.tensor([0.0, 0.1, 0.05, 0.2, 0.3], dtype=_F32)      # on a frame; fp32(0.1) > 0.1; between; fp32(0.3) > 0.3
SCALES = (1.0, 0.25)                                                     # Rs_per_ds; the points are divided by it (exact)


def sphere_grid(name):
    from sunerf_hip.volume import SphericalGrid
    r = np.array([1.0, 1.25, 1.5, 2.0])
    if name == 'patch':
        return SphericalGrid(np.linspace(0.0, math.pi / 2, 3), np.linspace(-math.pi / 2, math.pi / 2, 5), r)
    lat = np.linspace(-math.pi / 2, math.pi / 2, 5)
    if name == 'full_open_to_zero':
        # the open sphere turned so that its last longitude node is exactly 0: the +y axis (lon = -+0) lies on it, where the wrap
        # cell begins -- u == lon[-1] belongs to the last ordinary cell with weight 1, u > lon[-1] to the wrap cell
        return SphericalGrid(lat, np.arange(-7, 1) * (math.pi / 4), r)
    lon = np.linspace(-math.pi, math.pi, 9) if name == 'full_closed' else np.linspace(-math.pi, math.pi, 8, endpoint=False)
    return SphericalGrid(lat, lon, r)


def axis_radii():
    """1, 1.25, 2 and one fp32 step either side of 1 and of 2: (7,) fp32, and which of them lie inside the shells [1, 2]."""
    one, two = torch.tensor(1.0, dtype=_F32), torch.tensor(2.0, dtype=_F32)
    up, down = torch.tensor(math.inf, dtype=_F32), torch.tensor(-math.inf, dtype=_F32)
    radii = torch.stack([one, torch.tensor(1.25, dtype=_F32), two, torch.nextafter(one, down), torch.nextafter(one, up),
                         torch.nextafter(two, down), torch.nextafter(two, up)])
    return radii, [True, True, True, False, True, True, False]


ZERO_SIGNS = ((0.0, 0.0), (0.0, -0.0), (-0.0, 0.0), (-0.0, -0.0))


def axis_points():
    """(168, 3) fp32: the six axis directions (+x, -x, +y, -y, +z, -z) x the 7 radii of :func:`axis_radii` x the four
    combinations of +0.0 and -0.0 in the other two components (in the order of the components); index
    ``(direction * 7 + radius) * 4 + combination``.  The squared radius has one non-zero term of 48 bits, so the fp64 root is
    exact; asin(+-1), asin(+-0), atan2 of zeros and of (+-r, +-0) are IEEE special values."""
    radii, _ = axis_radii()
    pts = []
    for axis in range(3):
        for sign in (1.0, -1.0):
            for r in radii.tolist():
                for za, zb in ZERO_SIGNS:
                    p = [za, zb]
                    p.insert(axis, sign * r)
                    pts.append(p)
    return torch.tensor(pts, dtype=torch.float64).float()


def special_points():
    """r = 0 with every sign of zero that matters, a NaN in each component, and points a hair off the plane z = 0 (the
    patch's lat = 0 face: decided by the sign of z; fp32 holds 1e-30)."""
    nan = math.nan
    return torch.tensor([[0.0, 0.0, 0.0], [-0.0, 0.0, 0.0], [0.0, -0.0, -0.0], [-0.0, -0.0, -0.0],
                         [nan, 1.5, 0.0], [0.25, nan, 1.5], [1.5, 0.25, nan], [nan, nan, nan],
                         [0.0, 1.5, 1e-30], [0.0, 1.5, -1e-30], [0.5, 1.25, 1e-30], [0.5, 1.25, -1e-30]], dtype=torch.float64).float()


N_SPECIAL_OUTSIDE = 8           # the first 8 of special_points() are outside every grid


def continuity_points(name):
    """fp32 points of a periodic grid next to its seams, computed in fp64 and rounded: 1e-7 either side of ``lon[0]``, 1e-7
    from either pole, and 40 random points inside the wrap cell (the last cell of a closed longitude)."""
    assert name in PERIODIC
    grid = sphere_grid(name)
    lon = grid.axes[1]
    gen = torch.Generator().manual_seed(_seed('continuity', name))
    d = 1e-7
    lat_s = torch.tensor([-1.3, -0.7, 0.0, 0.4, 1.1, 1.5], dtype=torch.float64)
    r_s = torch.tensor([1.0625, 1.375, 1.75], dtype=torch.float64)
    la, rr = (x.reshape(-1) for x in torch.meshgrid(lat_s, r_s, indexing='ij'))
    sets = [sphere_to_points(la, torch.full_like(la, lon[0].item() + s * d), rr) for s in (1.0, -1.0)]
    lo_s = torch.tensor([-3.0, -1.6, -0.1, 0.9, 2.2, 3.1], dtype=torch.float64)          # (-0.1: inside the turned sphere's wrap cell)
    lo, rr = (x.reshape(-1) for x in torch.meshgrid(lo_s, r_s, indexing='ij'))
    sets += [sphere_to_points(torch.full_like(lo, s * (math.pi / 2 - d)), lo, rr) for s in (1.0, -1.0)]
    f = torch.rand(40, 3, generator=gen, dtype=torch.float64)
    last = lon[-1] if SPHERE_LON[name] == 'open' else lon[-2]
    sets.append(sphere_to_points(-1.5 + 3.0 * f[:, 0], last + f[:, 1] * (lon[0] + sref.TWO_PI - last), 1.0625 + 0.875 * f[:, 2]))
    return torch.cat(sets).float()


def sphere_points(name, Rs_per_ds=1.0):
    """All points of sphere ``name`` in model units: the axis points, the special points and (periodic grids) the continuity
    points, divided by ``Rs_per_ds`` (1 or a power of two: exact)."""
    sets = [axis_points(), special_points()]
    if name in PERIODIC:
        sets.append(continuity_points(name))
    return (torch.cat(sets) / float(Rs_per_ds)).contiguous()


def sphere_case(name, Rs_per_ds=1.0):
    """The static field on sphere ``name`` at :func:`sphere_points`, built once and shared."""
    key = ('sphere', name, Rs_per_ds)
    if key in _BUILT:
        return _BUILT[key]
    grid, lon = sphere_grid(name), SPHERE_LON[name]
    points = sphere_points(name, Rs_per_ds)
    gen = torch.Generator().manual_seed(_seed('sphere', name))          # the same values and g_raw at every scale
    values = torch.randn(*grid.shape, 4, generator=gen).float()
    g_raw = torch.randn(points.shape[0], 4, generator=gen).float()
    leaf = values.double().requires_grad_(True)
    raw, abs_sum, inside = sref.field(grid, leaf, points, FILL, Rs_per_ds, lon)
    (raw * g_raw.double()).sum().backward()
    terms, count = sref.node_terms(grid, points, g_raw, Rs_per_ds, lon)
    _BUILT[key] = dict(grid=grid, lon=lon, Rs=Rs_per_ds, points=points, g_raw=g_raw, values=values, raw=raw.detach(),
                       abs_sum=abs_sum, inside=inside, grad=leaf.grad.clone(), terms=terms, count=count,
                       ids=cell_ids(grid, points, Rs_per_ds, lon))
    return _BUILT[key]


def dynamic_sphere_case(name, time_mode, Rs_per_ds=1.0):
    """The field with a time axis on sphere ``name``: every point of :func:`sphere_points` at every time of SPHERE_TIMES
    (time-major), frames at SPHERE_TAU."""
    key = ('dynamic_sphere', name, time_mode, Rs_per_ds)
    if key in _BUILT:
        return _BUILT[key]
    grid, lon = sphere_grid(name), SPHERE_LON[name]
    p3 = sphere_points(name, Rs_per_ds)
    m = p3.shape[0]
    points = torch.cat([p3.repeat(SPHERE_TIMES.shape[0], 1), SPHERE_TIMES.repeat_interleave(m)[:, None]], 1).contiguous()
    gen = torch.Generator().manual_seed(_seed('dynamic_sphere', name))
    values = torch.randn(len(SPHERE_TAU), *grid.shape, 4, generator=gen).float()
    g_raw = torch.randn(points.shape[0], 4, generator=gen).float()
    leaf = values.double().requires_grad_(True)
    raw, abs_sum, inside = dref.field(grid, SPHERE_TAU, leaf, points, FILL, Rs_per_ds, lon, time_mode)
    (raw * g_raw.double()).sum().backward()
    terms, count = dref.node_terms(grid, SPHERE_TAU, points, g_raw, Rs_per_ds, lon, time_mode)
    _BUILT[key] = dict(grid=grid, lon=lon, Rs=Rs_per_ds, tau=SPHERE_TAU, time_mode=time_mode, points=points, g_raw=g_raw,
                       values=values, raw=raw.detach(), abs_sum=abs_sum, inside=inside, grad=leaf.grad.clone(), terms=terms,
                       count=count, ids=dynamic_ids(grid, SPHERE_TAU, points, Rs_per_ds, lon, time_mode), n_space=m)
    return _BUILT[key]


# ---- the random rays of the existing tests, off Rs_per_ds = 1 ---------------------------------------------------------------
SCALED_RS = 0.7
SCALED_GRIDS = ('rotated', 'sph_open')


def scaled_rays_case(name, c=2):
    """The rays of ``test_gpu_grid_field.make_rays`` in model units of 0.7 solar radii (origins and directions divided by 0.7
    in fp32), with the existing assertion that no sample lies within 1e-6 of a face."""
    key = ('scaled', name, c)
    if key in _BUILT:
        return _BUILT[key]
    grid, lon = static.make_grid(name), static.LON.get(name, 'patch')
    o, d, z = static.make_rays(name, seed=100 + static.GRIDS.index(name))
    o, d = (o / SCALED_RS).contiguous(), (d / SCALED_RS).contiguous()
    gen = torch.Generator().manual_seed(_seed('scaled', name))
    values = torch.randn(*grid.shape, c, generator=gen).float()
    g_raw = torch.randn(*z.shape, c, generator=gen).float()
    leaf = values.double().requires_grad_(True)
    raw, abs_sum, inside = sref.field_on_rays(grid, leaf, o, d, z, FILL[:c], SCALED_RS, lon)
    (raw * g_raw.double()).sum().backward()
    pts = sref.ray_points(o, d, z).reshape(-1, 3)
    dist = sref.boundary_distance(grid, pts, SCALED_RS, lon)
    assert dist.min().item() > 1e-6, (name, dist.min().item())          # no sample where the two could disagree on inside
    frac = inside.float().mean().item()
    assert 0.05 < frac < 0.95, (name, frac)
    terms, count = sref.node_terms(grid, pts, g_raw.reshape(-1, c), SCALED_RS, lon)
    _BUILT[key] = dict(grid=grid, lon=lon, Rs=SCALED_RS, o=o, d=d, z=z, values=values, g_raw=g_raw, raw=raw.detach(),
                       abs_sum=abs_sum, inside=inside, grad=leaf.grad.clone(), terms=terms, count=count, c=c)
    return _BUILT[key]
