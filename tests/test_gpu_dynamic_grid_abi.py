"""The two device entry points of include/sunerf_hip_ext.h stay inside their buffers: the checks of
tests/test_gpu_abi_extents.py (runs A and B, guards, inputs untouched, outputs equal to the wrapper by bits and independent of
what they held, the workspace bound, the empty call) on cases built with ``abi_cases.Ctx`` / ``Case`` / ``HostValue`` and the
guarded arena of tests/abi_arena.py, with the extents the extension header states.

The cases live in this file's own table ``EXT_CASES`` (tests/test_abi_tables_host.py holds it to the table's symbols)."""
import pytest
import torch

import abi_cases as ac
from abi_arena import IN, OUT
from abi_cases import F32, I32, I64, STREAM, Case, Ctx, HostValue

pytestmark = pytest.mark.gpu

FRAMES = {2: (0.25, 0.75), 3: (0.0, 0.375, 1.0)}


def _lib():
    return ac._lib()


def _descriptor(c, name, ch, n_frames, mode):
    """The descriptor of the grid ``name`` of tests/test_gpu_grid_field.py with ``n_frames`` frames, whose axis arrays and frame
    times are arena buffers."""
    from sunerf_hip import dynamic_grid as dg
    from sunerf_hip import grid_field as gf
    from test_gpu_grid_field import FILL
    grid, space = ac._grid_descriptor(c, name, ch)
    desc = dg.DynamicGridDescriptor(grid, ch, 1.0, FILL[:ch], gf.longitude_mode(grid), FRAMES[n_frames], mode, 'cpu')
    tau = c.IN('frame_times', desc.frame_times)
    desc.space, desc.frame_times, desc.device = space, tau.t, c.device
    return grid, desc, tau


def _times(n):
    from test_gpu_dynamic_grid import ray_times
    return ray_times(n).reshape(n)


FWD_SHAPES = [(n, s, ch, mode, idx) for (n, s), ch in zip(((1, 1), (5, 51), (257, 1), (12, 67)), (1, 3, 4, 2))
              for mode in ('rays', 'points4') for idx in (0, 1)]
FWD_TILES = 'dynamic_grid.hip GF_THREADS 256 (grid_gather.h): one sample per thread (1, 255, 257 and 804 samples)'


def dynamic_grid_fwd(shape, device):
    n, s, ch, mode, want_index = shape
    c = Ctx(device)
    name = {1: 'nonuniform', 2: 'rotated', 3: 'sph_open', 4: 'sph_closed'}[ch]
    time_mode = 'clamp' if mode == 'rays' else 'fill'
    grid, desc, tau = _descriptor(c, name, ch, 3, time_mode)
    values = c.IN('values', torch.randn(3, *grid.shape, ch, generator=ac._gen(7 + ch)))
    o_t, d_t, z_t = ac._grid_rays(name, n, s)
    t_t = _times(n)
    total = n * s
    if mode == 'rays':
        o, d, z, t = c.IN('rays_o', o_t), c.IN('rays_d', d_t), c.IN('z_vals', z_t), c.IN('ray_times', t_t)
        points, stride, n_rays, n_samples = c.NULL('points', IN), 0, n, s
    else:
        p = (o_t[:, None, :] + d_t[:, None, :] * z_t[:, :, None])
        p = torch.cat([p, t_t.reshape(n, 1, 1).expand(n, s, 1)], -1).reshape(total, 4).contiguous()
        o, d, z, t = (c.NULL(k, IN) for k in ('rays_o', 'rays_d', 'z_vals', 'ray_times'))
        points, stride, n_rays, n_samples = c.IN('points', p), 4, total, 1
    raw = c.OUT('raw', F32, total * ch)
    cells, weights = (c.OUT('cells', I32, total), c.OUT('weights', F32, total * 8)) if want_index else \
        (c.NULL('cells', OUT), c.NULL('weights', OUT))

    def expected():
        from sunerf_hip import dynamic_grid as dg
        v = values.t.view(3, *grid.shape, ch)
        if mode == 'rays':
            r = dg.dynamic_grid_rays(desc, v, o.t.view(n, 3), d.t.view(n, 3), z.t.view(n, s), t.t.view(n), want_index=bool(want_index))
        else:
            r = dg.dynamic_grid_points(desc, v, points.t.view(total, 4), want_index=bool(want_index))
        return {'raw': r[0], 'cells': r[1][0], 'weights': r[1][1]} if want_index else {'raw': r}
    return Case('sunerf_dynamic_grid_fwd', shape, c.arena,
                [HostValue(desc.ref(), keep=desc), tau, 3, desc.time_mode, values, o, d, z, t, n_rays, n_samples, points, stride, raw,
                 cells, weights, STREAM], expected, empty={9: 0})


BWD_SHAPES = [(total, ch, acc) for total, ch in ((63, 1), (64, 3), (65, 4), (129, 2), (804, 3)) for acc in (0, 1)]
BWD_TILES = ('grid_gather.h GF_CHUNK 64: sorted positions per piece of a long segment; totals up to 129: every sample in the one '
             'cell and the one interval of a 2 x 2 x 2 grid with two frames (16 nodes: less than one block), so that the '
             'long-segment path and its `part` workspace run; 804 samples on the open spherical grid with three frames')


def dynamic_grid_bwd(shape, device):
    total, ch, acc = shape
    c = Ctx(device)
    name, n_frames = ('cell', 2) if total <= 129 else ('sph_open', 3)
    grid, desc, tau = _descriptor(c, name, ch, n_frames, 'clamp')
    n, s = (-(-total // 67), 67) if name == 'cell' else (12, 67)
    o_t, d_t, z_t = ac._grid_rays(name, n, s)
    t_t = torch.full((n,), 0.5) if name == 'cell' else _times(n)
    p = (o_t[:, None, :] + d_t[:, None, :] * z_t[:, :, None])
    p = torch.cat([p, t_t.reshape(n, 1, 1).expand(n, s, 1)], -1).reshape(-1, 4)[:total].contiguous()
    gen = ac._gen(total + ch)
    n_values = n_frames * grid.n_voxels * ch
    g_raw = c.IN('g_raw', torch.randn(total, ch, generator=gen))
    if c.gpu:
        from sunerf_hip import dynamic_grid as dg
        values = torch.zeros(n_frames, *grid.shape, ch, device=c.device)
        _, (cells_t, weights_t) = dg.dynamic_grid_points(desc, values, p.to(c.device), want_index=True)
        ids, perm_t = torch.sort(cells_t, stable=True)
        seg_t = torch.searchsorted(ids, torch.arange(desc.n_ids + 1, dtype=I32, device=c.device))
    else:
        cells_t, weights_t = torch.zeros(total, dtype=I32), torch.zeros(total, 8)
        perm_t, seg_t = torch.arange(total), torch.zeros(desc.n_ids + 1, dtype=I64)
    cells, weights = c.IN('cells', cells_t), c.IN('weights', weights_t)
    perm, seg = c.IN('perm', perm_t), c.IN('seg_start', seg_t)
    nbytes = int(_lib().sunerf_dynamic_grid_bwd_workspace_bytes(total, ch))
    ws = c.WS('workspace', nbytes)
    g0 = torch.randn(n_values, generator=gen)
    g_values = c.INOUT('g_values', g0) if acc else c.OUT('g_values', F32, n_values)

    def expected():
        from sunerf_hip import dynamic_grid as dg
        out = g0.to(c.device).view(n_frames, *grid.shape, ch).clone() if acc else None
        return {'g_values': dg.dynamic_grid_bwd(desc, g_raw.t.view(total, ch), (cells.t, weights.t.view(total, 8)), out=out,
                                                accumulate=bool(acc))}

    def empty_effect():          # header: n_total == 0 zeroes g_values unless accumulate
        return {} if acc else {'g_values': torch.zeros(n_values)}
    return Case('sunerf_dynamic_grid_bwd', shape, c.arena,
                [HostValue(desc.ref(), keep=desc), n_frames, g_raw, cells, weights, perm, seg, total, ws, nbytes, g_values, acc,
                 STREAM], expected, ws_index=9, empty={7: 0}, empty_effect=empty_effect)


EXT_CASES = {'sunerf_dynamic_grid_fwd': (dynamic_grid_fwd, tuple(FWD_SHAPES)),
             'sunerf_dynamic_grid_bwd': (dynamic_grid_bwd, tuple(BWD_SHAPES))}
EXT_TILES = {'sunerf_dynamic_grid_fwd': FWD_TILES, 'sunerf_dynamic_grid_bwd': BWD_TILES}
PAIRS = [(name, shape) for name, (_, shapes) in EXT_CASES.items() for shape in shapes]


@pytest.mark.parametrize('name,shape', PAIRS, ids=[f'{n[7:]}-{ac.shape_id(s)}' for n, s in PAIRS])
def test_extension_entry_point_stays_inside_its_buffers(name, shape):
    import test_gpu_abi_extents as extents
    extents.check_entry_point(EXT_CASES[name][0], name, shape)
