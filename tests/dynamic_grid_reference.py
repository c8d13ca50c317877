"""float64 restatement of the voxel-grid field with a time axis in plain torch: the coordinates and cells
of tests/grid_field_reference.py for space, ``searchsorted`` on the frame times for time, a gather over the 16 corners; autograd
through the gather is the adjoint.  The checker of csrc/dynamic_grid.hip -- it shares no code with it or with
``sunerf_hip.dynamic_grid``.

Points and times are taken in fp32, as the kernel takes them, and promoted exactly; everything after that is float64.
"""
import torch

from grid_field_reference import grid_coordinates, locate, ray_points

TIME_MODES = ('clamp', 'fill')


def locate_time(frame_times, t, time_mode='clamp'):
    """Interval ``j (M,)`` long, weight ``s (M,)`` of the upper frame and ``inside (M,)`` of fp32 times ``t (M,)``.

    ``j = searchsorted(frame_times, t, 'left') - 1`` clipped to ``[0, T - 2]``, ``s = (t - tau_j) / (tau_{j+1} - tau_j)``.
    ``clamp``: ``t <= tau_0`` is ``(0, 0)``, ``t >= tau_{T-1}`` is ``(T - 2, 1)``; ``fill``: outside ``[tau_0, tau_{T-1}]`` is
    outside.  A NaN time is outside in both modes.  Outside samples get interval 0 and weight 0."""
    assert time_mode in TIME_MODES
    tau = torch.as_tensor(frame_times, dtype=torch.float64)
    n = tau.shape[0]
    t = t.double()
    nan = torch.isnan(t)
    inside = ~nan
    if time_mode == 'fill':
        inside = inside & (t >= tau[0]) & (t <= tau[-1])
    tt = torch.where(inside, t, tau[0].expand_as(t)).clamp(tau[0].item(), tau[-1].item())
    j = (torch.searchsorted(tau, tt.contiguous(), right=False) - 1).clamp(0, n - 2)
    s = (tt - tau[j]) / (tau[j + 1] - tau[j])
    return torch.where(inside, j, torch.zeros_like(j)), torch.where(inside, s, torch.zeros_like(s)), inside


def field(grid, frame_times, values, points, fill, Rs_per_ds=1.0, lon_mode='patch', time_mode='clamp'):
    """The field at fp32 ``points (M, 4) = (x, y, z, t)``: ``(raw (M, C) float64, abs_sum (M, C) = sum over the 16 corners of
    |w| |v|, inside (M,))``.  ``values (T, n0, n1, n2, C)`` (promoted; gradients flow to a float64 leaf passed in)."""
    v = values.double()
    u = grid_coordinates(grid, points, Rs_per_ds, lon_mode)
    i0, i1, t, inside = locate(grid, u, lon_mode)
    j, s, inside_t = locate_time(frame_times, points[:, 3], time_mode)
    inside = inside & inside_t
    m = points.shape[0]
    raw = torch.zeros(m, v.shape[-1], dtype=torch.float64)
    abs_sum = torch.zeros_like(raw)
    for dt in (0, 1):
        wt = s if dt else 1 - s
        for d0 in (0, 1):
            for d1 in (0, 1):
                for d2 in (0, 1):
                    idx = [(i1 if d else i0)[:, k] for k, d in enumerate((d0, d1, d2))]
                    w = wt.clone()
                    for k, d in enumerate((d0, d1, d2)):
                        w = w * (t[:, k] if d else 1 - t[:, k])
                    corner = v[j + dt, idx[0], idx[1], idx[2]]
                    raw = raw + w[:, None] * corner
                    abs_sum = abs_sum + w.abs()[:, None] * corner.detach().abs()
    fill = torch.as_tensor(fill, dtype=torch.float64).reshape(1, -1)
    raw = torch.where(inside[:, None], raw, fill.expand_as(raw))
    abs_sum = torch.where(inside[:, None], abs_sum, torch.zeros_like(abs_sum))
    return raw, abs_sum, inside


def node_terms(grid, frame_times, points, g_raw, Rs_per_ds=1.0, lon_mode='patch', time_mode='clamp'):
    """What bounds one (frame, node) of the adjoint on its own, from this restatement's cells, intervals and weights: ``(A (T,
    n0, n1, n2, C), n (T, n0, n1, n2) long)`` with ``A = sum_s |w_s| |g_s|`` over the inside samples whose (interval, cell)
    touches the frame's node (``w_s``: the sample's float64 weight at that corner of its 16) and ``n`` their number.
    ``points (M, 4)`` fp32, ``g_raw (M, C)``."""
    u = grid_coordinates(grid, points, Rs_per_ds, lon_mode)
    i0, i1, t, inside = locate(grid, u, lon_mode)
    j, s, inside_t = locate_time(frame_times, points[:, 3], time_mode)
    inside = inside & inside_t
    n_frames = len(frame_times)
    n0, n1, n2 = (int(a.shape[0]) for a in grid.axes)
    g = g_raw.reshape(points.shape[0], -1).double().abs()
    terms = torch.zeros(n_frames * n0 * n1 * n2, g.shape[1], dtype=torch.float64)
    count = torch.zeros(n_frames * n0 * n1 * n2, dtype=torch.long)
    for dt in (0, 1):
        wt = s if dt else 1 - s
        for d0 in (0, 1):
            for d1 in (0, 1):
                for d2 in (0, 1):
                    idx = [(i1 if d else i0)[:, k] for k, d in enumerate((d0, d1, d2))]
                    w = wt.clone()
                    for k, d in enumerate((d0, d1, d2)):
                        w = w * (t[:, k] if d else 1 - t[:, k])
                    flat = ((((j + dt) * n0 + idx[0]) * n1 + idx[1]) * n2 + idx[2])[inside]
                    terms.index_add_(0, flat, (w.abs()[:, None] * g)[inside])
                    count.index_add_(0, flat, torch.ones_like(flat))
    return terms.reshape(n_frames, n0, n1, n2, -1), count.reshape(n_frames, n0, n1, n2)


def field_on_rays(grid, frame_times, values, rays_o, rays_d, z_vals, times, fill, Rs_per_ds=1.0, lon_mode='patch',
                  time_mode='clamp'):
    """:func:`field` at the samples of a ray batch at the rays' fp32 ``times (N, 1) | (N,)``: ``(raw (N, S, C), abs_sum (N, S, C),
    inside (N, S))``."""
    pts = ray_points(rays_o, rays_d, z_vals)
    n, s = pts.shape[:2]
    t = times.float().cpu().reshape(n, 1, 1).expand(n, s, 1)
    raw, abs_sum, inside = field(grid, frame_times, values, torch.cat([pts, t], -1).reshape(-1, 4), fill, Rs_per_ds, lon_mode,
                                 time_mode)
    return raw.reshape(n, s, -1), abs_sum.reshape(n, s, -1), inside.reshape(n, s)


def temporal_smoothness(frame_times, values):
    """Hand computation of ``DynamicGridField.temporal_smoothness()`` with a Python loop over the intervals (float64)."""
    v = values.double()
    terms = []
    for j in range(v.shape[0] - 1):
        step = float(frame_times[j + 1]) - float(frame_times[j])
        terms.append(((v[j + 1] - v[j]) / step) ** 2)
    return torch.stack(terms).mean()


def smoothness(grid, values, lon_mode='patch'):
    """``DynamicGridField.smoothness()``: the mean over the frames of the static field's hand computation."""
    from grid_field_reference import smoothness as one
    return torch.stack([one(grid, values[f], lon_mode) for f in range(values.shape[0])]).mean()
