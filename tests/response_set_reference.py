"""Restatement of the density / temperature integral for a response set, in any dtype: ``sunerf_oracle.dt_integral`` with its
loop over the seven AIA rows replaced by a loop over the set's channels and codes (``orc.interp1d_linear_extrap0`` on each
channel's own grid), and the epilogues and gradients formed the way ``test_gpu_dt_integral.oracle`` forms them.  What the kernels
of csrc/dt_response_set.hip are held against (tests/test_gpu_response_set.py), evaluated in float64 and in float32."""
import torch

import sunerf_oracle as orc

CHUNK = 1024            # rays per evaluation: the scalar gradients are sums over rays, added over chunks in fp64


def dt_integral(inferences, log_abs, vol_c, z_vals, wavelengths, channels, pixel_intensity_factor):
    """``orc.dt_integral`` for ``channels`` = [(code, logt (n_c,), resp (n_c,))] and ``log_abs`` = one scalar per channel, in
    that order.  A wavelength entry that is no code of the set leaves response and absorption 0."""
    wl = wavelengths[:, None, :].expand(wavelengths.shape[0], inferences.shape[1], wavelengths.shape[1])
    density = torch.exp(torch.nn.functional.relu(inferences[..., 0]))
    density = density[:, :, None].expand(-1, -1, wl.shape[2])
    log_temperature = torch.nn.functional.relu(inferences[..., 1])
    temperature_response = torch.zeros_like(wl)
    absorption_coefficients = torch.zeros_like(wl)
    for (code, logt, resp), la in zip(channels, log_abs):
        sel = wl == float(code)
        if sel.any():
            tmp = orc.interp1d_linear_extrap0(logt, resp, log_temperature.flatten()).reshape(log_temperature.shape)
            temperature_response = torch.where(sel, tmp[:, :, None].expand_as(wl), temperature_response)
            absorption_coefficients = torch.where(sel, torch.nn.functional.relu(la).expand_as(wl), absorption_coefficients)
    absorption = density * absorption_coefficients
    absorption_integral = torch.cumulative_trapezoid(absorption, x=z_vals[:, :, None], dim=1)
    emission = density.pow(2) * temperature_response
    pixel_intensity_term = torch.exp(-absorption_integral) * emission[:, 0:-1, :]
    pixel_intensity = torch.trapezoid(pixel_intensity_term, x=z_vals[:, 0:-1, None], dim=1) * vol_c * pixel_intensity_factor
    weights = torch.nn.functional.relu(inferences[..., 0])
    weights = weights / (weights.sum(1)[:, None] + 1e-10)
    return {'image': pixel_intensity, 'weights': weights,
            'regularizing_quantity': torch.nn.functional.relu(inferences[..., 0])}


def oracle(c, channels, dtype, rest=None, reg_radius=1.25):
    """``dt_integral`` + the epilogues of base_tracing.py:99-110 in ``dtype`` on the fp32 inputs of case ``c`` (the dict of
    ``response_set_cases.make_case`` / ``test_gpu_dt_integral.make_case``), over chunks of rays.  ``channels``: [(code, name,
    logt, resp)].  Gradients of L = sum(g_image image) [+ sum(g_reg regularization) + sum(g_weights weights) + sum(g_reg_q reg_q)
    with ``rest``] w.r.t. the inferences (= raw), the M log_abs and vol_c, the scalar ones summed over the chunks in fp64."""
    chans = [(code, logt.to(dtype), resp.to(dtype)) for code, _, logt, resp in channels]
    m_ch = len(chans)
    keys = ('image', 'weights', 'reg_q', 'regularization', 'dist_k', 'height_map', 'absorption_map', 'g_raw')
    out = {k: [] for k in keys}
    g_la, g_vc = torch.zeros(m_ch, dtype=torch.float64), torch.zeros((), dtype=torch.float64)
    for a in range(0, c['n'], CHUNK):
        sl = slice(a, a + CHUNK)
        inf = c['inf'][sl].to(dtype).requires_grad_(True)
        la = [c['log_abs'][i].to(dtype).requires_grad_(True) for i in range(m_ch)]
        vc = c['vol_c'][0].to(dtype).requires_grad_(True)
        z = c['z'][sl].to(dtype)
        f = dt_integral(inf, la, vc, z, c['wl'][sl].to(dtype), chans, c['pixel'])
        pts = orc.points_on_rays(c['o'][sl].to(dtype), c['d'][sl].to(dtype), z)
        dist = pts.pow(2).sum(-1).pow(0.5)
        q = f['regularizing_quantity']
        reg = torch.relu(dist - reg_radius) * torch.relu(q)
        dist_k = ((pts[..., 0] * pts[..., 0] + pts[..., 1] * pts[..., 1]) + pts[..., 2] * pts[..., 2]).sqrt()
        loss = (f['image'] * c['g_image'][sl].to(dtype)).sum()
        if rest is not None:
            loss = loss + sum((t * rest[k][sl].to(dtype)).sum() for k, t in (('g_reg', reg), ('g_weights', f['weights']),
                                                                             ('g_reg_q', q)))
        grads = torch.autograd.grad(loss, [inf, vc] + la, allow_unused=True)
        with torch.no_grad():
            for k, v in (('image', f['image']), ('weights', f['weights']), ('reg_q', q), ('regularization', reg),
                         ('dist_k', dist_k),
                         ('height_map', (f['weights'] * dist).sum(-1)), ('absorption_map', (1 - q).sum(-1)), ('g_raw', grads[0])):
                out[k].append(v.detach())
            g_vc += grads[1].double()
            g_la += torch.stack([torch.zeros((), dtype=torch.float64) if g is None else g.double() for g in grads[2:]])
    res = {k: torch.cat(v) for k, v in out.items()}
    res.update(g_log_abs=g_la, g_vol_c=g_vc)
    return res


def measure(got, c, codes, ref64, ref32, full64=None, full32=None):
    """The figures of group 1 of tests/test_gpu_response_set.py for the outputs ``got`` (CPU tensors: the forward's keys, ``g_raw``,
    ``g_log_abs``, ``g_vol_c`` and, with ``full64``, ``g_raw_full`` / ``g_log_abs_full`` / ``g_vol_c_full``) of case ``c``
    against the references, with the definitions of tests/test_gpu_dt_integral.py (imported); asserts the exact zeros on the way.
    Returns {name: worst value}."""
    from conftest import gate_units
    from test_gpu_dt_integral import ray_units, scalar_rel
    m = {}
    m['image'] = gate_units(got['image'], ref64['image'], floor=2 * (ref32['image'].double() - ref64['image']).abs())
    absent = ~torch.isin(c['wl'], torch.tensor(codes, dtype=torch.float32))
    assert bool((got['image'][absent] == 0).all()), 'absent / unknown channel column not exactly 0'
    m['reg_q_bits'] = float(not torch.equal(got['reg_q'], ref32['reg_q']))
    w_err = (got['weights'].double() - ref64['weights']).abs()
    assert bool((w_err[ref64['weights'] == 0] == 0).all())
    m['weights'] = (w_err / ref64['weights'].abs().clamp_min(1e-300)).max().item()
    m['height_map'] = ((got['height_map'].double() - ref64['height_map']).abs() / ref64['height_map'].abs()).max().item()
    m['absorption_map'] = ((got['absorption_map'].double() - ref64['absorption_map']).abs()
                           / (1 - ref64['reg_q']).abs().sum(-1)).max().item()
    inf = c['inf']
    present = torch.tensor([bool((c['wl'] == float(code)).any()) for code in codes])
    la_zero = (c['log_abs'][:len(codes)] <= 0) | ~present
    none = ~present.any().reshape(1)
    for tag, r64, r32 in (('', ref64['g_raw'], ref32['g_raw']),) + ((('_full', full64, full32),) if full64 is not None else ()):
        g = got['g_raw' + tag]
        assert bool((g[..., 0][inf[..., 0] <= 0] == 0).all()), 'g_raw[..., 0] nonzero where relu(inf0) is flat'
        if not tag:
            assert bool((g[..., 1][inf[..., 1] <= 0] == 0).all()), 'g_raw[..., 1] nonzero where relu(inf1) is flat'
        m['g_raw' + tag] = ray_units(g, r64, r32)
        m['g_log_abs' + tag] = scalar_rel(got['g_log_abs' + tag], ref64['g_log_abs'], la_zero)
        m['g_vol_c' + tag] = scalar_rel(got['g_vol_c' + tag], ref64['g_vol_c'], none)
    return m


def assert_bounds(m, scalar_gradient_rel):
    """The bounds of tests/test_gpu_dt_integral.py's docstring on the figures of :func:`measure`."""
    assert m['image'] <= 1.0, m
    assert m['reg_q_bits'] == 0, 'reg_q differs from the fp32 expression by bits'
    assert m['weights'] <= 1e-5 and m['height_map'] <= 1e-5 and m['absorption_map'] <= 1e-5, m
    for k in m:
        if k.startswith('g_raw'):
            assert m[k] <= 1.0, (k, m)
        if k.startswith('g_log_abs') or k.startswith('g_vol_c'):
            assert m[k] <= scalar_gradient_rel, (k, m)


def rest_gradient(c, rest, dtype, reg_radius=1.25):
    """(N, S, 2): the gradient of sum(g_reg regularization) + sum(g_weights weights) + sum(g_reg_q reg_q) w.r.t. the inferences.
    None of the three depends on a channel, so the gradient of the full backward's loss is ``oracle(...)['g_raw']`` plus this
    (the sum autograd itself forms); evaluating the channel-free part alone keeps the large cases quick."""
    inf0 = c['inf'][..., 0].to(dtype).requires_grad_(True)
    q = torch.relu(inf0)
    weights = q / (q.sum(1)[:, None] + 1e-10)
    pts = orc.points_on_rays(c['o'].to(dtype), c['d'].to(dtype), c['z'].to(dtype))
    reg = torch.relu(pts.pow(2).sum(-1).pow(0.5) - reg_radius) * torch.relu(q)
    loss = sum((t * rest[k].to(dtype)).sum() for k, t in (('g_reg', reg), ('g_weights', weights), ('g_reg_q', q)))
    g, = torch.autograd.grad(loss, [inf0])
    return torch.stack([g, torch.zeros_like(g)], -1)


def render(field, heads, rays_o, rays_d, times, wavelengths, channels, n_coarse, n_fine, pixel_factor, t_vals=None,
           distance=1.3, reg_radius=1.25, z_given=None):
    """``orc.render_dt`` (base_tracing.py:46-111 for the DT subclass) against a response set, in fp32 on the CPU.  ``field``:
    ``(coarse, fine)`` callables ``points (N, S, 3), times -> inferences (N, S, 2)`` with the base offsets added; ``heads``:
    ``((log_abs list, vol_c), (log_abs list, vol_c))`` in the set's order; ``channels``: [(code, name, logt, resp)].
    ``z_given = (z_stratified, z_combined)``: integrate on these sample positions instead of placing the samples here (no
    gradient passes through them, sampling.py:120) -- what a test of the integral and the fields wants: the samplers have their
    own tests, and a resampled position that differs in its last bits moves every gradient a little."""
    chans = [(code, logt, resp) for code, _, logt, resp in channels]
    t_vals = orc.linspace_t_vals(n_coarse) if t_vals is None else t_vals
    z_vals = orc.stratified_z(rays_o, rays_d, t_vals, torch.tensor(distance, dtype=torch.float32),
                              torch.tensor(1., dtype=torch.float32)) if z_given is None else z_given[0]

    def one_pass(f, head, z):
        pts = orc.points_on_rays(rays_o, rays_d, z)
        inf = f(pts, times)
        out = dt_integral(inf, head[0], head[1], z, wavelengths, chans, pixel_factor)
        out.update(points=pts, inferences=inf)
        return out
    c = one_pass(field[0], heads[0], z_vals)
    new_z, z_comb = orc.hierarchical_z(z_vals, c['weights'], n_fine)
    if z_given is not None:
        z_comb = z_given[1]
    f = one_pass(field[1], heads[1], z_comb)
    q = f['regularizing_quantity']
    dist = f['points'].pow(2).sum(-1).pow(0.5)
    return {'z_vals_stratified': z_vals, 'coarse_image': c['image'], 'fine_image': f['image'], 'z_vals_hierarchical': new_z,
            'height_map': (f['weights'] * dist).sum(-1), 'absorption_map': (1 - q).sum(-1),
            'regularization': torch.relu(dist - reg_radius) * torch.relu(q), '_z_vals_combined': z_comb,
            '_fine_inferences': f['inferences'], '_coarse_inferences': c['inferences']}
