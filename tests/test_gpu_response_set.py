"""The density / temperature integral against a response set (csrc/dt_response_set.hip: sunerf_dt_response_fwd / _bwd /
_bwd_full, include/sunerf_hip_response.h) and the module path that uses it (``ResponseSet``, ``response_set=``, ``channels=``).

1. The kernels called directly against the fp64 restatement (tests/response_set_reference.py) on the 11-channel set and the
   cases of tests/response_set_cases.py: S in (3, 31, 32, 33, 65, 300) at N = 9, N in (1, 7, 16389) at S = 33, W in (1, 3, 8),
   both bases.  The bounds and their definitions are those of tests/test_gpu_dt_integral.py (imported), worst values measured
   on an MI355X over all cases of this group:
     image            gate_units vs fp64, floor 2 |ref32 - ref64|                                  <= 1      (0.015)
                      absent / unknown columns exactly 0
     reg_q            bit-identical to the fp32 expression
     weights          1e-5 relative per element                                                    (2.1e-7)
     height_map       1e-5 relative per ray                                                        (2.4e-7)
     absorption_map   1e-5 of sum_s |1 - q_s| per ray                                              (1.7e-7)
     g_raw            per ray, test_gpu_dt_integral.ray_units (image-only and full backward)       <= 1      (0.0085 / 0.017)
                      exactly 0 behind a closed relu
     g_log_abs, g_vol_c   SCALAR_GRADIENT_REL = 1e-4 relative                                      (9.4e-7 / 9.7e-7, two runs)
                      g_log_abs exactly 0 where log_abs <= 0 or the channel is absent from every ray
   Forward outputs and g_raw are bit-identical across reruns.
2. On ``ResponseSet.aia(g6 tables)`` and ``test_gpu_dt_integral.make_case``'s inputs the three entry points equal
   sunerf_dt_integral_fwd / _bwd / _bwd_full bit for bit (image, weights, reg_q, the maps, regularization, g_raw, absmax);
   g_log_abs / g_vol_c (float atomics) within SCALAR_GRADIENT_REL.
3. Empty batch, the LDS query and the LDS limit.
4. The module level: bit-equality of an AIA set with the default rendering, the generic hook path, one training step of
   ``NeRF_DT`` and of ``SimpleStar`` on the 11 channels, code 174 from both sides, the ``.snf`` round trip.
"""
import datetime

import pytest
import torch

import response_set_cases as rc
import response_set_reference as rr
import test_gpu_dt_integral as dt
from conftest import gate_units, load_golden

pytestmark = pytest.mark.gpu

SCALAR_GRADIENT_REL = dt.SCALAR_GRADIENT_REL
REG_RADIUS = rc.REG_RADIUS


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    from sunerf_hip import ops as _ops
    return _ops


def dev_args(c, rset):
    b_rho, b_t = dt.BASES[c['base']]
    return (c['raw'].cuda(), c['z'].cuda(), c['o'].cuda(), c['d'].cuda(), c['wl'].cuda(), rset, c['log_abs'].cuda(),
            c['vol_c'].cuda(), b_rho, b_t, c['pixel'], REG_RADIUS)


# ---- 1. kernels against fp64 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,s,w,base', rc.GROUP1, ids=[f'N{n}-S{s}-W{w}-{b}' for n, s, w, b in rc.GROUP1])
def test_response_kernels_against_fp64(ops, n, s, w, base):
    c = rc.group1_case(n, s, w, base)
    channels = rc.channels()
    args = dev_args(c, rc.response_set())
    g_img = c['g_image'].cuda()
    f, f_again = (ops.dt_response_fwd(*args, want_epilogues=True) for _ in range(2))
    bwd, bwd_again = (ops.dt_response_bwd(*args, g_img, None) for _ in range(2))
    ref64, ref32 = rr.oracle(c, channels, torch.float64), rr.oracle(c, channels, torch.float32)
    rest = dt.make_rest(c, ref64)
    rd = {k: v.cuda() for k, v in rest.items()}
    full, full_again = (ops.dt_response_bwd_full(*args, g_img, rd['g_reg'], rd['g_weights'], rd['g_reg_q']) for _ in range(2))
    torch.cuda.synchronize()
    for k in f:
        assert torch.equal(f[k], f_again[k]), f'forward {k} differs between two runs'
    assert torch.equal(bwd[0], bwd_again[0]) and torch.equal(full[0], full_again[0]), 'g_raw differs between two runs'
    assert bwd[3].view(torch.float32).item() == bwd[0].abs().max().item()
    assert full[3].view(torch.float32).item() == full[0].abs().max().item()

    got = {k: v.cpu() for k, v in f.items()}
    got.update(g_raw=bwd[0].cpu(), g_log_abs=bwd[1].cpu(), g_vol_c=bwd[2].cpu(), g_raw_full=full[0].cpu(),
               g_log_abs_full=full[1].cpu(), g_vol_c_full=full[2].cpu())
    full64 = ref64['g_raw'] + rr.rest_gradient(c, rest, torch.float64)
    full32 = ref32['g_raw'] + rr.rest_gradient(c, rest, torch.float32)
    m = rr.measure(got, c, rc.CODES, ref64, ref32, full64, full32)
    print(f'N={n} S={s} W={w} {base}: ' + ' '.join(f'{k} {v:.2e}' for k, v in m.items()))
    rr.assert_bounds(m, SCALAR_GRADIENT_REL)


def test_response_no_channel_present(ops):
    """Rows without a single code of the set: image, g_raw, g_log_abs and g_vol_c exactly 0."""
    c = rc.make_case(9, 40, 3, 'generic', seed=3)
    c['wl'] = torch.tensor([0., -1., rc.UNKNOWN]).repeat(9, 1)
    args = dev_args(c, rc.response_set())
    f = ops.dt_response_fwd(*args)
    g_raw, g_la, g_vc, _ = ops.dt_response_bwd(*args, c['g_image'].cuda(), None)
    torch.cuda.synchronize()
    assert bool((f['image'] == 0).all()) and bool((g_la == 0).all()) and bool((g_vc == 0).all()) and bool((g_raw == 0).all())


# ---- 2. equivalence with the AIA kernels ----------------------------------------------------------------------------------
@pytest.mark.parametrize('w', [1, 7])
@pytest.mark.parametrize('s', [3, 33, 257])
def test_aia_set_equals_the_aia_kernels_by_bits(ops, s, w):
    """An expression of dt_response_set.hip that differs from dt.hip shows here."""
    from sunerf_hip.response import ResponseSet
    base = 'nerf_dt' if w == 7 else 'generic'
    c = dt.make_case(21, s, w, base, seed=40 + s + w)
    g6 = load_golden('g6_dt_e2e')
    rset = ResponseSet.aia((g6['aia_logte'], g6['aia_tresp']), exposure=float(g6['aia_exp_time']))
    old, new = dt.dev_args(c), dev_args(c, rset)
    g_img = c['g_image'].cuda()
    gen = torch.Generator().manual_seed(s)
    extra = [(0.5 - torch.rand(21, s, generator=gen)).cuda() for _ in range(3)]
    f_old, f_new = ops.dt_integral_fwd(*old, want_epilogues=True), ops.dt_response_fwd(*new, want_epilogues=True)
    pairs = [(ops.dt_integral_bwd(*old, g_img, extra[0]), ops.dt_response_bwd(*new, g_img, extra[0])),
             (ops.dt_integral_bwd(*old, g_img, None), ops.dt_response_bwd(*new, g_img, None)),
             (ops.dt_integral_bwd_full(*old, g_img, *extra), ops.dt_response_bwd_full(*new, g_img, *extra))]
    torch.cuda.synchronize()
    assert set(f_old) == set(f_new)
    for k in f_old:
        assert torch.equal(f_old[k].view(torch.int32), f_new[k].view(torch.int32)), f'forward {k}'
    assert bool((f_new['image'] != 0).any())
    for i, (a, b) in enumerate(pairs):
        assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)), f'g_raw of backward {i}'
        assert torch.equal(a[3], b[3]), f'absmax of backward {i}'
        for k in (1, 2):
            ref = a[k].cpu().double()
            assert dt.scalar_rel(b[k], ref, ref.reshape(-1) == 0) <= SCALAR_GRADIENT_REL, (i, k, a[k], b[k])


# ---- 3. empty batch, LDS ------------------------------------------------------------------------------------------------------
def _bwd_raw(ops, c, rset, n, small, entry='sunerf_dt_response_bwd'):
    """The backward through the C entry point, the three small outputs in caller-owned (prefilled) memory -> status."""
    from sunerf_hip import lib as _l
    args = dev_args(c, rset)
    raw, z, o, d, wl = (t[:n] for t in args[:5])
    g_image = c['g_image'][:n].cuda()
    g_raw = torch.full((n, c['s'], 2), float('nan'), device='cuda')
    dev = z.device
    fn = getattr(_l.load(), entry)
    status = fn(ops._ptr(raw), ops._ptr(z), ops._ptr(o), ops._ptr(d), ops._ptr(wl), c['w'], *ops._response_set_args(rset, dev),
                ops._ptr(args[6]), ops._ptr(args[7]), *args[8:12], n, c['s'], ops._ptr(g_image),
                *([None] * (3 if entry.endswith('_full') else 1)), ops._ptr(g_raw),
                ops._ptr(small[0]), ops._ptr(small[1]), ops._ptr(small[2]), ops._stream(dev))
    return status, g_raw


def test_response_bwd_empty_batch(ops):
    """n_rays = 0 clears g_log_abs [M], g_vol_c and the absmax word, whether the three share one buffer or not; the forward
    returns 0 without reading a pointer."""
    rset = rc.response_set()
    m = rset.n_channels
    c = rc.make_case(1, 33, 8, 'generic', seed=1)
    joint = torch.full((m + 2,), float('nan'), device='cuda')
    assert _bwd_raw(ops, c, rset, 0, (joint[:m], joint[m:m + 1], joint[m + 1:]))[0] == 0
    apart = [torch.full((k,), float('nan'), device='cuda') for k in (m, 1, 1)]
    assert _bwd_raw(ops, c, rset, 0, apart)[0] == 0
    torch.cuda.synchronize()
    assert bool((joint == 0).all()), joint
    assert all(bool((t == 0).all()) for t in apart), apart
    e = rc.make_case(0, 33, 8, 'generic', seed=1)
    out = ops.dt_response_bwd(*dev_args(e, rset), torch.zeros(0, 8, device='cuda'), None)
    f = ops.dt_response_fwd(*dev_args(e, rset))
    torch.cuda.synchronize()
    assert out[0].numel() == 0 and bool((out[1] == 0).all()) and out[1].numel() == m and bool((out[2] == 0).all()) \
        and out[3].item() == 0
    assert f['image'].shape == (0, 8)


def test_response_bwd_lds_query_and_limit(ops):
    """The query is what the launcher enforces: with the 11-channel set (1005 nodes) 605 samples x 8 columns need 163 720 B and
    run; 606 need 163 976 B, more than a CU's 160 KiB: SUNERF_E_UNSUPPORTED before anything is queued, nothing written.  The
    same 606 samples at one column run: the slab is strided by the call's W."""
    from sunerf_hip import lib as _l
    rset = rc.response_set()
    m, nodes = rset.n_channels, rset.n_nodes
    query = _l.load().sunerf_dt_response_bwd_lds_bytes
    assert nodes == 1005 and rset.max_samples(8) == 605
    for s, w in ((605, 8), (606, 8), (606, 1), (3, 1)):
        assert query(s, w, nodes) == (200 + 2 * nodes + 8 * s * w) * 4 == rset.bwd_lds_bytes(s, w)
    assert query(605, 8, nodes) <= 160 * 1024 < query(606, 8, nodes)
    assert rset.fits(605, 8) and not rset.fits(606, 8) and rset.fits(606, 1)

    c = rc.make_case(9, 606, 8, 'generic', seed=2)
    for entry in ('sunerf_dt_response_bwd', 'sunerf_dt_response_bwd_full'):
        small = torch.full((m + 2,), float('nan'), device='cuda')
        status, g_raw = _bwd_raw(ops, c, rset, 9, (small[:m], small[m:m + 1], small[m + 1:]), entry)
        torch.cuda.synchronize()
        assert status == -2
        assert bool(torch.isnan(small).all()) and bool(torch.isnan(g_raw).all()), 'outputs written although the call was refused'
    with pytest.raises(ValueError, match='LDS'):           # the wrapper says which S fit before it calls
        ops.dt_response_bwd(*dev_args(c, rset), c['g_image'].cuda(), None)
    with pytest.raises(ValueError, match='LDS'):
        ops.dt_response_bwd_full(*dev_args(c, rset), c['g_image'].cuda(), None, None, None)
    # one sample fewer runs at W = 8, and the refused S runs at W = 1
    ok = {k: (v[:, :605].contiguous() if k in ('raw', 'z', 'inf') else v) for k, v in c.items()}
    ok['s'] = 605
    one = dict(c, w=1, wl=c['wl'][:, :1].contiguous(), g_image=c['g_image'][:, :1].contiguous())
    for case in (ok, one):
        g_raw, g_la, g_vc, _ = ops.dt_response_bwd(*dev_args(case, rset), case['g_image'].cuda(), None)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(g_raw).all()) and bool(torch.isfinite(g_la).all())
    f = ops.dt_response_fwd(*dev_args(c, rset))                     # the forward has no LDS that grows with S
    torch.cuda.synchronize()
    assert bool(torch.isfinite(f['image']).all())


# ---- 4. module level ----------------------------------------------------------------------------------------------------------
N_C = N_F = 16
STAR_ABSORPTION = {str(code): (i + 1) * 1e-9 for i, code in enumerate(rc.CODES)}      # g9's size: optical depths below 1
NERF_ABSORPTION = {str(code): v * 1e-6 for code, v in zip(rc.CODES, (2, 4, -1, 3, 5, 1, 2, 3, 1.5, 2.5, 4))}


def _rendering(model, g, response_set=None, model_config=None, trainer=False, cls=None):
    from sunerf.model.sunerf import DensityTemperatureSuNeRFModule
    from sunerf.rendering.density_temperature import DensityTemperatureRadiativeTransfer
    kw = dict(Rs_per_ds=1.0, model=model, model_config=dict(model_config or {}),
              sampling_config={'type': 'stratified', 'n_samples': N_C, 'perturb': False},
              hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': N_F},
              pixel_intensity_factor=float(g['pixel_intensity_factor']))
    if response_set is not None:
        kw['response_set'] = response_set
    else:
        kw['response_table'] = (g['aia_logte'].numpy(), g['aia_tresp'].numpy())
    if trainer:
        return DensityTemperatureSuNeRFModule(seconds_per_dt=1.0, image_scaling_config={}, **kw)
    return (cls or DensityTemperatureRadiativeTransfer)(**kw)


def _g6_mlp(mod, g, all_grids=False):
    """g6's trained-like MLP weights into both models of ``mod`` (its absorption scalars only where the names exist).
    ``all_grids``: g6's second output lies in [-0.19, -0.03] (coarse) and [0.48, 0.58] (fine) around its rays; the out layers
    times 2 and base temperatures of 6.7 and 5.45 put log T at 6.3 ... 6.65 in both models, inside every grid of the 11-channel
    set (the hot channel starts at 6.25, the 2-node grid ends at 7.0)."""
    sd = {k[4:].replace('__', '.'): v for k, v in g.items() if k.startswith('sd__')}
    own = mod.state_dict()
    mod.load_state_dict({k: v for k, v in sd.items() if k in own}, strict=False)
    if all_grids:
        with torch.no_grad():
            for m, base in ((mod.coarse_model, 6.7), (mod.fine_model, 5.45)):
                m.out_layer.weight.mul_(2.0)
                m.out_layer.bias.mul_(2.0)
                m.base_log_temperature = base


def _rays(n_rows=8, res=64):
    from sunerf_hip.rays import observer_rays
    o, d = observer_rays(res, row_start=(res - n_rows) // 2, row_end=(res + n_rows) // 2, device='cuda')
    t = torch.rand(o.shape[0], 1, generator=torch.Generator().manual_seed(5)).cuda()
    return o, d, t


def _mixed_rows(n, w=8, seed=9):
    """Wavelength rows that mix both instruments: AIA codes and the four new ones in every row, permuted per ray, with absent
    and unknown entries."""
    gen = torch.Generator().manual_seed(seed)
    codes = torch.tensor(rc.CODES, dtype=torch.float32)
    new = codes[7:][torch.argsort(torch.rand(n, 4, generator=gen), -1)]
    old = codes[:7][torch.argsort(torch.rand(n, 7, generator=gen), -1)[:, :w - 4]]
    wl = torch.cat([old, new], -1)
    wl = wl.gather(1, torch.argsort(torch.rand(n, w, generator=gen), -1))
    m = torch.rand(n, w, generator=gen)
    wl = torch.where(m < 0.05, torch.zeros(()), wl)
    wl = torch.where((m >= 0.05) & (m < 0.08), torch.tensor(rc.UNKNOWN), wl)
    return wl.contiguous()


def test_aia_response_set_renders_the_default_bits():
    from sunerf.model.model import NeRF_DT
    from sunerf_hip.response import ResponseSet
    g = load_golden('g6_dt_e2e')
    rset = ResponseSet.aia((g['aia_logte'].numpy(), g['aia_tresp'].numpy()), exposure=2.9)
    default = _rendering(NeRF_DT, g, model_config={'d_filter': 64})
    with_set = _rendering(NeRF_DT, g, rset, model_config={'d_filter': 64})
    assert torch.equal(torch.as_tensor(rset.table(2)[1]), default.response_table[2])
    for mod in (default, with_set):
        _g6_mlp(mod, g)
    assert all(torch.equal(a, b) for a, b in zip(default.state_dict().values(), with_set.state_dict().values()))
    default, with_set = default.cuda(), with_set.cuda()
    args = tuple(g[k].cuda() for k in ('rays_o', 'rays_d', 'times', 'wavelengths'))
    outs = []
    for mod in (default, with_set):
        torch.manual_seed(3)
        with torch.no_grad():
            outs.append(mod(*args))
    for k in outs[0]:
        assert torch.equal(outs[0][k].view(torch.int32), outs[1][k].view(torch.int32)), k
    assert gate_units(outs[1]['fine_image'], g['out__fine_image']) <= 1.0


def test_generic_hook_path_takes_the_set():
    """A subclass that replaces a hook renders through ``SuNeRFRendering.forward`` -> ``_render`` -> ``raw2outputs``: both
    accept the set, give the fused path's image and carry the gradient to the new channels' scalars."""
    from sunerf.model.model import NeRF_DT
    from sunerf.rendering.density_temperature import DensityTemperatureRadiativeTransfer

    class Hooked(DensityTemperatureRadiativeTransfer):
        def regularization(self, distance, regularizing_quantity):
            return super().regularization(distance, regularizing_quantity)

    g = load_golden('g6_dt_e2e')
    rset = rc.response_set()
    config = {'d_filter': 64, 'channels': rset}
    fused = _rendering(NeRF_DT, g, rset, model_config=config)
    hooked = _rendering(NeRF_DT, g, rset, model_config=config, cls=Hooked)
    _g6_mlp(fused, g, all_grids=True)
    _g6_mlp(hooked, g, all_grids=True)
    assert all(torch.equal(a, b) for a, b in zip(fused.state_dict().values(), hooked.state_dict().values()))
    fused, hooked = fused.cuda(), hooked.cuda()
    assert hooked._hooks_replaced(DensityTemperatureRadiativeTransfer) and not fused._hooks_replaced(DensityTemperatureRadiativeTransfer)
    o, d, t = _rays(2)
    wl = _mixed_rows(o.shape[0]).cuda()
    with torch.no_grad():
        a = fused(o, d, t, wl)
    b = hooked(o, d, t, wl)
    assert bool((a['fine_image'][wl == 174.] != 0).any())
    for k in ('coarse_image', 'fine_image'):
        assert gate_units(b[k], a[k].cpu()) <= 1.0, k
    b['fine_image'].sum().backward()
    for code in rc.NEW_CODES:
        grad = hooked.fine_model.log_absortpion[str(code)].grad
        assert grad is not None and grad.item() != 0, code
    # raw2outputs called by hand on the state the model answers
    z = fused.sampler.z_vals(o, d)
    query = torch.cat([o[:, None, :] + d[:, None, :] * z[:, :, None], t[:, None].repeat(1, z.shape[1], 1)], -1)
    with torch.no_grad():
        state = fused.coarse_model(query.view(-1, 4))
        state['inferences'] = state['inferences'].reshape(*z.shape, 2)
        out = fused.raw2outputs(**state, z_vals=z, rays_d=d, wavelengths=wl)
    assert gate_units(out['image'], a['coarse_image'].cpu()) <= 1.0


def _own_raw(rendering, model, o, d, t, z):
    """The raw (N, S, 2) of ``model`` at the samples, with its base offsets added in fp32: what the pass integrates."""
    from sunerf.rendering import functional as F
    with torch.no_grad():
        if hasattr(model, 'field_on_rays'):
            raw = F._field_raw(model, o, d, z, t)
        else:
            raw = F.mlp_on_rays(model, o, d, t, z)
        return torch.stack([raw[..., 0] + model.base_log_density, raw[..., 1] + model.base_log_temperature], -1).cpu()


def _image_of_raw(inf, model, z, wl, channels, pixel, dtype):
    la = [model.log_absortpion[str(code)].detach().cpu().to(dtype) for code, *_ in channels]
    chans = [(code, x.to(dtype), y.to(dtype)) for code, _, x, y in channels]
    with torch.no_grad():
        return rr.dt_integral(inf.to(dtype), la, model.volumetric_constant.detach().cpu().to(dtype), z.cpu().to(dtype),
                              wl.cpu().to(dtype), chans, pixel)['image']


@pytest.mark.parametrize('kind', ['nerf_dt', 'simple_star'])
def test_training_step_on_two_instruments(kind):
    """One training step on 512 rays whose rows mix AIA and the second instrument, ``channels=`` the 11 codes: the images
    against the restatement on the pass's own raw (the gate), every parameter gradient against the CPU restatement's autograd
    over the same composition of passes to 1e-3 per tensor (the bound of test_gpu_dt.py / test_gpu_simple_star_grad.py), and the
    four new channels' scalars with non-zero gradients."""
    import sunerf_oracle as orc
    from sunerf.model.model import NeRF_DT
    from sunerf.model.stellar_model import SimpleStar
    g = load_golden('g6_dt_e2e' if kind == 'nerf_dt' else 'g9_simple_star')
    rset = rc.response_set()
    channels = rc.channels()
    pixel = float(g['pixel_intensity_factor'])
    if kind == 'nerf_dt':
        lm = _rendering(NeRF_DT, g, rset, {'d_filter': 64, 'channels': rc.CODES}, trainer=True)
        _g6_mlp(lm.rendering, g, all_grids=True)
        absorption = NERF_ABSORPTION
    else:
        # T0 = 2.5e6 K (log T 6.4 beyond Rs) lights the hot channel, whose grid starts at 6.25.  R_s = 1.1: from 215 radii away
        # the fp32 sample positions carry 1.5e-5 radii of rounding, 8e-4 of the default ramp's width (1 ... 1.02 radii), and
        # the temperature of a sample on the ramp with it; where the ramp crosses a steep response (304 peaks at log T 4.9)
        # that noise of both sides, not the integral, is what a gradient comparison at 1e-3 would measure (1.1e-3 measured
        # on the 304 scalar at R_s = 1.02, with either side's sample placement).  A ramp five times as wide keeps it below.
        lm = _rendering(SimpleStar, g, rset, {'channels': rc.CODES, 'T0': 2.5e6, 'R_s': 1.1}, trainer=True)
        absorption = STAR_ABSORPTION
    rnd = lm.rendering
    with torch.no_grad():
        for m in (rnd.coarse_model, rnd.fine_model):
            assert tuple(m.log_absortpion.keys()) == rset.keys
            for k, v in absorption.items():
                m.log_absortpion[k].fill_(v)
        rnd.fine_model.log_absortpion['10171'].mul_(1.5)      # the two models differ: a gradient in the wrong instance shows
        if kind == 'simple_star':
            rnd.fine_model.stellar_parameters['h0'].mul_(1.05)
            rnd.fine_model.stellar_parameters['T0'].mul_(0.97)
            for m in (rnd.coarse_model, rnd.fine_model):
                m.volumetric_constant.copy_(g['vol_c'])
    lm = lm.cuda()
    o, d, t = _rays(8)
    n = o.shape[0]
    assert n == 512
    wl = _mixed_rows(n).cuda()

    # ---- the sample positions of the step (deterministic: perturb off), then the CPU restatement of the whole step on them,
    # fp32, with autograd
    with torch.no_grad():
        out = rnd(o, d, t, wl)
    z_c = out['z_vals_stratified']
    z_f = torch.sort(torch.cat([z_c, out['z_vals_hierarchical']], -1), -1).values
    leaf = lambda p: p.detach().cpu().clone().requires_grad_(True)      # noqa: E731
    leaves = {name: leaf(p) for name, p in rnd.named_parameters()}
    fields, heads = [], []
    for prefix, model in (('coarse_model.', rnd.coarse_model), ('fine_model.', rnd.fine_model)):
        heads.append(([leaves[f'{prefix}log_absortpion.{k}'] for k in rset.keys], leaves[prefix + 'volumetric_constant']))
        if kind == 'nerf_dt':
            params = orc.params_from_state_dict(leaves, prefix)
            base = torch.tensor([model.base_log_density, model.base_log_temperature])

            def field(pts, times, params=params, base=base):
                q = torch.cat([pts, times[:, None].repeat(1, pts.shape[1], 1)], -1)
                return (orc.mlp_forward(params, q.view(-1, 4)) + base).reshape(*pts.shape[:-1], 2)
        else:
            sp = {k: leaves[f'{prefix}stellar_parameters.{k}'] for k in ('Rs', 'h0', 'T0', 'rho_0')}

            def field(pts, times, sp=sp):
                return orc.simple_star_field(pts.reshape(-1, 3), sp['rho_0'], sp['h0'], sp['T0'], sp['Rs']).reshape(*pts.shape[:-1], 2)
        fields.append(field)
    want = rr.render(fields, heads, o.cpu(), d.cpu(), t.cpu(), wl.cpu(), channels, N_C, N_F, pixel,
                     t_vals=rnd.sampler.t_vals.detach().cpu(), z_given=(z_c.cpu(), z_f.cpu()))
    assert torch.equal(want['z_vals_stratified'], z_c.cpu())
    target = (want['fine_image'] * 0.8).detach()
    mse = torch.nn.functional.mse_loss
    ref_loss = mse(want['coarse_image'], target) + mse(want['fine_image'], target) + want['regularization'].mean()
    ref_loss.backward()

    batch = {'tracing': {'rays': torch.stack([o, d], 1), 'time': t, 'target_image': target.cuda(), 'wavelength': wl}}
    loss = lm.training_step(batch, 0)
    assert abs(loss.item() - ref_loss.item()) < 2e-4 * abs(ref_loss.item()), (loss.item(), ref_loss.item())
    loss.backward()

    # ---- images against the restatement on the passes' own raw
    for key, model, z in (('coarse_image', rnd.coarse_model, z_c), ('fine_image', rnd.fine_model, z_f)):
        inf = _own_raw(rnd, model, o, d, t, z)
        i64, i32 = (_image_of_raw(inf, model, z, wl, channels, pixel, dt_) for dt_ in (torch.float64, torch.float32))
        units = gate_units(out[key], i64, floor=2 * (i32.double() - i64).abs())
        print(f'{kind} {key}: {units:.3f} gate units against the restatement on the pass\'s own raw')
        assert units <= 1.0, (key, units)
        known = torch.isin(wl.cpu(), torch.tensor(rc.CODES, dtype=torch.float32))
        assert bool((out[key].cpu()[~known] == 0).all())
        for code in rc.CODES:
            assert bool((out[key].cpu()[wl.cpu() == float(code)] != 0).any()), (key, code)

    # ---- gradients
    worst = {}
    for name, p in rnd.named_parameters():
        ref = leaves[name].grad
        assert ref is not None and p.grad is not None, name
        got = p.grad.detach().cpu()
        if ref.abs().max() == 0:
            assert got.abs().max() == 0, name
            continue
        worst[name] = ((got.double() - ref.double()).norm() / ref.double().norm()).item()
    print(f'{kind}: worst gradient ' + ', '.join(f'{k} {v:.2e}' for k, v in sorted(worst.items(), key=lambda kv: -kv[1])[:4]))
    bad = {k: v for k, v in worst.items() if not v < 1e-3}
    assert not bad, bad
    for prefix in ('coarse_model.', 'fine_model.'):
        for code in rc.NEW_CODES:
            assert dict(rnd.named_parameters())[f'{prefix}log_absortpion.{code}'].grad.item() != 0, (prefix, code)


def test_code_174_renders_with_the_set_and_not_without():
    """The gap, pinned from both sides: a row that holds code 174 renders a non-zero image against the set and exactly 0 in the
    default rendering (which knows the seven AIA wavelengths only)."""
    from sunerf.model.stellar_model import SimpleStar
    g = load_golden('g9_simple_star')
    default = _rendering(SimpleStar, g).cuda()
    with_set = _rendering(SimpleStar, g, rc.response_set(), {'channels': rc.CODES}).cuda()
    with torch.no_grad():
        for mod in (default, with_set):
            for m in (mod.coarse_model, mod.fine_model):
                for p in m.log_absortpion.values():
                    p.fill_(2e-9)
        o, d, t = _rays(2)
        wl = torch.tensor([174., 171.]).repeat(o.shape[0], 1).cuda()
        a, b = default(o, d, t, wl), with_set(o, d, t, wl)
    assert bool((a['image'][:, 0] == 0).all()) and bool((a['coarse_image'][:, 0] == 0).all())
    assert bool((a['image'][:, 1] > 0).any())
    assert bool((b['image'][:, 0] > 0).any()) and bool((b['coarse_image'][:, 0] > 0).any())
    assert torch.equal(a['image'][:, 1], b['image'][:, 1])          # AIA's 171 row is the same row in both


def test_snf_round_trip_renders_the_same_bits(tmp_path):
    from sunerf.evaluation.loader import SuNeRFLoader
    from sunerf.model.model import NeRF_DT
    from sunerf.model.sunerf import save_state
    g = load_golden('g6_dt_e2e')
    rset = rc.response_set()
    rendering = _rendering(NeRF_DT, g, rset, {'d_filter': 64, 'channels': rset})
    _g6_mlp(rendering, g, all_grids=True)
    rendering = rendering.cuda()

    class _Module:
        pass

    class _Data:
        config = {'wavelength': None, 'times': [datetime.datetime(2022, 1, 1), datetime.datetime(2022, 1, 3)],
                  'resolution': (16, 16), 'wcs': {'shape': (16, 16), 'cdelt': (150., 150.)}}
        Rs_per_ds, seconds_per_dt, ref_time = 1.0, 86400., datetime.datetime(2022, 1, 1)
    holder = _Module()
    holder.rendering = rendering
    path = str(tmp_path / 'run' / 'save_state.snf')
    save_state(holder, _Data(), path)
    loader = SuNeRFLoader(path, device='cuda')
    assert loader.rendering.response_set == rset and 'response' not in loader.rendering.__dict__
    o, d, t = _rays(2)
    wl = _mixed_rows(o.shape[0]).cuda()
    with torch.no_grad():
        a, b = rendering(o, d, t, wl), loader.rendering(o, d, t, wl)
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    assert bool((a['image'] != 0).any())
