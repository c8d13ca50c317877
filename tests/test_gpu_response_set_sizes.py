"""The response-set kernels (csrc/dt_response_set.hip) at the limits their header states -- 1 ... 64 channels, 4096 nodes -- where
tests/test_gpu_response_set.py runs them on 11 channels and 1005 nodes only.  What these sizes reach: the second code of a
lane in the lookup (rows 32 ... 63), every per-row index (offsets, log_abs, the LDS accumulators, the g_vol slot beside
accumulator 63), M = 1 and M = 32 | 33, 16 staging trips per thread, a binary search of depth 12, the slab base behind 8192
floats of tables, and the > 64 KiB launch and the 160 KiB refusal reached through the node count.

The sets (tests/response_set_cases.py) are ROUGH: non-uniform grids and responses drawn node by node over a decade, so that a
sample resolved to the neighbouring interval or to another row is off by O(1); tests/test_response_set_host.py shows that a
lookup reading row m - 32 for m >= 32 fails every case with M >= 33, and that the fp32 restatement alone stays within a quarter
of every bound with the bounds' noise terms removed.  Tried once on an MI355X: a library whose lookup takes the absorption of row
m mod 32 passes every test of tests/test_gpu_response_set.py and fails 18 of the 25 here.

1. ``SIZE_CASES`` against the fp64 restatement (tests/response_set_reference.py), exactly as
   ``test_gpu_response_set.test_response_kernels_against_fp64`` runs its cases, with the project's bounds unchanged.  Worst
   values measured on an MI355X over all cases of this file:
     image            gate_units vs fp64, floor 2 |ref32 - ref64|                                  <= 1      (0.014)
                      absent columns exactly 0: 0, -1, 1600, NaN, +Inf, code + 0.5, 2^24, 1e-40
     reg_q            bit-identical to the fp32 expression
     weights          1e-5 relative per element                                                    (1.7e-7)
     height_map       1e-5 relative per ray                                                        (1.9e-7)
     absorption_map   1e-5 of sum_s |1 - q_s| per ray                                              (1.3e-7)
     g_raw            per ray, test_gpu_dt_integral.ray_units (image-only and full backward)       <= 1      (0.0095 / 0.0065)
                      exactly 0 behind a closed relu
     g_log_abs, g_vol_c   SCALAR_GRADIENT_REL = 1e-4 relative, each of the up to 64 scalars        (8.7e-7 / 1.2e-7, two runs)
                      g_log_abs exactly 0 where log_abs <= 0 or the channel is absent from every ray
   Forward outputs and g_raw are bit-identical across reruns; the absmax word is max |g_raw|; a NaN or Inf column leaves every
   output finite.
2. 8200 rays (1025 groups: the grid-stride walk) of the 64-channel set by bits against the 72 rays they repeat, the scalar
   gradients against 113 x the fp64 gradient of the 72 rays + that of the first 64 (g_log_abs 5.2e-6, g_vol_c 9.7e-7, three runs).
3. The 11-channel set inside a 64-channel one, in another order: the bits of the 11-channel call (g_log_abs within 1.1e-7 of it).
4. The LDS limit at 4096 nodes (508 samples run, 509 are refused) and the empty batch at M = 64.
5. The module path: one training step of ``NeRF_DT`` on 64 channels (images 0.002 / 0.002 gate units against the restatement on
   the passes' own raw, worst parameter gradient 2.3e-4 of its tensor), folded ``render_dem`` against ``forward``'s image for 40
   non-AIA channels on one grid (NeRF_DT 0.003 / 0.002 gate units thin / attenuated, SimpleStar 0.003 / 0.003), ``invert_dem`` on
   eight of them, and the ``.snf`` round trip of a 64-channel rendering.
"""
import datetime

import numpy as np
import pytest
import torch

import response_set_cases as rc
import response_set_reference as rr
import test_gpu_dt_integral as dt
import test_gpu_response_set as rs
from conftest import gate_units, load_golden

pytestmark = pytest.mark.gpu

SCALAR_GRADIENT_REL = dt.SCALAR_GRADIENT_REL
_REFS = {}


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    from sunerf_hip import ops as _ops
    return _ops


def refs(shape):
    """(fp64, fp32) restatement of a case of ``SIZE_CASES``: computed once, shared, left unchanged."""
    if shape not in _REFS:
        c, channels = rc.size_case(*shape), list(rc.set_channels(shape[0]))
        _REFS[shape] = (rr.oracle(c, channels, torch.float64), rr.oracle(c, channels, torch.float32))
    return _REFS[shape]


def _present(c, codes):
    return torch.tensor([bool((c['wl'] == float(code)).any()) for code in codes])


# ---- 1. kernels against fp64 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', rc.SIZE_CASES, ids=[rc.size_case_id(s) for s in rc.SIZE_CASES])
def test_size_cases_against_fp64(ops, shape):
    name, n, s, w, base = shape
    c = rc.size_case(*shape)
    channels = list(rc.set_channels(name))
    codes = [ch[0] for ch in channels]
    args = rs.dev_args(c, rc.set_of(name))
    g_img = c['g_image'].cuda()
    f, f_again = (ops.dt_response_fwd(*args, want_epilogues=True) for _ in range(2))
    bwd, bwd_again = (ops.dt_response_bwd(*args, g_img, None) for _ in range(2))
    ref64, ref32 = refs(shape)
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
    # a NaN or an Inf in a wavelengths row is an absent column and nothing more: no output of any ray is touched by it
    assert bool(torch.isnan(c['wl']).any()) and bool(torch.isinf(c['wl']).any())
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), f'{k} is not finite'
    for again in (bwd_again, full_again):
        assert bool(torch.isfinite(again[1]).all()) and bool(torch.isfinite(again[2]).all())
    full64 = ref64['g_raw'] + rr.rest_gradient(c, rest, torch.float64)
    full32 = ref32['g_raw'] + rr.rest_gradient(c, rest, torch.float32)
    m = rr.measure(got, c, codes, ref64, ref32, full64, full32)
    # the second run's scalar gradients (float atomics: the order of the adds is free) are held as the first's
    la_zero = (c['log_abs'] <= 0) | ~_present(c, codes)
    for tag, again in (('', bwd_again), ('_full', full_again)):
        m['g_log_abs' + tag + '_again'] = dt.scalar_rel(again[1], ref64['g_log_abs'], la_zero)
        m['g_vol_c' + tag + '_again'] = dt.scalar_rel(again[2], ref64['g_vol_c'], torch.zeros(1, dtype=torch.bool))
    print(f'{rc.size_case_id(shape)}: ' + ' '.join(f'{k} {v:.2e}' for k, v in m.items()))
    rr.assert_bounds(m, SCALAR_GRADIENT_REL)


# ---- 2. the grid-stride walk on 64 channels -------------------------------------------------------------------------------
def test_grid_stride_walk_on_64_channels(ops):
    """8200 rays = 1025 groups of 8, one more than the backward's grid: ray ``i`` is ray ``i mod 72`` of the 72-ray case.  The
    per-ray outputs have the bits of the 72-ray call; the scalar gradients are 113 times those of the 72 rays plus those of the
    first 64 (8200 = 113 x 72 + 64), taken from the fp64 restatement: no oracle of 8200 rays is needed."""
    shape = ('R64', 72, 33, 8, 'generic')
    c = rc.size_case(*shape)
    channels = list(rc.set_channels('R64'))
    codes = [ch[0] for ch in channels]
    rset = rc.set_of('R64')
    ref64, _ = refs(shape)
    n_big = 8200
    assert (n_big + 7) // 8 == 1025 and n_big == 113 * 72 + 64
    idx = torch.arange(n_big) % 72
    rest = dt.make_rest(c, ref64)
    per_ray = ('raw', 'z', 'o', 'd', 'wl', 'g_image', 'inf')
    big = dict(c, n=n_big, **{k: c[k][idx].contiguous() for k in per_ray})
    head = dict(c, n=64, **{k: c[k][:64].contiguous() for k in per_ray})
    g64 = rr.oracle(head, channels, torch.float64)
    want_la = 113 * ref64['g_log_abs'] + g64['g_log_abs']
    want_vc = 113 * ref64['g_vol_c'] + g64['g_vol_c']
    la_zero = (c['log_abs'] <= 0) | ~_present(c, codes)
    assert int((~la_zero).sum()) >= 50 and bool((want_la[~la_zero] != 0).all())

    out = {}
    for tag, case, r in (('small', c, rest), ('big', big, {k: v[idx].contiguous() for k, v in rest.items()})):
        args = rs.dev_args(case, rset)
        g_img = case['g_image'].cuda()
        rd = {k: v.cuda() for k, v in r.items()}
        out[tag] = (ops.dt_response_fwd(*args, want_epilogues=True), ops.dt_response_bwd(*args, g_img, None),
                    ops.dt_response_bwd_full(*args, g_img, rd['g_reg'], rd['g_weights'], rd['g_reg_q']))
    torch.cuda.synchronize()
    (f_s, b_s, full_s), (f_b, b_b, full_b) = out['small'], out['big']
    dev_idx = idx.cuda()
    for k in f_s:
        assert torch.equal(f_b[k].view(torch.int32), f_s[k][dev_idx].view(torch.int32)), f'forward {k}'
    assert bool((f_b['image'] != 0).any())
    worst = {}
    for what, small, large in (('bwd', b_s, b_b), ('bwd_full', full_s, full_b)):
        assert torch.equal(large[0].view(torch.int32), small[0][dev_idx].view(torch.int32)), f'g_raw of {what}'
        assert torch.equal(large[3], small[3]), f'absmax of {what}'
        worst[what + ' g_log_abs'] = dt.scalar_rel(large[1], want_la, la_zero)
        worst[what + ' g_vol_c'] = dt.scalar_rel(large[2], want_vc, torch.zeros(1, dtype=torch.bool))
    print('8200 rays on R64: ' + ' '.join(f'{k} {v:.2e}' for k, v in worst.items()))
    assert max(worst.values()) <= SCALAR_GRADIENT_REL, worst


# ---- 3. embedding invariance ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,s,w,base', [(9, 33, 8, 'generic'), (9, 300, 8, 'generic'), (7, 33, 3, 'nerf_dt')])
def test_a_channel_does_not_depend_on_the_rest_of_its_set(ops, n, s, w, base):
    """The 11 channels as rows 53 ... 63 of a 64-channel set, in another order, behind 53 rough filler channels with positive
    absorption: all three entry points give the bits of the 11-channel call, and the filler rows no gradient."""
    from sunerf_hip.response import ResponseSet
    c = rc.group1_case(n, s, w, base)
    small_set, big_set = rc.response_set(), ResponseSet(list(rc.embedded_channels()))
    rows = [53 + rc.EMBED_PERM.index(p) for p in range(11)]                  # where channel p of the 11 sits
    la = torch.full((64,), 0.5 * float(c['log_abs'].abs().max()))
    la[rows] = c['log_abs']
    e = dict(c, log_abs=la)
    gen = torch.Generator().manual_seed(s)
    extra = [(0.5 - torch.rand(n, s, generator=gen)).cuda() for _ in range(3)]
    g_img = c['g_image'].cuda()
    res = []
    for case, rset in ((c, small_set), (e, big_set)):
        args = rs.dev_args(case, rset)
        res.append((ops.dt_response_fwd(*args, want_epilogues=True), ops.dt_response_bwd(*args, g_img, extra[0]),
                    ops.dt_response_bwd(*args, g_img, None), ops.dt_response_bwd_full(*args, g_img, *extra)))
    torch.cuda.synchronize()
    (f_a, *bwd_a), (f_b, *bwd_b) = res
    assert set(f_a) == set(f_b) == {'image', 'weights', 'reg_q', 'height_map', 'absorption_map', 'regularization'}
    for k in f_a:
        assert torch.equal(f_a[k].view(torch.int32), f_b[k].view(torch.int32)), f'forward {k}'
    assert bool((f_a['image'] != 0).any())
    worst = 0.0
    for i, (a, b) in enumerate(zip(bwd_a, bwd_b)):
        assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)), f'g_raw of backward {i}'
        assert torch.equal(a[3], b[3]), f'absmax of backward {i}'
        assert b[1].shape == (64,) and bool((b[1][:53] == 0).all()), f'filler rows of backward {i} have a gradient'
        ref = a[1].cpu().double()
        worst = max(worst, dt.scalar_rel(b[1][rows], ref, ref == 0))
        ref = a[2].cpu().double()
        worst = max(worst, dt.scalar_rel(b[2], ref, ref.reshape(-1) == 0))
    print(f'N={n} S={s} W={w} {base} embedded: scalar gradients within {worst:.2e} of the 11-channel call')
    assert worst <= SCALAR_GRADIENT_REL


# ---- 4. the LDS limit through the tables, the empty batch ---------------------------------------------------------------------
def test_lds_limit_reached_through_the_node_count(ops):
    """With 4096 nodes 508 samples x 8 columns need 163 616 B and run (the (9, 508, 8) case above, held to fp64); 509 need
    163 872 B, more than a CU's 160 KiB: SUNERF_E_UNSUPPORTED before anything is queued, nothing written.  The 11-channel set
    takes 605."""
    from sunerf_hip import lib as _l
    rset = rc.set_of('R64')
    m, nodes = rset.n_channels, rset.n_nodes
    query = _l.load().sunerf_dt_response_bwd_lds_bytes
    assert (m, nodes) == (64, 4096) and rset.max_samples(8) == 508
    for s in (508, 509):
        assert query(s, 8, nodes) == (200 + 2 * 4096 + 8 * s * 8) * 4 == rset.bwd_lds_bytes(s, 8)
        assert ops.dt_response_bwd_lds_bytes(s, 8, nodes) == query(s, 8, nodes)
    assert query(508, 8, nodes) <= 160 * 1024 < query(509, 8, nodes)
    assert rset.fits(508, 8) and not rset.fits(509, 8)
    assert ('R64', 9, 508, 8, 'generic') in rc.SIZE_CASES

    c = rc.make_case(9, 509, 8, 'generic', seed=2, channels=list(rc.set_channels('R64')))
    for entry in ('sunerf_dt_response_bwd', 'sunerf_dt_response_bwd_full'):
        small = torch.full((m + 2,), float('nan'), device='cuda')
        status, g_raw = rs._bwd_raw(ops, c, rset, 9, (small[:m], small[m:m + 1], small[m + 1:]), entry)
        torch.cuda.synchronize()
        assert status == -2
        assert bool(torch.isnan(small).all()) and bool(torch.isnan(g_raw).all()), 'outputs written although the call was refused'
    with pytest.raises(ValueError, match='LDS'):
        ops.dt_response_bwd(*rs.dev_args(c, rset), c['g_image'].cuda(), None)
    with pytest.raises(ValueError, match='LDS'):
        ops.dt_response_bwd_full(*rs.dev_args(c, rset), c['g_image'].cuda(), None, None, None)
    f = ops.dt_response_fwd(*rs.dev_args(c, rset))                  # the forward has no LDS that grows with S
    torch.cuda.synchronize()
    assert bool(torch.isfinite(f['image']).all()) and bool((f['image'] != 0).any())


def test_empty_batch_clears_64_scalars(ops):
    """n_rays = 0 at M = 64 clears g_log_abs [64], g_vol_c and the absmax word, in one buffer or in three."""
    rset = rc.set_of('R64')
    m = rset.n_channels
    channels = list(rc.set_channels('R64'))
    c = rc.make_case(1, 33, 8, 'generic', seed=1, channels=channels)
    for entry in ('sunerf_dt_response_bwd', 'sunerf_dt_response_bwd_full'):
        joint = torch.full((m + 2,), float('nan'), device='cuda')
        assert rs._bwd_raw(ops, c, rset, 0, (joint[:m], joint[m:m + 1], joint[m + 1:]), entry)[0] == 0
        apart = [torch.full((k,), float('nan'), device='cuda') for k in (m, 1, 1)]
        assert rs._bwd_raw(ops, c, rset, 0, apart, entry)[0] == 0
        torch.cuda.synchronize()
        assert m == 64 and bool((joint == 0).all()), joint
        assert all(bool((t == 0).all()) for t in apart), apart
    e = rc.make_case(0, 33, 8, 'generic', seed=1, channels=channels)
    out = ops.dt_response_bwd(*rs.dev_args(e, rset), torch.zeros(0, 8, device='cuda'), None)
    f = ops.dt_response_fwd(*rs.dev_args(e, rset))
    torch.cuda.synchronize()
    assert out[0].numel() == 0 and out[1].shape == (64,) and bool((out[1] == 0).all()) and bool((out[2] == 0).all()) \
        and out[3].item() == 0
    assert f['image'].shape == (0, 8)


# ---- 5. module level ----------------------------------------------------------------------------------------------------------
ABSORPTION_PATTERN = (2, 4, -1, 3, 5, 1, 2, 3, 1.5, 2.5, 4)       # x 1e-6, period 11: test_gpu_response_set.NERF_ABSORPTION


def _set_rows(n, codes, w=8, seed=9):
    """Rows built as the cases' are: ``base_rows``, a few absent and unknown entries, the odd values and the lane pairs."""
    gen = torch.Generator().manual_seed(seed)
    wl = rc.base_rows(n, w, codes)
    m = torch.rand(n, w, generator=gen)
    wl = torch.where(m < 0.05, torch.zeros(()), wl)
    wl = torch.where((m >= 0.05) & (m < 0.08), torch.tensor(rc.UNKNOWN), wl)
    return rc.set_rows(wl, codes)


def test_training_step_on_64_channels():
    """``test_gpu_response_set.test_training_step_on_two_instruments`` for ``NeRF_DT`` on 64 smooth channels, each on a grid of
    its own: the loss and both images against the CPU restatement, every parameter gradient -- the 2 x 64 absorption scalars
    among them, each a tensor of its own -- against the restatement's autograd to 1e-3, and a gradient on every positive
    scalar.  Coarse and fine differ on rows 40 and 63: a gradient in the wrong instance or the wrong row shows."""
    import sunerf_oracle as orc
    from sunerf.model.model import NeRF_DT
    from sunerf_hip.response import ResponseSet
    g = load_golden('g6_dt_e2e')
    channels = list(rc.smooth_channels_64())
    rset = ResponseSet(channels)
    codes = rset.codes
    pixel = float(g['pixel_intensity_factor'])
    lm = rs._rendering(NeRF_DT, g, rset, {'d_filter': 64, 'channels': rset}, trainer=True)
    rs._g6_mlp(lm.rendering, g, all_grids=True)
    rnd = lm.rendering
    with torch.no_grad():
        for m in (rnd.coarse_model, rnd.fine_model):
            assert tuple(m.log_absortpion.keys()) == rset.keys and len(rset.keys) == 64
            for i, k in enumerate(rset.keys):
                m.log_absortpion[k].fill_(ABSORPTION_PATTERN[i % 11] * 1e-6)
        rnd.fine_model.log_absortpion[rset.keys[40]].mul_(1.5)
        rnd.fine_model.log_absortpion[rset.keys[63]].mul_(0.5)
    lm = lm.cuda()
    o, d, t = rs._rays(8)
    n = o.shape[0]
    assert n == 512
    wl_host = _set_rows(n, codes)
    assert min(int((wl_host == float(code)).any(-1).sum()) for code in codes) >= 32
    assert bool(torch.isnan(wl_host).any()) and bool(torch.isinf(wl_host).any())
    wl = wl_host.cuda()

    with torch.no_grad():
        out = rnd(o, d, t, wl)
    z_c = out['z_vals_stratified']
    z_f = torch.sort(torch.cat([z_c, out['z_vals_hierarchical']], -1), -1).values
    leaf = lambda p: p.detach().cpu().clone().requires_grad_(True)      # noqa: E731
    leaves = {name: leaf(p) for name, p in rnd.named_parameters()}
    fields, heads = [], []
    for prefix, model in (('coarse_model.', rnd.coarse_model), ('fine_model.', rnd.fine_model)):
        heads.append(([leaves[f'{prefix}log_absortpion.{k}'] for k in rset.keys], leaves[prefix + 'volumetric_constant']))
        params = orc.params_from_state_dict(leaves, prefix)
        base = torch.tensor([model.base_log_density, model.base_log_temperature])

        def field(pts, times, params=params, base=base):
            q = torch.cat([pts, times[:, None].repeat(1, pts.shape[1], 1)], -1)
            return (orc.mlp_forward(params, q.view(-1, 4)) + base).reshape(*pts.shape[:-1], 2)
        fields.append(field)
    want = rr.render(fields, heads, o.cpu(), d.cpu(), t.cpu(), wl_host, channels, rs.N_C, rs.N_F, pixel,
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

    known = torch.isin(wl_host, torch.tensor(codes, dtype=torch.float32))
    for key, model, z in (('coarse_image', rnd.coarse_model, z_c), ('fine_image', rnd.fine_model, z_f)):
        inf = rs._own_raw(rnd, model, o, d, t, z)
        i64, i32 = (rs._image_of_raw(inf, model, z, wl, channels, pixel, dt_) for dt_ in (torch.float64, torch.float32))
        units = gate_units(out[key], i64, floor=2 * (i32.double() - i64).abs())
        print(f'64 channels {key}: {units:.3f} gate units against the restatement on the pass\'s own raw')
        assert units <= 1.0, (key, units)
        assert bool((out[key].cpu()[~known] == 0).all())
        for code in codes:
            assert bool((out[key].cpu()[wl_host == float(code)] != 0).any()), (key, code)

    worst = {}
    params = dict(rnd.named_parameters())
    for name, p in params.items():
        ref = leaves[name].grad
        assert ref is not None and p.grad is not None, name
        got = p.grad.detach().cpu()
        if ref.abs().max() == 0:
            assert got.abs().max() == 0, name
            continue
        worst[name] = ((got.double() - ref.double()).norm() / ref.double().norm()).item()
    print('64 channels: worst gradient ' + ', '.join(f'{k} {v:.2e}' for k, v in sorted(worst.items(), key=lambda kv: -kv[1])[:4]))
    bad = {k: v for k, v in worst.items() if not v < 1e-3}
    assert not bad, bad
    held = 0
    for prefix in ('coarse_model.', 'fine_model.'):
        for k in rset.keys:
            name = f'{prefix}log_absortpion.{k}'
            if params[name].item() > 0:
                assert params[name].grad.item() != 0 and name in worst, name
                held += 1
            else:
                assert params[name].grad.item() == 0, name
    assert held == 2 * (64 - 6)


def _dem_rendering(model, model_config, n_samples):
    from sunerf.rendering.density_temperature import DensityTemperatureRadiativeTransfer
    from sunerf_hip.response import ResponseSet
    g = load_golden('g6_dt_e2e' if 'd_filter' in model_config else 'g9_simple_star')
    rset = ResponseSet(list(rc.smooth_channels_40()))
    mod = DensityTemperatureRadiativeTransfer(
        Rs_per_ds=1.0, model=model, model_config=dict(model_config, channels=rset), response_set=rset,
        sampling_config={'type': 'stratified', 'n_samples': n_samples, 'perturb': False},
        hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': n_samples, 'perturb': False},
        pixel_intensity_factor=float(g['pixel_intensity_factor']))
    if 'd_filter' in model_config:
        rs._g6_mlp(mod, g)
    return mod.cuda(), rset


def _fill_absorption(mod, values):
    with torch.no_grad():
        for m in (mod.coarse_model, mod.fine_model):
            for p, v in zip(m.log_absortpion.values(), values):
                p.fill_(v)


def _image_of_all(mod, rset, o, d, t):
    """``forward``'s image of all 40 channels: five calls of eight columns."""
    cols = []
    with torch.no_grad():
        for a in range(0, 40, 8):
            wl = torch.tensor(rset.codes[a:a + 8], dtype=torch.float32, device='cuda').expand(o.shape[0], 8).contiguous()
            cols.append(mod(o, d, t, wl)['image'])
    return torch.cat(cols, -1)


def _dem_identity(mod, rset, what):
    """``test_gpu_dem._identity`` against a response set: the folded line-of-sight DEM (csrc/dem.hip and ``numpy.interp``, which
    share nothing with the response-set kernels) is the image of every channel, rows >= 32 included."""
    import test_gpu_dem as td
    from sunerf_hip import dem
    o, d, t = td._observer_rays()
    n = o.shape[0]
    factor = float(mod.fine_model.volumetric_constant.detach()) * mod.pixel_intensity_factor
    _fill_absorption(mod, [(-1e-3, 0.)[i % 2] for i in range(40)])
    image = _image_of_all(mod, rset, o, d, t)
    out = mod.render_dem(o, d, t)
    grid = rset.shared_grid()
    assert grid is not None and out['dem'].shape == (n, 100) and torch.equal(out['logt_nodes'].cpu(), torch.as_tensor(grid))
    assert bool((image > 0).any(0).all()) and bool((out['em'] > 0).all())
    on_nodes = rset.on_nodes(out['logt_nodes'])
    folded = dem.fold(out['dem'].double(), on_nodes.to(out['dem'].device)) * factor
    u = gate_units(folded, image.cpu())
    print(f'{what}: folded render_dem vs the image of 40 channels, optically thin, {u:.3f} gate units')
    assert folded.shape == (n, 40) and u <= 1.0, (what, u)
    row = 35
    code = rset.codes[row]
    tau1 = float(out['column'].max())
    _fill_absorption(mod, [1.0 / tau1 if i == row else 0. for i in range(40)])
    wl = torch.tensor(rset.codes[32:40], dtype=torch.float32, device='cuda').expand(n, 8).contiguous()
    with torch.no_grad():
        image_a = mod(o, d, t, wl)['image'][:, row - 32]
    out_a = mod.render_dem(o, d, t, attenuation_wavelength=code)
    assert bool((out_a['em'] < out['em']).all()) and td.same_bits(out_a['column'], out['column'])
    folded_a = dem.fold(out_a['dem'].double(), on_nodes[row].to(out['dem'].device)) * factor
    u = gate_units(folded_a, image_a.cpu())
    lit = image[:, row] > 0
    dimmed = (image_a[lit] / image[:, row][lit]).min().item()
    print(f'{what}: folded render_dem vs image, attenuated at row {row}, {u:.3f} gate units (dimmest ray x {dimmed:.2f})')
    assert u <= 1.0 and dimmed < 0.8, (what, u, dimmed)
    with pytest.raises(ValueError, match='not a channel'):
        mod.render_dem(o, d, t, attenuation_wavelength=1600)


def test_render_dem_folds_to_the_image_of_40_channels_nerf_dt(monkeypatch):
    from sunerf.model.model import NeRF_DT
    monkeypatch.setenv('SUNERF_FORWARD_PRECISION', 'exact')
    _dem_identity(*_dem_rendering(NeRF_DT, {'d_filter': 64}, 16), 'NeRF_DT d_filter 64')


def test_render_dem_folds_to_the_image_of_40_channels_simple_star():
    from sunerf.model.stellar_model import SimpleStar
    _dem_identity(*_dem_rendering(SimpleStar, {}, 24), 'SimpleStar')


def test_invert_dem_with_a_set():
    """Eight channels of the 40, five of them rows >= 32, inverted and folded back: the assertion of
    ``test_gpu_dem_inversion.test_through_the_model``; all 40 at once are refused as unsupported."""
    import test_gpu_dem as td
    import test_gpu_dem_inversion as ti
    from sunerf.model.stellar_model import SimpleStar
    from sunerf_hip import dem, dem_inversion
    mod, rset = _dem_rendering(SimpleStar, {}, 24)
    _fill_absorption(mod, [0.] * 40)
    o, d, t = td._observer_rays(17)
    n = o.shape[0]
    rows = [3, 33, 12, 39, 36, 20, 32, 35]
    codes = [rset.codes[r] for r in rows]
    assert sum(r >= 32 for r in rows) == 5
    wl = torch.tensor(codes, dtype=torch.float32, device='cuda').expand(n, 8).contiguous()
    with torch.no_grad():
        image = mod(o, d, t, wl)['image']
    out = mod.invert_dem(image, wavelengths=codes)
    assert out['dem'].shape == (n, 100) and torch.equal(out['logt_nodes'].cpu(), torch.as_tensor(rset.shared_grid()))
    status = out['status'].cpu().numpy()
    assert (status & 1 == 0).all()
    interior = (status & 0xff) == 0
    assert interior.sum() >= n // 2
    G = mod.inversion_response(codes)
    factor = float(mod.fine_model.volumetric_constant.detach()) * float(mod.pixel_intensity_factor)
    assert torch.equal(G.cpu(), rset.on_nodes(out['logt_nodes'])[rows] * factor)
    sigma = dem_inversion.default_errors(image).double()
    folded = dem.fold(out['dem'].double(), G)
    chi2_fold = (((folded - image.double()) / sigma) ** 2).sum(dim=1).cpu().numpy()
    chi2 = out['chi2'].double().cpu().numpy()
    print(f'interior {interior.sum()} of {n}: chi2 / target solver up to {chi2[interior].max() / 8:.8f}, folded back up to '
          f'{chi2_fold[interior].max() / 8:.8f}')
    assert (chi2[interior] <= 8 * (1 + 2e-5 + ti.B)).all()
    dr = 2.0 ** -24 * np.linalg.norm((image.double() / sigma).cpu().numpy(), axis=1)
    assert (np.abs(chi2_fold - chi2) <= 2 * np.sqrt(chi2) * dr + dr * dr + ti.B * chi2)[interior].all()
    with pytest.raises(ValueError, match='unsupported'):
        mod.invert_dem(torch.zeros(n, 40, device='cuda'), wavelengths=None)


def test_snf_round_trip_of_a_64_channel_rendering(tmp_path):
    from sunerf.evaluation.loader import SuNeRFLoader
    from sunerf.model.model import NeRF_DT
    from sunerf.model.sunerf import save_state
    from sunerf_hip.response import ResponseSet
    g = load_golden('g6_dt_e2e')
    rset = ResponseSet(list(rc.smooth_channels_64()))
    rendering = rs._rendering(NeRF_DT, g, rset, {'d_filter': 64, 'channels': rset})
    rs._g6_mlp(rendering, g, all_grids=True)
    with torch.no_grad():
        for m in (rendering.coarse_model, rendering.fine_model):
            for i, p in enumerate(m.log_absortpion.values()):
                p.fill_(ABSORPTION_PATTERN[i % 11] * 1e-6 * (1 + i / 64))
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
    assert loader.rendering.response_set == rset and len(loader.rendering.response_set) == 64
    assert tuple(loader.rendering.fine_model.log_absortpion.keys()) == rset.keys
    o, d, t = rs._rays(2)
    wl_host = _set_rows(o.shape[0], rset.codes)
    wl = wl_host.cuda()
    with torch.no_grad():
        a, b = rendering(o, d, t, wl), loader.rendering(o, d, t, wl)
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    high = torch.isin(wl_host, torch.tensor(rset.codes[32:], dtype=torch.float32))
    assert bool((a['image'].cpu()[high] != 0).any()) and bool(torch.isfinite(a['image']).all())
