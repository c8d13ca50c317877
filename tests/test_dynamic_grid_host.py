"""CPU-only checks of the voxel-grid field with a time axis (no GPU): the float64 restatement the GPU tests check
the kernels against (vs scipy on a 4-D grid, the time rule), the Python side (refusals, from_volume, the temporal prior,
pickling, module defaults), the extension entry points (declared, bound, kept out of the first table; argument errors in
their documented order) and the case table of tests/test_gpu_dynamic_grid_abi.py."""
import ctypes
import inspect
import io
import math
import os

import numpy as np
import pytest
import torch

import dynamic_grid_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAU5 = (0.0, 0.25, 0.375, 0.75, 1.0)


@pytest.fixture(scope='session')
def lib():
    import sunerf_hip
    if not os.path.exists(sunerf_hip.LIB_PATH):
        import subprocess
        subprocess.check_call(['bash', os.path.join(ROOT, '2024-hl-spi3s-sunerf_amd', 'csrc', 'build.sh')])
    return sunerf_hip.load()


def nonuniform_grid(**kwargs):
    from sunerf_hip.volume import CartesianGrid
    return CartesianGrid([-1.0, -0.4, 0.1, 0.3, 1.2], [-0.9, -0.2, 0.5, 0.8], [-1.1, 0.05, 0.7], **kwargs)


# ---- the restatement --------------------------------------------------------------------------------------------------------
def test_restatement_agrees_with_scipy_on_a_nonuniform_4d_grid():
    from scipy.interpolate import RegularGridInterpolator
    grid = nonuniform_grid()
    tau = (0.0, 0.2, 0.45, 1.0)
    gen = torch.Generator().manual_seed(21)
    values = torch.randn(4, 5, 4, 3, 2, generator=gen, dtype=torch.float64)
    lo = torch.tensor([-1.0, -0.9, -1.1, 0.0])
    hi = torch.tensor([1.2, 0.8, 0.7, 1.0])
    pts = (lo + (hi - lo) * (0.01 + 0.98 * torch.rand(3000, 4, generator=gen))).float()        # interior points
    raw, abs_sum, inside = ref.field(grid, tau, values, pts, (-7.0, 3.0))
    assert bool(inside.all()) and bool((abs_sum > 0).all())
    for c in range(2):
        rgi = RegularGridInterpolator((np.asarray(tau),) + tuple(a.numpy() for a in grid.axes), values[..., c].numpy(),
                                      method='linear')
        want = rgi(pts.double().numpy()[:, [3, 0, 1, 2]])
        assert np.abs(raw[:, c].numpy() - want).max() <= 1e-12
    # autograd through the restatement is the adjoint: <A v, g> = <v, A^T g>
    leaf = values.clone().requires_grad_(True)
    g = torch.randn(3000, 2, generator=gen, dtype=torch.float64)
    out, _, _ = ref.field(grid, tau, leaf, pts, (0.0, 0.0))
    (out * g).sum().backward()
    assert abs((out.detach() * g).sum().item() - (values * leaf.grad).sum().item()) <= 1e-9


def test_time_rule():
    f32 = torch.float32
    below0 = torch.nextafter(torch.tensor(0.0, dtype=f32), torch.tensor(-math.inf, dtype=f32)).item()
    above0 = torch.nextafter(torch.tensor(0.0, dtype=f32), torch.tensor(math.inf, dtype=f32)).item()
    below1 = torch.nextafter(torch.tensor(1.0, dtype=f32), torch.tensor(-math.inf, dtype=f32)).item()
    above1 = torch.nextafter(torch.tensor(1.0, dtype=f32), torch.tensor(math.inf, dtype=f32)).item()
    # (t, j, s, inside under 'clamp', inside under 'fill'); s is exact where it is written as a fraction of dyadic numbers
    rows = [(0.0, 0, 0.0, True, True), (0.25, 0, 1.0, True, True), (0.375, 1, 1.0, True, True), (0.75, 2, 1.0, True, True),
            (1.0, 3, 1.0, True, True),
            (0.125, 0, 0.5, True, True), (0.3125, 1, 0.5, True, True), (0.5625, 2, 0.5, True, True), (0.875, 3, 0.5, True, True),
            (below0, 0, 0.0, True, False), (above0, 0, above0 / 0.25, True, True),
            (below1, 3, (below1 - 0.75) / 0.25, True, True), (above1, 3, 1.0, True, False),
            (-0.5, 0, 0.0, True, False), (1.5, 3, 1.0, True, False), (math.nan, 0, 0.0, False, False)]
    t = torch.tensor([r[0] for r in rows], dtype=f32)
    for mode, col in (('clamp', 3), ('fill', 4)):
        j, s, inside = ref.locate_time(TAU5, t, mode)
        assert inside.tolist() == [r[col] for r in rows], mode
        for k, r in enumerate(rows):
            if r[col]:
                assert j[k].item() == r[1] and s[k].item() == r[2], (mode, r, j[k].item(), s[k].item())
            else:
                assert j[k].item() == 0 and s[k].item() == 0.0, (mode, r)
    # a field that is linear in time and constant in space: the blend returns the line; outside, the clamp or the fill
    grid = nonuniform_grid()
    values = torch.tensor(TAU5, dtype=torch.float64).reshape(5, 1, 1, 1, 1).expand(5, 5, 4, 3, 1).contiguous()
    pts = torch.cat([torch.zeros(len(rows), 3), t[:, None]], 1)
    raw, _, inside = ref.field(grid, TAU5, values, pts, (-9.0,), time_mode='clamp')
    want = torch.tensor([min(max(r[0], 0.0), 1.0) if r[3] else -9.0 for r in rows], dtype=torch.float64)
    assert (raw[:, 0] - want).abs().max().item() <= 1e-15
    raw, _, inside = ref.field(grid, TAU5, values, pts, (-9.0,), time_mode='fill')
    want = torch.tensor([r[0] if r[4] else -9.0 for r in rows], dtype=torch.float64)
    assert (raw[:, 0] - want).abs().max().item() <= 1e-15


# ---- the Python side --------------------------------------------------------------------------------------------------------
def test_refusals():
    from sunerf.model.grid_model import DynamicGridField, DynamicGridFieldDT
    from sunerf_hip import SunerfHipError
    grid = nonuniform_grid()
    with pytest.raises(ValueError, match='at least two frames'):
        DynamicGridField(grid, frame_times=[0.5])
    with pytest.raises(ValueError, match='frame_times'):
        DynamicGridField(grid)
    with pytest.raises(ValueError, match='strictly increasing'):
        DynamicGridField(grid, frame_times=[0.0, 0.5, 0.5])
    with pytest.raises(ValueError, match='strictly increasing'):
        DynamicGridField(grid, frame_times=[1.0, 0.0])
    with pytest.raises(ValueError, match='finite'):
        DynamicGridField(grid, frame_times=[0.0, math.nan, 1.0])
    with pytest.raises(ValueError, match='finite'):
        DynamicGridField(grid, frame_times=[0.0, math.inf])
    with pytest.raises(ValueError, match='d_input must be 4'):
        DynamicGridField(grid, d_input=3, frame_times=[0.0, 1.0])
    with pytest.raises(ValueError, match='time_mode'):
        DynamicGridField(grid, frame_times=[0.0, 1.0], time_mode='periodic')
    with pytest.raises(ValueError, match='1 to 4'):
        DynamicGridField(grid, d_output=5, frame_times=[0.0, 1.0])
    with pytest.raises(ValueError, match='d_output must be 2'):
        DynamicGridFieldDT(grid, d_output=1, frame_times=[0.0, 1.0])
    with pytest.raises(ValueError, match='init has shape'):
        DynamicGridField(grid, frame_times=[0.0, 1.0], init=torch.zeros(3, 5, 4, 3, 2))
    field = DynamicGridField(grid, frame_times=[0.0, 1.0])
    with pytest.raises(SunerfHipError):                       # no CPU path
        field.field_on_rays(torch.zeros(4, 3), torch.ones(4, 3), torch.ones(4, 8), torch.zeros(4, 1))
    with pytest.raises(ValueError, match=r'\(M, 4\)'):
        field(torch.zeros(4, 3))
    with pytest.raises(SunerfHipError):
        field(torch.zeros(4, 4))


def test_init_forms():
    from sunerf.model.grid_model import DynamicGridField
    grid = nonuniform_grid()
    tau = [0.0, 0.5, 2.0]
    assert DynamicGridField(grid, frame_times=tau).values.shape == (3, 5, 4, 3, 2)
    assert float(DynamicGridField(grid, frame_times=tau).values.detach().abs().max()) == 0.0
    assert bool((DynamicGridField(grid, frame_times=tau, init=1.5).values == 1.5).all())
    per_channel = DynamicGridField(grid, d_output=3, frame_times=tau, init=(1.0, 2.0, 3.0)).values
    assert torch.equal(per_channel[2, 4, 3, 2], torch.tensor([1.0, 2.0, 3.0]))
    frame = torch.randn(5, 4, 3, 2)
    repeated = DynamicGridField(grid, frame_times=tau, init=frame).values
    assert all(torch.equal(repeated[f], frame) for f in range(3)) and repeated.is_contiguous()
    full = torch.randn(3, 5, 4, 3, 2)
    field = DynamicGridField(grid, frame_times=tau, init=full, time_mode='fill', trainable=False)
    assert torch.equal(field.values, full) and field.values.data_ptr() != full.data_ptr() and not field.values.requires_grad
    assert field.time_dependent and field.n_frames == 3 and field.time_mode == 'fill'
    assert field.frame_times.dtype == torch.float64 and field.frame_times.tolist() == tau
    assert field.field_parameters() == [field.values]


def test_from_volume_keeps_the_bits_and_refuses_a_single_time():
    from sunerf.model.grid_model import DynamicGridField, GridField
    grid = nonuniform_grid(origin=(0.1, -0.2, 0.3))
    inf = torch.randn(3, 5, 4, 3, 2, generator=torch.Generator().manual_seed(3))
    inf[0, 0, 0, 0, 0] = float(np.float32(1e-42))                 # a subnormal survives too
    volume = {'inferences': inf, 'radius': grid.radius_f64().float(), 'grid': grid, 'times': [0.25, 0.5, 0.75], 'Rs_per_ds': 0.5,
              'kind': 'emission'}
    field = DynamicGridField.from_volume(volume)
    assert torch.equal(field.values.detach().view(torch.int32), inf.view(torch.int32))
    assert field.Rs_per_ds == 0.5 and field.d_output == 2 and not field.values.requires_grad
    assert field.values.data_ptr() != inf.data_ptr() and field.frame_times.tolist() == [0.25, 0.5, 0.75]
    assert torch.equal(field.fill, torch.tensor([-50.0, 0.0]))
    as_numpy = DynamicGridField.from_volume({**volume, 'inferences': inf.numpy()}, trainable=True, time_mode='fill')
    assert torch.equal(as_numpy.values.detach().view(torch.int32), inf.view(torch.int32)) and as_numpy.values.requires_grad
    single = {**volume, 'inferences': inf[0], 'times': 0.25}
    with pytest.raises(ValueError, match='GridField'):
        DynamicGridField.from_volume(single)
    with pytest.raises(ValueError, match='GridField'):
        DynamicGridField.from_volume({**volume, 'inferences': inf[:1], 'times': [0.25]})
    assert GridField.from_volume(single).values.shape == (5, 4, 3, 2)       # where the message points
    with pytest.raises(ValueError, match='do not fit'):
        DynamicGridField.from_volume({**volume, 'times': [0.25, 0.5]})
    with pytest.raises(ValueError, match='float32'):
        DynamicGridField.from_volume({**volume, 'inferences': inf.double()})
    with pytest.raises(ValueError, match='strictly increasing'):
        DynamicGridField.from_volume({**volume, 'times': [0.25, 0.75, 0.5]})


def test_priors_against_hand_computations():
    from sunerf.model.grid_model import DynamicGridField, GridField
    from sunerf_hip.volume import SphericalGrid
    lon = np.linspace(-math.pi, math.pi, 12, endpoint=False)
    for grid, mode in ((nonuniform_grid(), 'patch'), (SphericalGrid(np.linspace(-1.2, 1.2, 7), lon, np.array([1.0, 1.1, 1.25, 1.5, 2.0])), 'open')):
        init = torch.randn(5, *grid.shape, 3, generator=torch.Generator().manual_seed(5))
        field = DynamicGridField(grid, d_output=3, frame_times=TAU5, init=init)
        got = field.temporal_smoothness()
        want = ref.temporal_smoothness(TAU5, field.values.detach())
        assert abs(got.item() - want.item()) <= 1e-5 * abs(want.item())
        got.backward()
        assert field.values.grad is not None and bool(torch.isfinite(field.values.grad).all()) and field.values.grad.abs().max() > 0
        # the spatial prior: the mean over the frames of the static field's
        got = field.smoothness()
        want = ref.smoothness(grid, field.values.detach(), mode)
        assert abs(got.item() - want.item()) <= 1e-5 * abs(want.item())
        per_frame = torch.stack([GridField(grid, d_output=3, init=init[f]).smoothness() for f in range(5)]).mean()
        assert abs(got.item() - per_frame.item()) <= 1e-6 * abs(per_frame.item())
    still = DynamicGridField(nonuniform_grid(), frame_times=TAU5, init=torch.randn(5, 4, 3, 2))     # one frame, repeated
    assert still.temporal_smoothness().item() == 0.0 and still.smoothness().item() > 0.0
    # the uneven steps count: doubling one interval's length quarters its term
    v = torch.zeros(3, 5, 4, 3, 1)
    v[1:] = 1.0
    assert DynamicGridField(nonuniform_grid(), d_output=1, frame_times=(0.0, 0.5, 1.0), init=v).temporal_smoothness().item() == 2.0
    assert DynamicGridField(nonuniform_grid(), d_output=1, frame_times=(0.0, 1.0, 1.5), init=v).temporal_smoothness().item() == 0.5


def test_pickle_and_state_dict_round_trip():
    from sunerf.model.grid_model import DynamicGridField, DynamicGridFieldDT
    from sunerf.rendering.emission import EmissionRadiativeTransfer
    grid = nonuniform_grid()
    field = DynamicGridFieldDT(grid, init=torch.randn(3, *grid.shape, 2), fill=(1.0, 2.0), Rs_per_ds=2.0, frame_times=(0.0, 0.3, 1.0),
                               time_mode='fill')
    field._descs['stale'] = object()                           # stands for a device descriptor (ctypes: not picklable)
    buf = io.BytesIO()
    torch.save(field, buf)
    buf.seek(0)
    back = torch.load(buf, weights_only=False)
    assert back._descs == {} and back.lon_mode == field.lon_mode and back.Rs_per_ds == 2.0 and back.time_mode == 'fill'
    assert torch.equal(back.values, field.values) and torch.equal(back.fill, field.fill)
    assert torch.equal(back.frame_times, field.frame_times) and back.frame_times.dtype == torch.float64
    assert set(back.state_dict()) == set(field.state_dict())
    assert {'values', 'fill', 'frame_times', 'volumetric_constant', 'log_absortpion.171'} <= set(field.state_dict())
    assert set(DynamicGridField(grid, frame_times=(0.0, 1.0)).state_dict()) == {'values', 'fill', 'frame_times'}
    other = DynamicGridFieldDT(grid, frame_times=(0.0, 0.5, 2.0))
    other.load_state_dict(field.state_dict())
    assert torch.equal(other.values, field.values) and other.frame_times.tolist() == [0.0, 0.3, 1.0]
    assert math.isclose(field.fill[0].item(), 1.0) and DynamicGridFieldDT(grid, frame_times=(0.0, 1.0)).fill[1].item() == -10.0
    # a rendering whose models have a time axis pickles whole (what save_state writes into a .snf)
    mod = EmissionRadiativeTransfer(Rs_per_ds=1.0, sampling_config={'type': 'stratified', 'n_samples': 8, 'perturb': False},
                                    hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 8},
                                    model=DynamicGridField, model_config={'grid': grid, 'frame_times': (0.0, 0.5, 1.0)})
    assert isinstance(mod.fine_model, DynamicGridField) and mod.fine_model.d_output == 2 and mod.fine_model.n_frames == 3
    buf = io.BytesIO()
    torch.save({'rendering': mod}, buf)
    buf.seek(0)
    back = torch.load(buf, weights_only=False)['rendering']
    assert torch.equal(back.fine_model.values, mod.fine_model.values)
    assert torch.equal(back.fine_model.frame_times, mod.fine_model.frame_times)


def _module(**kwargs):
    from sunerf.model.sunerf import EmissionSuNeRFModule
    return EmissionSuNeRFModule(Rs_per_ds=1.0, seconds_per_dt=1.0, image_scaling_config={'vmax': 1, 'a': 0.005},
                                sampling_config={'type': 'stratified', 'n_samples': 8, 'perturb': False},
                                hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 8}, **kwargs)


def test_lambda_temporal_defaults_to_todays_behaviour():
    from sunerf.model.grid_model import DynamicGridField, GridField
    from sunerf.model.model import NeRF
    from sunerf.model.sunerf import DensityTemperatureSuNeRFModule, EmissionSuNeRFModule
    for cls in (EmissionSuNeRFModule, DensityTemperatureSuNeRFModule):
        assert inspect.signature(cls.__init__).parameters['lambda_temporal'].default == 0.0
    loss = torch.tensor(1.25)
    m = _module(model_config={'d_filter': 64})
    assert isinstance(m.rendering.fine_model, NeRF) and m.lambda_temporal == 0.0
    assert m._with_smoothness(loss) is loss                    # nothing is added, not even a zero
    m.lambda_temporal = 0.5
    assert m._with_smoothness(loss) is loss                    # a NeRF has no temporal prior
    s = _module(model=GridField, model_config={'grid': nonuniform_grid(), 'init': torch.randn(5, 4, 3, 2)}, lambda_temporal=0.5)
    assert s._with_smoothness(loss) is loss                    # nor has a static grid
    init = torch.randn(3, 5, 4, 3, 2)
    g = _module(model=DynamicGridField, model_config={'grid': nonuniform_grid(), 'init': init, 'frame_times': (0.0, 0.5, 1.0)})
    assert g.lambda_temporal == 0.0 and g._with_smoothness(loss) is loss
    g.lambda_temporal = 0.5
    coarse, fine = g.rendering.coarse_model, g.rendering.fine_model
    want = loss + 0.5 * (coarse.temporal_smoothness() + fine.temporal_smoothness())
    assert torch.equal(g._with_smoothness(loss), want) and want.item() > 1.25
    g.lambda_smoothness = 0.25                                 # both priors, the spatial one first
    want = (loss + 0.25 * (coarse.smoothness() + fine.smoothness())) + 0.5 * (coarse.temporal_smoothness() + fine.temporal_smoothness())
    assert torch.equal(g._with_smoothness(loss), want)
    g.lambda_temporal = 0.0
    assert torch.equal(g._with_smoothness(loss), loss + 0.25 * (coarse.smoothness() + fine.smoothness()))


# ---- the entry points -------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_kept_out_of_the_first_table(lib):
    """(The table itself -- declared, bound, frozen, versioned, built, its symbols in no other table or older header:
    tests/test_abi_tables_host.py.)"""
    ext = open(os.path.join(ROOT, 'include', 'sunerf_hip_ext.h')).read()
    assert 'mhd_model.py:112-124' in ext and '8l' in ext
    assert lib.sunerf_abi_version() == 9 and lib.sunerf_ext_abi_version() == 1


def _desc(n=(5, 4, 3), c=2, kind=0, lon_mode=0, scale=1.0):
    from sunerf_hip.grid_field import GridFieldDesc
    d = GridFieldDesc()
    for k in range(3):
        d.n[k] = n[k]
    d.n_channels, d.kind, d.lon_mode, d.Rs_per_ds = c, kind, lon_mode, scale
    return d


@pytest.mark.parametrize('c', [1, 4])
@pytest.mark.parametrize('n_total', [0, 1, 64, 65])
def test_workspace_formula(lib, n_total, c):
    assert lib.sunerf_dynamic_grid_bwd_workspace_bytes(n_total, c) == math.ceil(n_total / 64) * 2 * 16 * c * 4


def test_argument_errors_without_gpu(lib):
    """include/sunerf_hip_ext.h: the descriptor and the sizes first (-1; the id range -2), then the empty batch (0), then null
    pointers (-1) and the workspace (-3); all before anything touches a device."""
    one = ctypes.c_void_p(8)            # a non-null pointer that is never followed: the call is refused first

    def fwd(d, n_frames=3, mode=0, n_rays=4, n_samples=8, points=None, stride=0):
        return lib.sunerf_dynamic_grid_fwd(ctypes.byref(d) if d is not None else None, None, n_frames, mode, None, None, None, None,
                                           None, n_rays, n_samples, points, stride, None, None, None, None)

    def bwd(d, n_frames=3, n_total=100, ws_bytes=0, g_values=None, others=None):
        return lib.sunerf_dynamic_grid_bwd(ctypes.byref(d) if d is not None else None, n_frames, others, others, others, others,
                                           others, n_total, others, ws_bytes, g_values, 0, None)
    # 1. the descriptor and the sizes: even the empty batch is refused
    assert fwd(None, n_rays=0) == -1 and bwd(None, n_total=0) == -1
    for bad_n in ((1, 4, 3), (5, 1, 3), (5, 4, 1)):
        assert fwd(_desc(n=bad_n), n_rays=0) == -1 and bwd(_desc(n=bad_n), n_total=0) == -1
    assert fwd(_desc(c=0), n_rays=0) == -1 and fwd(_desc(c=5), n_rays=0) == -2 and bwd(_desc(c=5), n_total=0) == -2
    assert fwd(_desc(kind=2), n_rays=0) == -1 and fwd(_desc(kind=0, lon_mode=1), n_rays=0) == -1
    assert fwd(_desc(scale=0.0), n_rays=0) == -1
    for bad_frames in (1, 0, -3):
        assert fwd(_desc(), n_frames=bad_frames, n_rays=0) == -1 and bwd(_desc(), n_frames=bad_frames, n_total=0) == -1
    assert fwd(_desc(), mode=2, n_rays=0) == -1 and fwd(_desc(), mode=-1, n_rays=0) == -1
    assert fwd(_desc(), n_rays=-1) == -1 and fwd(_desc(), n_rays=0, n_samples=0) == -1
    assert fwd(_desc(), n_rays=0, n_samples=1, points=one, stride=3) == -1      # a point needs its time
    assert fwd(_desc(), n_rays=0, n_samples=2, points=one, stride=4) == -1
    assert bwd(_desc(), n_total=-1) == -1
    # ... the id range: (T - 1) * n_cells ids and the sentinel must fit int32.  1024^3 nodes: 1023^3 = 1 070 599 167 cells,
    # twice that is 2 141 198 334 < 2^31 - 1, three times is not
    big = _desc(n=(1024, 1024, 1024))
    assert fwd(big, n_frames=3, n_rays=0) == 0 and bwd(big, n_frames=3, n_total=0, g_values=None) == -1      # (null g_values)
    assert fwd(big, n_frames=4, n_rays=0) == -2 and bwd(big, n_frames=4, n_total=0) == -2
    assert fwd(_desc(n=(2048, 2048, 2048)), n_frames=2, n_rays=0) == -2                                       # the static limit
    # the size errors come before the range: -1, not -2
    assert fwd(big, n_frames=4, mode=2, n_rays=0) == -1 and fwd(big, n_frames=4, n_rays=-1) == -1
    # 2. the empty batch: 0 with every pointer null (modes, channel counts, a periodic longitude)
    assert fwd(_desc(), n_rays=0) == 0 and fwd(_desc(c=4), mode=1, n_rays=0) == 0 and fwd(_desc(kind=1, lon_mode=2), n_rays=0) == 0
    assert fwd(_desc(), n_rays=0, n_samples=1, points=one, stride=4) == 0
    # 3. null pointers
    assert fwd(_desc()) == -1 and fwd(_desc(), n_samples=1, points=one, stride=4) == -1
    assert bwd(_desc(), n_total=0) == -1                                                                      # g_values
    assert bwd(_desc(), g_values=one) == -1 and bwd(_desc(), g_values=one, ws_bytes=1 << 30) == -1
    # 4. the workspace, after the pointers
    need = lib.sunerf_dynamic_grid_bwd_workspace_bytes(100, 2)
    assert need == 2 * 2 * 16 * 2 * 4
    assert bwd(_desc(), g_values=one, others=one, ws_bytes=need - 1) == -3 and bwd(_desc(), g_values=one, others=one, ws_bytes=0) == -3


# ---- the case table of the buffer-extent test -----------------------------------------------------------------------------------
def test_extent_cases_build_on_the_cpu_and_match_the_binding(lib):
    import abi_arena as aa
    import abi_cases as ac
    from sunerf_hip import lib as binding
    before = dict(ac.CASES)
    import test_gpu_dynamic_grid_abi as ext
    assert ac.CASES == before and not set(ext.EXT_CASES) & set(ac.CASES)          # importing registers nothing
    assert set(ext.EXT_CASES) == {'sunerf_dynamic_grid_fwd', 'sunerf_dynamic_grid_bwd'} and all(ext.EXT_TILES[k] for k in ext.EXT_CASES)
    integers = (ctypes.c_int, ctypes.c_int64, ctypes.c_size_t)
    for name, (builder, shapes) in ext.EXT_CASES.items():
        argtypes = binding.signature(name)[1]
        assert len(shapes) == len(set(shapes)) and shapes
        for shape in shapes:
            case = builder(shape, 'cpu')
            assert case.name == name and len(case.args) == len(argtypes), (shape, len(case.args), len(argtypes))
            assert case.args[-1] == ac.STREAM and len(case.ctypes_args(None)) == len(argtypes)
            seen = set()
            for i, (arg, ctype) in enumerate(zip(case.args[:-1], argtypes[:-1])):
                where = f'{name} {shape} argument {i}'
                if isinstance(arg, (aa.Buffer, aa.Absent)):
                    assert ctype is ctypes.c_void_p and arg.tag in aa.TAGS and arg.name not in seen, where
                    seen.add(arg.name)
                    if isinstance(arg, aa.Buffer):
                        assert arg.numel > 0 and arg in case.arena.buffers, where
                elif isinstance(arg, ac.HostValue):
                    assert ctype is ctypes.c_void_p and i == 0, where
                else:
                    assert ctype in integers and isinstance(arg, int) and not isinstance(arg, bool), (where, arg)
            for b in case.arena.buffers:
                assert b.guard_bytes >= aa.MIN_GUARD_BYTES
            if case.ws_index is not None:
                assert argtypes[case.ws_index] is ctypes.c_size_t and case.args[case.ws_index] > 0
                ws = case.args[case.ws_index - 1]
                assert isinstance(ws, aa.Buffer) and ws.tag == aa.WORKSPACE and ws.numel == case.args[case.ws_index]
            assert all(argtypes[i] in integers for i in case.empty)
            # the extents are the header's: 8 weights per sample, (T - 1) n_cells + 1 segment starts, T frames of values
            sizes = {b.name: b.numel for b in case.arena.buffers}
            if name == 'sunerf_dynamic_grid_fwd':
                n, s, ch, mode, want_index = shape
                assert sizes['raw'] == n * s * ch and sizes['frame_times'] == 3 and sizes['values'] % (3 * ch) == 0
                assert (sizes.get('weights'), sizes.get('cells')) == ((n * s * 8, n * s) if want_index else (None, None))
                assert ('points' in sizes) == (mode == 'points4') and sizes.get('points', 4 * n * s) == 4 * n * s
                assert sizes.get('ray_times', n) == n
            else:
                total, ch, acc = shape
                n_frames = case.args[1]
                assert sizes['weights'] == total * 8 and sizes['perm'] == sizes['cells'] == total and sizes['g_raw'] == total * ch
                assert sizes['g_values'] % (n_frames * ch) == 0 and sizes['frame_times'] == n_frames
                assert sizes['workspace'] == math.ceil(total / 64) * 2 * 16 * ch * 4
                from sunerf_hip.grid_field import n_cells
                grid = case.args[0].keep.grid
                assert sizes['seg_start'] == (n_frames - 1) * n_cells(grid, case.args[0].keep.space.lon_mode) + 1
