"""Registration on the device against its NumPy restatement (tests/register_reference.py): the cases of the host test
at orders 0, 1, 3 and 5 under CLOSEST and 2 and 3 under MISSING.  Sampling: ``out`` against scipy's ``map_coordinates`` at the
DEVICE's own coordinates under the gate the project holds the same tap sum to (``prep_reference.gate``).  Geometry: the device's
coordinates against the restatement's under the per-pixel first-order bound the restatement computes.  Status and counts exactly,
NaN sets, reruns by bits, independence of what the outputs held, ``coords = NULL``; the wrapper and ``register_views`` on top.
Pixels whose decision rounding can flip (none in these cases, asserted by tests/test_register_host.py to be at most 2 %) are
left out of the status and value comparison.  Every figure is printed."""
import functools

import numpy as np
import pytest
import torch

import prep_reference as pr
import register_reference as rr

pytestmark = pytest.mark.gpu

MISSING_VALUE = -7.5
CASES = [(name, order, off) for name in rr.cases() for order, off in rr.VARIANTS]


def _dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda', torch.cuda.current_device())


def frame_mask(frame):
    """What the wrapper hands the kernel: the flagged pixels and the non-finite ones."""
    if frame.get('mask') is None:
        return None
    return ((frame['mask'] != 0) | ~np.isfinite(frame['planes'])).astype(np.uint8)


def device_call(case, order, off_disk, missing=MISSING_VALUE, fill=None, want_coords=True):
    """``sunerf_register_frames`` on a case of the restatement, through the raw entry point, with outputs that hold ``fill`` before the
    call.  Coefficients come from the project's prefilter.  Returns numpy ``(out, status, coords or None, state)``."""
    from sunerf_hip import lib, ops
    from sunerf_hip.prep import spline_prefilter
    from sunerf_hip.register import FRAME_DESC, N_STATE
    dev = _dev()
    keep, rows = [], np.zeros(len(case['frames']), dtype=FRAME_DESC)
    for row, frame in zip(rows, case['frames']):
        coef, _ = spline_prefilter(torch.from_numpy(np.ascontiguousarray(frame['planes'])).to(dev), order)
        mask = frame_mask(frame)
        mask = torch.from_numpy(mask).to(dev) if mask is not None else None
        tx, ty = torch.from_numpy(np.ascontiguousarray(frame['tx'])).to(dev), torch.from_numpy(np.ascontiguousarray(frame['ty'])).to(dev)
        keep += [coef, mask, tx, ty]
        row['coefficients'], row['mask'], row['tx'], row['ty'] = coef.data_ptr(), mask.data_ptr() if mask is not None else 0, tx.data_ptr(), ty.data_ptr()
        row['height'], row['width'] = coef.shape[1], coef.shape[2]
        row['c2w'] = np.asarray(frame['c2w'], dtype=np.float32).reshape(-1)
        row['dt'], row['shift_y'], row['shift_x'] = frame['dt'], frame['shift_y'], frame['shift_x']
    table = torch.from_numpy(rows.view(np.uint8).reshape(-1).copy()).to(dev)
    c2w_ref = torch.from_numpy(np.asarray(case['c2w_ref'], dtype=np.float32).reshape(-1).copy()).to(dev)
    tx_ref, ty_ref = torch.from_numpy(case['tx_ref'].copy()).to(dev), torch.from_numpy(case['ty_ref'].copy()).to(dev)
    t, c, h, w = len(rows), case['frames'][0]['planes'].shape[0], ty_ref.shape[0], tx_ref.shape[0]
    out = torch.empty((t, c, h, w), dtype=torch.float32, device=dev)
    status = torch.empty((t, h, w), dtype=torch.uint8, device=dev)
    coords = torch.empty((t, 2, h, w), dtype=torch.float64, device=dev) if want_coords else None
    state = torch.empty((t, N_STATE), dtype=torch.int64, device=dev)
    if fill is not None:
        out.fill_(fill)
        status.fill_(0xA5)
        state.fill_(-12345)
        if coords is not None:
            coords.fill_(fill)
    A, B, C = case['rates']
    lib.call(dev, 'sunerf_register_frames', ops._ptr(table), t, c, order, ops._ptr(c2w_ref), ops._ptr(tx_ref), ops._ptr(ty_ref), h, w,
             float(case['radius']), float(A), float(B), float(C), off_disk, float(missing), case['flags'], ops._ptr(out), ops._ptr(status),
             ops._ptr(coords), ops._ptr(state), ops._stream(dev))
    torch.cuda.synchronize(dev)
    return out.cpu().numpy(), status.cpu().numpy(), coords.cpu().numpy() if want_coords else None, state.cpu().numpy()


@functools.lru_cache(maxsize=None)
def device_result(name, order, off_disk):
    return device_call(rr.cases()[name], order, off_disk, fill=float('nan'))


@pytest.mark.parametrize('name,order,off_disk', CASES, ids=[f'{n}-o{o}-{"closest" if f else "missing"}' for n, o, f in CASES])
def test_the_device_agrees_with_the_restatement(name, order, off_disk):
    case = rr.cases()[name]
    want_out, want_status, want_coords, want_state, detail = rr.case_reference(name, order, off_disk, MISSING_VALUE)
    out, status, coords, state = device_result(name, order, off_disk)
    worst_geometry, worst_sampling = 0.0, 0.0
    for k, (frame, geo) in enumerate(zip(case['frames'], detail)):
        keep = ~geo['excluded']
        share = 1.0 - float(keep.mean())
        assert share <= rr.MAX_UNDECIDABLE
        # status and counts: exact on the pixels rounding cannot flip
        assert np.array_equal(status[k][keep], want_status[k][keep])
        assert np.abs(state[k] - want_state[k]).sum() <= 2 * int((~keep).sum()) and state[k].sum() == keep.size
        assert np.array_equal(state[k], [int((status[k] == s).sum()) for s in (rr.ON_DISK, rr.OFF_DISK, rr.BEHIND, rr.OUTSIDE)])
        # geometry: NaN where no coordinate was formed, else within the bound the restatement computes
        for axis, bound in ((0, geo['bound_y']), (1, geo['bound_x'])):
            got, want = coords[k, axis], want_coords[k, axis]
            assert np.array_equal(np.isnan(got)[keep], np.isnan(want)[keep])
            both = keep & ~np.isnan(want) & ~np.isnan(got)
            if both.any():
                ratio = float((np.abs(got - want)[both] / bound[both]).max())
                worst_geometry = max(worst_geometry, ratio)
        # sampling: the device's value against scipy at the device's own coordinates
        sampled = np.isin(status[k], (rr.ON_DISK, rr.OFF_DISK)) & ~np.isnan(coords[k, 0])
        if off_disk == rr.MISSING:
            sampled &= status[k] == rr.ON_DISK
        assert np.array_equal(sampled[keep], geo['sample'][keep])
        values = rr.sample_planes(frame['planes'], coords[k, 0], coords[k, 1], sampled, order)
        expect = np.where(sampled[None], values, MISSING_VALUE)
        if case['flags'] & rr.PROPAGATE:
            expect[rr.tap_hits(frame_mask(frame), coords[k, 0], coords[k, 1], sampled, order)] = np.nan
        at = np.broadcast_to(keep[None], expect.shape)
        scale = float(np.nanmax(np.abs(np.where(np.isfinite(frame['planes']), frame['planes'], 0.0))))
        worst_sampling = max(worst_sampling, pr.gate(out[k][at], expect[at], scale))
        print(f'{name} frame {k} order {order} off_disk {off_disk}: state {state[k].tolist()}, {100 * share:.2f} % left out, '
              f'{int(np.isnan(out[k]).sum())} NaN values')
    print(f'{name} order {order} off_disk {off_disk}: worst coordinate error / bound {worst_geometry:.2e}, worst value error / gate {worst_sampling:.3f}')
    assert worst_geometry <= 1.0 and worst_sampling <= 1.0
    if case['flags'] & rr.PROPAGATE:
        assert np.isnan(out).any() and not np.isnan(out).all()


@pytest.mark.parametrize('name,order,off_disk', [('three', 3, rr.CLOSEST), ('masked', 5, rr.CLOSEST), ('west', 0, rr.MISSING), ('one', 1, rr.CLOSEST)])
def test_reruns_agree_by_bits_and_no_output_depends_on_what_it_held(name, order, off_disk):
    case = rr.cases()[name]
    first = device_result(name, order, off_disk)          # outputs held NaN
    again = device_call(case, order, off_disk, fill=float('nan'))
    sentinel = device_call(case, order, off_disk, fill=12345.0)
    bare = device_call(case, order, off_disk)
    for other in (again, sentinel, bare):
        for a, b in zip(first, other):
            assert a.tobytes() == b.tobytes()
    # coords = NULL changes nothing else
    without = device_call(case, order, off_disk, fill=12345.0, want_coords=False)
    assert without[2] is None
    for i in (0, 1, 3):
        assert first[i].tobytes() == without[i].tobytes()
    # `missing` may be NaN
    nan = device_call(case, order, off_disk, missing=float('nan'))
    assert np.array_equal(np.isnan(nan[0]), (first[0] == np.float32(MISSING_VALUE)) | np.isnan(first[0])) and np.array_equal(nan[1], first[1])


def _observers(case, dev):
    from sunerf_hip.reprojection import Observer
    out = []
    for frame in case['frames']:
        o = Observer(0.0, 0.0, rr.AU, tx=frame['tx'], ty=frame['ty'])
        o.c2w = torch.from_numpy(np.vstack([frame['c2w'], [[0, 0, 0, 1]]]).astype(np.float32))
        out.append(o)
    ref = Observer(0.0, 0.0, rr.AU, tx=case['tx_ref'], ty=case['ty_ref'])
    ref.c2w = torch.from_numpy(np.vstack([case['c2w_ref'], [[0, 0, 0, 1]]]).astype(np.float32))
    return out, ref


@pytest.mark.parametrize('name', ['three', 'masked', 'east'])
def test_the_wrapper_is_the_raw_call_with_its_own_prefilter(name):
    """``register_frames`` (a list of frames of different shapes, one tensor, shifts, a mask with ``propagate``, explicit sidereal
    rates) gives the bits of the raw call on the same case."""
    from sunerf_hip.register import CARRINGTON_RATE, register_frames
    dev = _dev()
    case = rr.cases()[name]
    observers, ref = _observers(case, dev)
    frames = [torch.from_numpy(np.ascontiguousarray(f['planes'])).to(dev) for f in case['frames']]
    masked = bool(case['flags'] & rr.PROPAGATE)
    kw = dict(reference=ref, reference_time=0.0, rotation=(rr.SIDEREAL[0], rr.SIDEREAL[1], rr.SIDEREAL[2]), order=3, missing=MISSING_VALUE,
              shifts=[[f['shift_y'], f['shift_x']] for f in case['frames']], return_coords=True)
    if masked:
        kw.update(bad=[torch.from_numpy(f['mask']).to(dev) for f in case['frames']], propagate=True)
    got = register_frames(frames if len(frames) > 1 else torch.stack(frames), observers, [f['dt'] for f in case['frames']], **kw)
    assert rr.CARRINGTON == CARRINGTON_RATE
    out, status, coords, state = device_call(case, 3, rr.CLOSEST)
    assert np.array_equal(got['status'].cpu().numpy(), status) and np.array_equal(got['counts'].cpu().numpy(), state)
    assert got['coords'].cpu().numpy().tobytes() == coords.tobytes() and got['image'].cpu().numpy().tobytes() == out.tobytes()
    if name == 'east':          # [T, H, W] in, [T, H', W'] out; derotate is the same call
        from sunerf_hip.register import derotate
        single = register_frames(torch.stack(frames)[:, 0], observers, [2.0], **kw)
        assert single['image'].shape == (1,) + status.shape[1:] and torch.equal(single['image'], got['image'][:, 0])
        kw.pop('rotation')
        turned = derotate(torch.stack(frames), observers[0], [2.0], reference=ref, reference_time=0.0, order=3, missing=MISSING_VALUE)
        assert turned['image'].cpu().numpy().tobytes() == out.tobytes()


def test_register_views_is_register_frames_on_the_views():
    from sunerf_hip.observations import ObservationSet
    from sunerf_hip.reprojection import Observer
    from sunerf_hip.register import register_frames
    dev = _dev()
    obs = ObservationSet(device=dev)
    shapes, lons, times = [(21, 19), (18, 30), (24, 20)], [0.3, -0.2, 0.0], [2.0, -1.0, 0.5]
    for shape, lon, time in zip(shapes, lons, times):
        tx, ty = rr.axes_for(shape, 1.25 * rr.DISK)
        obs.add_view(torch.from_numpy(rr.frame_planes(shape, 2, 20).copy()), 0.05, lon, rr.AU, time=time, tx=tx, ty=ty, wavelengths=[171.0, 193.0])
    kw = dict(rotation=(2.9e-6, -0.4e-6, -0.4e-6), order=3, return_coords=True)
    got = obs.register_views([0, 1, 2], reference=2, **kw)
    views = [obs.views[i] for i in range(3)]
    want = register_frames([v.image for v in views], [Observer.of_view(v) for v in views], [v.time for v in views], reference=2, Rs_per_ds=obs.Rs_per_ds,
                           seconds_per_dt=obs.seconds_per_dt, **kw)
    assert got['image'].shape == (3, 2, 24, 20) and got['status'].shape == (3, 24, 20)
    for k in ('image', 'status', 'counts', 'coords'):
        assert got[k].cpu().numpy().tobytes() == want[k].cpu().numpy().tobytes(), k
    # the reference view comes back as it is (order 3: to the gate), every pixel of it sampled
    counts = got['counts'].cpu().numpy()
    assert counts[2, 2] == 0 and counts[2, 3] == 0 and counts[0, 2] > 0
    image = got['image'][2].cpu().numpy()
    assert pr.gate(image, views[2].image.cpu().numpy().astype(np.float64), float(views[2].image.abs().max())) <= 1.0
    default = obs.register_views()
    assert default['image'].shape == (3, 2, 21, 19)
