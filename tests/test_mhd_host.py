"""CPU checks of the MHD cube field (no GPU): the fp64 restatement the GPU tests use against scipy's interpolator (what the
reference calls), and the host side of ``MHDModel`` -- frame numbering and file naming (mhd_model.py:27-30, :62), frame
loading and its errors, the state-dict keys."""
import os
import sys

import numpy as np
import pytest
import torch

import mhd_reference as ref

REFERENCE_STATE_KEYS = {'log_absortpion.94', 'log_absortpion.131', 'log_absortpion.171', 'log_absortpion.193',
                        'log_absortpion.211', 'log_absortpion.304', 'log_absortpion.335', 'volumetric_constant'}


def _scipy_points(axes, rng):
    """In-bounds points, points beyond each bound of each axis, exact nodes and exact bounds, NaN coordinates."""
    lo = np.array([a[0] for a in axes])
    hi = np.array([a[-1] for a in axes])
    pts = [lo + (hi - lo) * rng.uniform(0, 1, (200, 3))]
    for k in range(3):
        for beyond in (lo[k] - 1e-3, hi[k] + 1e-3, lo[k] - 1.0, hi[k] + 1.0):
            p = lo + (hi - lo) * rng.uniform(0, 1, (5, 3))
            p[:, k] = beyond
            pts.append(p)
    nodes = np.stack([a[rng.integers(0, a.size, 40)] for a in axes], -1)     # exact node hits on every axis
    pts.append(nodes)
    corners = np.array([[lo[0], lo[1], lo[2]], [hi[0], hi[1], hi[2]], [lo[0], hi[1], lo[2]], [hi[0], lo[1], hi[2]]])
    pts.append(corners)                                                       # exact boundary hits (inclusive)
    mixed = lo + (hi - lo) * rng.uniform(0, 1, (6, 3))
    mixed[0, 0] = hi[0]
    mixed[1, 1] = lo[1]
    mixed[2, 2] = hi[2]
    mixed[3, 0] = np.nan
    mixed[4, 1] = np.nan
    mixed[5, 2] = np.nan
    pts.append(mixed)
    return np.concatenate(pts)


def test_restatement_matches_scipy_regular_grid_interpolator():
    """The checker against what the reference calls (mhd_model.py:45-75): in-bounds, out of bounds on every axis, exact
    nodes and bounds, NaN."""
    interpolate = pytest.importorskip('scipy.interpolate')
    rng = np.random.default_rng(11)
    r, th, phi, rho, temp = ref.synthetic_frame(3)
    axes = (phi, th, r)
    pts = _scipy_points(axes, rng)
    for data in (rho, temp):
        clamped = data.copy()
        clamped[np.where(clamped < 0)] = 1e-10                      # mhd_model.py:64
        want = interpolate.RegularGridInterpolator(axes, clamped, method='linear', bounds_error=False, fill_value=1e-10)(pts)
        got = ref.interp_linear(axes, data, pts)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        assert np.isnan(got).sum() == 3
        fin = ~np.isnan(want)
        assert np.allclose(got[fin], want[fin], rtol=1e-12, atol=0), np.abs(got[fin] - want[fin]).max()
        assert (got[200:260] == 1e-10).all()                        # the out-of-bounds block


def test_restatement_time_and_coordinates():
    """mhd_model.py:100-103, :121-124 as the restatement computes them."""
    f1, f2, w = ref.frame_pair(torch.tensor([0., 0.5, 1., 0.25]), 10, 14)
    assert f1.tolist() == [10, 12, 14, 11] and f2.tolist() == [10, 12, 14, 11] and w.tolist() == [0., 0., 0., 0.]
    f1, f2, w = ref.frame_pair(torch.tensor([0.3]), 10, 14)
    assert (f1.item(), f2.item()) == (11, 12) and abs(w.item() - 0.2) < 1e-6
    r, th, phi = ref.spherical(torch.tensor([[0., -1., 0.], [1., 0., 0.], [0., 0., 2.]]))
    assert torch.allclose(phi, torch.tensor([1.5 * np.pi, 0., 0.], dtype=torch.float32))
    assert torch.allclose(th, torch.tensor([np.pi / 2, np.pi / 2, 0.], dtype=torch.float32)) and r.tolist() == [1., 1., 2.]


def test_frame_numbers_and_file_names(tmp_path):
    from sunerf.model.mhd_model import MHDModel, frame_file, frame_number
    root = ref.write_placeholders(tmp_path / 'run', [2531, 2532, 2534])
    m = MHDModel(root, device='cpu', reader=ref.DictReader({}))
    assert (m.ffirst, m.flast) == (2531, 2534)
    assert [os.path.basename(p) for p in m.density_files] == ['rho002531.h5', 'rho002532.h5', 'rho002534.h5']
    assert [os.path.basename(p) for p in m.temperature_files] == ['t002531.h5', 't002532.h5', 't002534.h5']
    assert frame_file(root, 't', 2532) == os.path.join(root, 't', 't002532.h5')
    assert frame_number('/x/rho/rho002531.h5') == 2531
    # the reference's quirk, kept: a number containing 00 is cut there
    assert frame_number('/x/rho/rho001005.h5') == 1
    assert frame_number('/x/rho/rho002500.h5') == 25
    with pytest.raises(ValueError):
        frame_number('/x/rho/rho0000.h5')
    # frames of a time, fp32 like mhd_model.py:121-124
    assert m.frames_for(torch.tensor([0., 1.])) == [2531, 2534]
    assert m.frames_for(torch.tensor([0.5, 0.5, float('nan')])) == [2532, 2533]
    with pytest.raises(ValueError, match='outside'):
        m.frames_for(torch.tensor([1.5]))


def test_frame_loading_clamps_interleaves_and_raises(tmp_path):
    from sunerf.model.mhd_model import MHDModel
    frames = {10: ref.synthetic_frame(1), 11: ref.synthetic_frame(2, n_r=31), 12: ref.synthetic_frame(3)}
    root = ref.write_placeholders(tmp_path / 'run', [10, 11, 12])
    m = MHDModel(root, device='cpu', reader=ref.DictReader(frames))
    data, (phi, th, r) = m.load_frame(11)
    fr_r, fr_th, fr_phi, rho, temp = frames[11]
    assert data.dtype == np.float32 and data.shape == (fr_phi.size, fr_th.size, fr_r.size, 2) and data.flags.c_contiguous
    assert np.array_equal(r, fr_r.astype(np.float32)) and np.array_equal(phi, fr_phi.astype(np.float32))
    assert np.array_equal(data[..., 0], np.where(rho < 0, 1e-10, rho).astype(np.float32))
    assert np.array_equal(data[..., 1], np.where(temp < 0, 1e-10, temp).astype(np.float32))
    assert (data > 0).all()
    # rho and t of one frame on different grids: the t file is named
    shifted_r = frames[12][0].copy()
    shifted_r[5] += 1e-3

    def reader(path):
        got = ref.DictReader(frames)(path)
        return (shifted_r,) + got[1:] if os.path.basename(os.path.dirname(path)) == 't' else got
    m_bad = MHDModel(root, device='cpu', reader=reader)
    with pytest.raises(ValueError, match=r't0012\.h5'):
        m_bad.load_frame(12)
    # a frame inside [ffirst, flast] without its files
    os.remove(os.path.join(root, 'rho', 'rho0011.h5'))
    m_gap = MHDModel(root, device='cpu', reader=ref.DictReader(frames))
    with pytest.raises(FileNotFoundError, match=r'rho0011\.h5'):
        m_gap.load_frame(11)
    with pytest.raises(FileNotFoundError):
        MHDModel(str(tmp_path / 'empty'), device='cpu', reader=ref.DictReader(frames))


def test_default_reader_needs_h5py_or_says_so(tmp_path):
    from sunerf.model.mhd_model import MHDModel
    try:
        import h5py  # noqa: F401
        pytest.skip('h5py is installed: the default reader is usable')
    except ImportError:
        pass
    root = ref.write_placeholders(tmp_path / 'run', [10, 11])
    with pytest.raises(ImportError, match='reader='):
        MHDModel(root, device='cpu').load_frame(10)


def test_state_dict_keys_are_the_references():
    import tempfile
    from sunerf.model.mhd_model import MHDModel
    with tempfile.TemporaryDirectory() as d:
        root = ref.write_placeholders(os.path.join(d, 'run'), [10, 11])
        m = MHDModel(root, device='cpu', reader=ref.DictReader({}))
    sd = m.state_dict()
    assert set(sd) == REFERENCE_STATE_KEYS
    assert [round(sd[f'log_absortpion.{w}'].item(), 4) for w in (94, 131, 171, 193, 211, 304, 335)] == [
        20.4, 20.2, 20.0, 19.8, 19.6, 19.4, 19.2]
    assert sd['volumetric_constant'].item() == 1.0 and all(v.dtype == torch.float32 for v in sd.values())
    assert m.time_dependent and (m.base_log_density, m.base_log_temperature) == (0.0, 0.0)


# ---- the default reader on PSI's file layout -------------------------------------------------------------------------------
class _FakeDataset:
    """What the reader touches of an h5py ``Data`` dataset: ``ndim``, ``dims[k][0]`` (the attached scale), ``[...]``."""

    def __init__(self, data, scales):
        self._data = data
        self.ndim = data.ndim
        self.dims = [[s] for s in scales]

    def __getitem__(self, key):
        return self._data[key]


def _fake_h5py(files):
    import types

    class _File:
        def __init__(self, path, mode='r'):
            self._ds = files[str(path)]

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            return False

        def __getitem__(self, name):
            assert name == 'Data'
            return self._ds
    mod = types.ModuleType('h5py')
    mod.File = _File
    return mod


def _psi_layout(frame):
    """PSI's layout of one variable: data[i_phi, i_theta, i_r], scales attached in Fortran order (dims[0] = r, the length
    of the last data axis; dims[1] = theta; dims[2] = phi)."""
    r, th, phi, rho, temp = frame
    return {'rho': _FakeDataset(rho, (r, th, phi)), 't': _FakeDataset(temp, (r, th, phi))}


@pytest.mark.parametrize('square', [False, True])
def test_default_reader_maps_psi_dimension_scales(tmp_path, monkeypatch, square):
    """``Data.dims[0]`` carries r, ``dims[2]`` phi (PSI's rdhdf_3d -> ``r, th, phi``, mhd_model.py:62).  ``square``: n_phi ==
    n_r, where swapped axes would still have the right lengths."""
    from sunerf.model import mhd_model
    frames = {10: ref.synthetic_frame(1, n_phi=23, n_theta=17, n_r=29),
              11: ref.synthetic_frame(2, n_phi=25, n_theta=17, n_r=25) if square else ref.synthetic_frame(2, n_r=31)}
    root = ref.write_placeholders(tmp_path / 'run', sorted(frames))
    files = {}
    for f, fr in frames.items():
        for var, ds in _psi_layout(fr).items():
            files[mhd_model.frame_file(root, var, f)] = ds
    monkeypatch.setitem(sys.modules, 'h5py', _fake_h5py(files))
    r, th, phi, data = mhd_model.read_psi_hdf5(mhd_model.frame_file(root, 'rho', 11))
    assert np.array_equal(r, frames[11][0]) and np.array_equal(th, frames[11][1]) and np.array_equal(phi, frames[11][2])
    assert data.shape == (phi.size, th.size, r.size)
    psi = mhd_model.MHDModel(root, device='cpu')           # the default reader
    mem = mhd_model.MHDModel(root, device='cpu', reader=ref.DictReader(frames))
    for f in frames:
        got, want = psi.load_frame(f), mem.load_frame(f)
        assert np.array_equal(got[0], want[0]) and all(np.array_equal(a, b) for a, b in zip(got[1], want[1]))


def test_default_reader_on_a_real_psi_layout_file(tmp_path):
    """The same with h5py itself: a file written the way PSI's tools write theirs (dim1 = r on Data.dims[0])."""
    h5py = pytest.importorskip('h5py')
    from sunerf.model import mhd_model
    frames = {10: ref.synthetic_frame(1), 11: ref.synthetic_frame(2, n_r=31)}
    root = ref.write_placeholders(tmp_path / 'run', sorted(frames))
    for f, (r, th, phi, rho, temp) in frames.items():
        for var, data in (('rho', rho), ('t', temp)):
            path = mhd_model.frame_file(root, var, f)
            os.remove(path)
            with h5py.File(path, 'w') as h5:
                ds = h5.create_dataset('Data', data=data.astype(np.float32))
                for k, (name, scale) in enumerate((('dim1', r), ('dim2', th), ('dim3', phi))):
                    sc = h5.create_dataset(name, data=scale.astype(np.float32))
                    sc.make_scale(name)
                    ds.dims[k].attach_scale(sc)
    psi = mhd_model.MHDModel(root, device='cpu')
    mem = mhd_model.MHDModel(root, device='cpu', reader=ref.DictReader(frames))
    for f in frames:
        got, want = psi.load_frame(f), mem.load_frame(f)
        assert np.array_equal(got[0], want[0]) and all(np.array_equal(a, b) for a, b in zip(got[1], want[1]))


def test_bucket_table_is_capped_on_a_psi_clustered_r_grid():
    """r = 1 + 29 u^3 on 301 nodes: span / smallest spacing ~ 2.7e7, so the table is capped and its first buckets hold several
    nodes each (the kernel walks them); every entry is the cell of its bucket's lower edge."""
    from sunerf_hip import ops
    r = torch.from_numpy(ref.psi_clustered_r().astype(np.float32))
    table, inv_width = ops.mhd_bucket_table(r)
    assert table.numel() == ops.MHD_MAX_BUCKETS
    assert (table[1:] - table[:-1]).max().item() > 1
    g = r.double()
    edges = g[0] + torch.arange(table.numel(), dtype=torch.float64) * ((g[-1] - g[0]) / table.numel())
    assert torch.equal(table.long(), (torch.searchsorted(g, edges, right=True) - 1).clamp(0, r.numel() - 2))
    assert abs(inv_width - table.numel() / (g[-1] - g[0]).item()) < 1e-6 * inv_width
