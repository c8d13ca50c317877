"""Mirror of the reference's ``sunerf/rendering/density_temperature.py`` on the fused HIP path."""
import torch

from sunerf.model.model import NeRF_DT
from sunerf.rendering.base_tracing import SuNeRFRendering, field_on_query_points
from sunerf.rendering.functional import _field_raw, dt_pass, dt_raw2outputs
from sunerf_hip import ops
from sunerf_hip.genx import CHANNELS, read_aia_temp_resp
from sunerf_hip.response import ResponseSet


def _tensors_inside(obj, depth=3):
    """1-D tensors reachable through the attributes of ``obj`` (an interpolator object of unknown class)."""
    found = []
    if torch.is_tensor(obj):
        return [obj] if obj.ndim == 1 and obj.numel() >= 2 else []
    if depth == 0:
        return found
    for v in (vars(obj).values() if hasattr(obj, '__dict__') else (obj if isinstance(obj, (list, tuple)) else ())):
        found += _tensors_inside(v, depth - 1)
    return found


def _tables_from_interpolators(response):
    """(logte [7, n], response [7, n]) out of the ``{wavelength: Interp1D(logte, tresp * exposure)}`` dict a reference-written
    state carries (density_temperature.py:132-146): per channel the strictly increasing grid and the other tensor of its
    length.  None when the objects do not show them (then the table is read from the file again)."""
    rows_x, rows_y = [], []
    for channel in CHANNELS:
        ts = _tensors_inside(response.get(channel))
        grids = [t for t in ts if bool((t[1:] > t[:-1]).all())]
        if not grids:
            return None
        x = grids[0]
        ys = [t for t in ts if t is not x and t.numel() == x.numel() and t.data_ptr() != x.data_ptr()]
        if len(ys) != 1:
            return None
        rows_x.append(x.detach().float().cpu())
        rows_y.append(ys[0].detach().float().cpu())
    if len({r.numel() for r in rows_x}) != 1:
        return None
    return torch.stack(rows_x), torch.stack(rows_y)


class DensityTemperatureRadiativeTransfer(SuNeRFRendering):
    """density_temperature.py:78-274.  Same constructor; the AIA response table is read from
    ``sunerf/data/aia_temp_resp.genx`` relative to the working directory exactly like the reference (:131) unless
    ``response_table=(logte [7,101], tresp [7,101])`` is passed.

    ``response_set`` (a ``sunerf_hip.response.ResponseSet``): render against that set's channels instead of the AIA table --
    any instrument, any number of channels up to 64, each on its own log T grid.  The rays' ``wavelengths`` rows then carry the
    set's codes, and the models need one ``log_absortpion`` scalar per code (``model_config={'channels': response_set}``).  The
    AIA table is neither read nor held then.  Without it every call is what it was."""

    def __init__(self, model_config=None, device=None, aia_exp_time=2.9, pixel_intensity_factor=1e10,
                 response_table=None, response_path="sunerf/data/aia_temp_resp.genx", response_set=None, **kwargs):
        model_config = {} if model_config is None else model_config
        if response_set is not None and not isinstance(response_set, ResponseSet):
            raise TypeError('response_set must be a sunerf_hip.response.ResponseSet')
        kwargs.setdefault('model', NeRF_DT)
        super().__init__(model_config=model_config, **kwargs)
        self.response_set = response_set
        device = torch.device("cuda" if torch.cuda.is_available() else "cpu") if device is None else device
        self.device = device
        self.pixel_intensity_factor = pixel_intensity_factor
        if response_set is not None:
            return
        logte, tresp = read_aia_temp_resp(response_path) if response_table is None else response_table
        # density_temperature.py:137-146: response x exposure time, cast to fp32
        self.register_buffer('response_logte', torch.as_tensor(logte).float(), persistent=False)
        self.register_buffer('response_table', torch.as_tensor(tresp * aia_exp_time).float(), persistent=False)

    # ---- .snf compatibility in both directions (sunerf.py:62-74 pickles this object) ---------------------------------
    def __getstate__(self):
        """What the reference's class needs besides modules and scalars is ``self.response`` (density_temperature.py:132-146,
        read at :248): one ``xitorch`` interpolator per channel.  Where xitorch is installed -- any environment that runs the
        reference -- they are built through its public constructor exactly as the reference builds them, so that a state
        written here renders in the reference; elsewhere the file simply lacks them (and still loads here)."""
        st = self.__dict__.copy()
        if st.get('response_set') is not None:      # no AIA interpolators to offer: such a state renders here only
            return st
        try:
            from xitorch.interpolate import Interp1D
        except ImportError:
            return st
        x, y = self._buffers['response_logte'], self._buffers['response_table']
        st['response'] = {c: Interp1D(x[i].clone(), y[i].clone(), method='linear', extrap=0) for i, c in enumerate(CHANNELS)}
        return st

    def __setstate__(self, state):
        """A state written by the REFERENCE has the interpolators but not this class's table buffers: take the table out of
        them, or read the file again like the constructor."""
        self.__dict__.update(state)
        self.__dict__.setdefault('response_set', None)      # states written before response sets existed
        if self.response_set is not None:
            return
        if 'response_logte' in self._buffers and 'response_table' in self._buffers:
            return
        tables = _tables_from_interpolators(state['response']) if isinstance(state.get('response'), dict) else None
        if tables is None:
            logte, tresp = read_aia_temp_resp("sunerf/data/aia_temp_resp.genx")
            tables = torch.as_tensor(logte).float(), torch.as_tensor(tresp * 2.9).float()     # the constructor's default exposure
        where = next((p.device for p in self.parameters()), torch.device('cpu'))
        self.register_buffer('response_logte', tables[0].to(where), persistent=False)
        self.register_buffer('response_table', tables[1].to(where), persistent=False)

    def _tables(self):
        """What the DT passes interpolate in: the response set, or the AIA pair of buffers."""
        if self.response_set is not None:
            return self.response_set
        return (self.response_logte, self.response_table)

    def _table_device(self):
        if self.response_set is None:
            return self.response_logte.device
        return next((p.device for p in self.parameters()), torch.device('cpu'))

    def regularization(self, distance, regularizing_quantity):
        return torch.relu(distance[:, :] - 1.25 / self.Rs_per_ds) * torch.relu(regularizing_quantity)

    def forward(self, rays_o, rays_d, times, wavelengths=None):
        """base_tracing.py:46-111 for the DT subclass: same 8 output keys, images are (N, W)."""
        if wavelengths is None:
            raise ValueError('DensityTemperatureRadiativeTransfer needs the wavelengths of every ray')
        if self._hooks_replaced(DensityTemperatureRadiativeTransfer):   # a subclass with its own raw2outputs / _render / regularization
            return SuNeRFRendering.forward(self, rays_o, rays_d, times, wavelengths)
        tables = self._tables()
        reg_radius = 1.25 / self.Rs_per_ds
        z_vals = self.sampler.z_vals(rays_o, rays_d)
        coarse = dt_pass(self.coarse_model, tables, self.pixel_intensity_factor, rays_o, rays_d, times, z_vals, wavelengths,
                         reg_radius, want_epilogues=False)
        new_z, z_comb = self.sampler_hierarchical.resample(z_vals, coarse['weights'])
        fine = dt_pass(self.fine_model, tables, self.pixel_intensity_factor, rays_o, rays_d, times, z_comb, wavelengths,
                       reg_radius, want_epilogues=True)
        return {'z_vals_stratified': z_vals, 'coarse_image': coarse['image'], 'z_vals_hierarchical': new_z,
                'fine_image': fine['image'], 'image': fine['image'], 'height_map': fine['height_map'],
                'absorption_map': fine['absorption_map'], 'regularization': fine['regularization']}

    # ---- line-of-sight DEM (sunerf_hip/dem.py) ---------------------------------------------------------------
    def dem_nodes(self, logt_nodes=None):
        """The log T nodes of a DEM as a float32 device vector: ``logt_nodes``, or the response table's own grid."""
        if logt_nodes is None:
            if self.response_set is None:
                return self.response_logte[0].contiguous()
            grid = self.response_set.shared_grid()
            if grid is None:
                raise ValueError('the channels of the response set have different log T grids: pass logt_nodes')
            logt_nodes = grid
        return torch.as_tensor(logt_nodes, dtype=torch.float32).to(self._table_device()).contiguous()

    def attenuation_scalar(self, attenuation_wavelength=None):
        """The fine model's ``log_absortpion`` scalar of channel ``attenuation_wavelength`` as a one-element device tensor
        (no host read), or None for an optically thin DEM."""
        if attenuation_wavelength is None:
            return None
        try:
            key = str(int(attenuation_wavelength))
            ok = float(attenuation_wavelength) == int(attenuation_wavelength)
        except (TypeError, ValueError):
            key, ok = repr(attenuation_wavelength), False
        if not ok or key not in self.fine_model.log_absortpion:
            raise ValueError(f'attenuation_wavelength {attenuation_wavelength!r} is not a channel of the model '
                             f'({", ".join(self.fine_model.log_absortpion.keys())})')
        return self.fine_model.log_absortpion[key].detach().float().reshape(1)

    @torch.no_grad()
    def fine_raw(self, rays_o, rays_d, times, z_vals):
        """The fine field's ``raw`` (N, S, 2) at the samples, without the base offsets, obtained the way ``dt_pass`` obtains
        it: the fused MLP kernel for a ``NeRF_DT``, ``field_on_rays`` for a ``SimpleStar`` / ``MHDModel``."""
        model = self.fine_model
        if hasattr(model, 'field_on_rays'):
            return _field_raw(model, rays_o, rays_d, z_vals, times)
        return ops.emission_render_fwd(model.packed(), rays_o, rays_d, times, z_vals, 0.0, want_raw=True,
                                       probe_sensitivity=2.0)['raw']

    @torch.no_grad()
    def render_dem(self, rays_o, rays_d, times, logt_nodes=None, attenuation_wavelength=None, r_range=(0., float('inf'))):
        """The thermal structure behind every pixel of ``forward``: the same samples (sampler -> coarse pass -> hierarchical
        resample), the fine field's ``raw`` on them, and ``sunerf_hip.dem.dem_integral`` with the model's base offsets.
        Forward only.

        ``logt_nodes``: (K,) strictly increasing log T grid (default: the response table's, on which ``dem`` folded with a
        channel's response row, times ``volumetric_constant * pixel_intensity_factor``, is ``forward``'s image of an optically
        thin channel).  ``attenuation_wavelength``: attenuate with that channel's ``log_absortpion`` (then the identity holds
        for that channel).  ``r_range``: radius mask in model units.
        Returns ``dem`` (N, K), ``em``, ``logt_mean``, ``column`` (N,), ``logt_nodes`` (K,) and ``z_vals`` (N, S)."""
        from sunerf_hip.dem import dem_integral
        if self._hooks_replaced(DensityTemperatureRadiativeTransfer):
            raise TypeError('render_dem needs the built-in density-temperature hooks and a NeRF_DT or field model')
        nodes = self.dem_nodes(logt_nodes)
        log_abs = self.attenuation_scalar(attenuation_wavelength)
        tables = self._tables()
        z_vals = self.sampler.z_vals(rays_o, rays_d)
        # the coarse weights = relu(inf0) / sum do not depend on the channel: one present channel keeps the pass cheap
        cheap = ops.AIA_WAVELENGTHS[2] if self.response_set is None else self.response_set.codes[0]
        wl = torch.full((z_vals.shape[0], 1), float(cheap), dtype=torch.float32, device=z_vals.device)
        coarse = dt_pass(self.coarse_model, tables, self.pixel_intensity_factor, rays_o, rays_d, times, z_vals, wl,
                         1.25 / self.Rs_per_ds, want_epilogues=False)
        _, z_comb = self.sampler_hierarchical.resample(z_vals, coarse['weights'])
        raw = self.fine_raw(rays_o, rays_d, times, z_comb)
        model = self.fine_model
        out = dem_integral(raw, z_comb, nodes, (model.base_log_density, model.base_log_temperature), log_abs, rays_o, rays_d,
                           r_range)
        out.update(logt_nodes=nodes, z_vals=z_comb)
        return out

    # ---- per-pixel DEM inversion of images (sunerf_hip/dem_inversion.py) ------------------------------------------
    def channel_indices(self, wavelengths=None):
        """Rows of the response table for ``wavelengths`` (default: all of ``ops.AIA_WAVELENGTHS``); an unknown channel raises
        like :meth:`attenuation_scalar`."""
        if self.response_set is not None:      # by code
            return self.response_set.index_of(self.response_set.codes if wavelengths is None else list(wavelengths))
        rows = []
        for w in (ops.AIA_WAVELENGTHS if wavelengths is None else wavelengths):
            try:
                ok = float(w) == int(w) and int(w) in ops.AIA_WAVELENGTHS
            except (TypeError, ValueError):
                ok = False
            if not ok:
                raise ValueError(f'wavelength {w!r} is not a channel of the model '
                                 f'({", ".join(str(c) for c in ops.AIA_WAVELENGTHS)})')
            rows.append(ops.AIA_WAVELENGTHS.index(int(w)))
        return rows

    @torch.no_grad()
    def inversion_response(self, wavelengths=None, logt_nodes=None):
        """``G`` (M, K) float64 of :meth:`invert_dem`: ``volumetric_constant * pixel_intensity_factor`` times the channels'
        response rows on the nodes (``dem_inversion.response_on_nodes``), so that ``G @ dem`` is ``forward``'s optically thin
        image of a line-of-sight DEM ``dem``."""
        from sunerf_hip.dem_inversion import response_on_nodes
        rows = self.channel_indices(wavelengths)
        nodes = self.dem_nodes(logt_nodes)
        if self.response_set is not None:
            resp = self.response_set.on_nodes(nodes)[rows].to(nodes.device)
        else:
            resp = response_on_nodes(self.response_logte[rows], self.response_table[rows], nodes)
        vol_c = self.fine_model.volumetric_constant.detach().to(device=resp.device, dtype=torch.float64)
        return resp * (vol_c * float(self.pixel_intensity_factor))

    @torch.no_grad()
    def invert_dem(self, images, wavelengths=None, logt_nodes=None, errors=None, **solver):
        """The classical per-pixel DEM inversion of ``images`` (..., M), the channels ``wavelengths`` (default: all seven of
        ``ops.AIA_WAVELENGTHS``, in that order) of ``forward``'s image or of observations in its units:
        ``sunerf_hip.dem_inversion.invert_dem`` with :meth:`inversion_response`; ``errors`` and ``**solver`` (``lam``, ``prior``,
        ``chi2_target``, ``lam_range``, ...) go through.  This is the OPTICALLY THIN inversion: the model's ``log_absortpion`` is
        not inverted, so compare with ``render_dem`` without ``attenuation_wavelength``.  On the default nodes
        ``dem.fold(result['dem'], response rows) * constants`` is comparable with ``forward``'s image and ``result['dem']`` /
        ``em`` / ``logt_mean`` with ``render_dem``'s, key for key."""
        from sunerf_hip.dem_inversion import invert_dem
        G = self.inversion_response(wavelengths, logt_nodes)
        if not isinstance(images, torch.Tensor) or images.dim() < 1 or images.shape[-1] != G.shape[0]:
            raise ValueError(f'images must be (..., {G.shape[0]}): one value per channel')
        return invert_dem(images, G, self.dem_nodes(logt_nodes), errors, **solver)

    def _render(self, model, query_points, rays_d, rays_o, z_vals, wavelengths):
        """density_temperature.py:148-190: ``model.forward`` at the query points -- inferences with the base offsets, the
        absorption scalars, the volumetric constant -- plus ``z_vals`` / ``rays_d`` / ``wavelengths`` into ``raw2outputs``."""
        inferences, state = field_on_query_points(model, query_points, rays_o, rays_d, z_vals)
        return self.raw2outputs(inferences=inferences, z_vals=z_vals, rays_d=rays_d, wavelengths=wavelengths, **state)

    def raw2outputs(self, inferences, log_abs, vol_c, z_vals, rays_d, wavelengths, **kwargs):
        """density_temperature.py:192-271 on the state ``NeRF_DT.forward`` returns (``inferences`` (N, S, 2) with the base
        offsets added, the ``log_absortpion`` ParameterDict, ``volumetric_constant``): ``{'image' (N,W), 'weights',
        'regularizing_quantity'}``; differentiable through ``image`` (sunerf_dt_integral_fwd / _bwd)."""
        return dt_raw2outputs(self._tables(), self.pixel_intensity_factor, inferences, log_abs,
                              vol_c, z_vals, rays_d, wavelengths)
