"""Mirror of the reference's ``sunerf/rendering/thompson.py`` on the fused HIP path: white-light Thomson scattering (total
brightness tB and polarised brightness pB, Howard & Tappin 2009) of the coronal electrons.

The reference's class cannot run: its constructor drops ``Rs_per_ds``, ``raw2outputs`` returns
neither ``image`` nor ``regularizing_quantity``, the time coordinate enters the radius, and its fp32 geometry loses up to
8 % at 215 solar radii.  Here those are resolved to the evident intent and the integral is ``csrc/thomson.hip``."""
import torch

from sunerf.rendering.base_tracing import SuNeRFRendering
from sunerf.rendering.functional import LN10, thomson_pass, thomson_raw2outputs


class ThompsonScattering(SuNeRFRendering):
    """thompson.py:7-109.  Same constructor (``Rs_per_ds`` and the base's keyword arguments) and the reference's three
    buffers, so that state-dict keys match a reference-built module."""

    def __init__(self, Rs_per_ds, **kwargs):
        super().__init__(Rs_per_ds=Rs_per_ds, **kwargs)
        C_0 = 1  # thompson.py:11 (the physical cross-section constant is commented out there)
        self.register_buffer('limb_darkening_coeff', torch.tensor(0.63, dtype=torch.float32))
        self.register_buffer('C_0', torch.tensor(C_0, dtype=torch.float32))
        self.register_buffer('solar_radius', torch.tensor(1. / Rs_per_ds, dtype=torch.float32))   # 1 R_sun in model units

    def _constants(self):
        return self.solar_radius, self.limb_darkening_coeff, self.C_0

    def _kappa(self) -> float:
        """rho = exp(kappa raw0): a NeRF answers log10 rho (thompson.py:39), a field module with ``field_on_rays``
        (SimpleStar, MHDModel) ln rho (stellar_model.py:88, mhd_model.py:137)."""
        return 1.0 if hasattr(self.fine_model, 'field_on_rays') else LN10

    def forward(self, rays_o, rays_d, times, wavelengths=None):
        """base_tracing.py:46-111 for the white-light subclass: the base's eight keys (images (N, 2) = (tB, pB),
        ``height_map`` = sum w r, ``absorption_map`` and ``regularization`` zero: the medium is optically thin) plus the fine
        pass's ``pixel_B`` (the image), ``pixel_density``, ``distance_from_sun`` and ``distance_from_obs``."""
        if self._hooks_replaced(ThompsonScattering):     # a subclass with its own raw2outputs / _render / regularization
            return SuNeRFRendering.forward(self, rays_o, rays_d, times, wavelengths)
        if wavelengths is not None:
            raise ValueError('ThompsonScattering takes no wavelengths (white light)')
        constants = self._constants()
        z_vals = self.sampler.z_vals(rays_o, rays_d)
        coarse = thomson_pass(self.coarse_model, constants, rays_o, rays_d, times, z_vals)
        new_z, z_comb = self.sampler_hierarchical.resample(z_vals, coarse['weights'].detach())   # no gradient (sampling.py:120)
        fine = thomson_pass(self.fine_model, constants, rays_o, rays_d, times, z_comb)
        n = z_comb.shape[0]
        return {'z_vals_stratified': z_vals, 'coarse_image': coarse['image'], 'z_vals_hierarchical': new_z,
                'fine_image': fine['image'], 'image': fine['image'],
                'height_map': fine['distance_from_sun'],                  # sum_j (rho_j / (M + 1e-10)) r_j
                'absorption_map': z_comb.new_zeros(n), 'regularization': torch.zeros_like(z_comb),
                'pixel_B': fine['pixel_B'], 'pixel_density': fine['pixel_density'], 'distance_from_sun': fine['distance_from_sun'],
                'distance_from_obs': fine['distance_from_obs']}

    def raw2outputs(self, raw, z_vals, rays_d, rays_o, query_points=None, **kwargs):
        """thompson.py:17-109 on a given ``raw`` (N, S, C): ``{pixel_B (N,2), pixel_density, distance_from_sun,
        distance_from_obs (N,), weights (N,S), image (= pixel_B), regularizing_quantity (ones)}``, differentiable w.r.t.
        ``raw`` through the first five (sunerf_thomson_integral_fwd / _bwd).  The sample radius is that of ``o + d z``, the
        spatial part of ``query_points``."""
        return thomson_raw2outputs(raw, z_vals, rays_o, rays_d, self._constants(), self._kappa())
