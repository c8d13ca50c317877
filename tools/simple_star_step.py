"""Training steps of DensityTemperatureSuNeRFModule(model=SimpleStar): 32768 rays x 7 channels, 64 + 128 samples, the stellar
parameters of both stars trained by the module's own optimiser (ClipAdam; the absorption scalars, of order 1e-9, and the
volumetric constants fixed: an Adam step of lr 1e-4 would change the optical depths by orders of magnitude).  Meant
for a kernel trace:  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/simple_star_step.py [steps]
(the first step warms up, the trace's per-kernel statistics then cover every step)."""
import os
import sys
import time

import numpy as np
import torch

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(R, '2024-hl-spi3s-sunerf_amd'))
from sunerf.model.stellar_model import SimpleStar                                 # noqa: E402
from sunerf.model.sunerf import DensityTemperatureSuNeRFModule, fit_steps         # noqa: E402
from sunerf_hip import ops                                                        # noqa: E402
from sunerf_hip.rays import observer_rays                                         # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
fx = np.load(os.path.join(R, 'tests', 'golden', 'g9_simple_star.npz'))
rays_o, rays_d = observer_rays(182)
rays_o, rays_d = rays_o[:32768].contiguous(), rays_d[:32768].contiguous()
n = rays_o.shape[0]
wl = torch.tensor([94., 131., 171., 193., 211., 304., 335.], device='cuda').repeat(n, 1)
lm = DensityTemperatureSuNeRFModule(Rs_per_ds=1.0, seconds_per_dt=1.0, image_scaling_config={}, model=SimpleStar,
                                    pixel_intensity_factor=1e10, response_table=(fx['aia_logte'], fx['aia_tresp']),
                                    model_config={}, sampling_config={'type': 'stratified', 'n_samples': 64, 'perturb': True},
                                    hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 128}).cuda()
with torch.no_grad():
    for m in (lm.rendering.coarse_model, lm.rendering.fine_model):
        for w in ops.AIA_WAVELENGTHS:
            m.log_absortpion[str(w)].copy_(torch.from_numpy(fx[f'la__{w}']))
        m.volumetric_constant.copy_(torch.from_numpy(fx['vol_c']))
        for p in [*m.log_absortpion.values(), m.volumetric_constant]:
            p.requires_grad_(False)
    target = lm.rendering(rays_o, rays_d, torch.zeros(n, 1, device='cuda'), wl)['image'] * 0.9
batch = {'tracing': {'rays': torch.stack([rays_o, rays_d], 1), 'time': torch.zeros(n, 1, device='cuda'),
                     'target_image': target, 'wavelength': wl}}
lm.strict_finite_check = False
fit_steps(lm, [batch])                     # warm-up
torch.cuda.synchronize()
t0 = time.perf_counter()
losses = fit_steps(lm, [batch] * steps)
torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / steps
sp = lm.rendering.fine_model.stellar_parameters
print(f'{steps} SimpleStar DT training steps, {n} rays x 7 channels, 64 + 128 samples: {dt * 1e3:.2f} ms/step, '
      f'loss {losses[0].item():.4e} -> {losses[-1].item():.4e}, fine h0 {sp["h0"].item():.6f} T0 {sp["T0"].item():.1f}')
