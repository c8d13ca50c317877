"""Two instruments, one model: a small NeRF_DT is fitted to a SimpleStar that two instruments see from different directions,

  - AIA with three channels (codes 171, 193, 211: the rows of the AIA table), from longitude 0;
  - a synthetic second instrument with four channels on its own 25-node log T grid (codes 10171, 10195, 10284, 10304), from
    longitude 1.2 rad,

through one ResponseSet, and scored on a held-out view between them (longitude 0.6 rad) in all seven channels.  The same fit
with the second instrument's rays dropped shows what those rays add.  Prints the per-channel PSNR of the held-out view for both.

``--gain-error F``: the second instrument's views are multiplied by the hidden factor F, as two instruments never
share one intensity scale, and the fit on both instruments runs under the noise likelihood (``sunerf_hip.likelihood``, 'observed'
mode, every channel read as 1e4 photons at the mean intensity of the first view, read noise 1) -- once with every gain frozen at
1 and, with ``--fit-gains``, once with the second instrument's rows free.  Prints the recovered gains next to the held-out
scores; the held-out view carries no gain error, and the prediction scored is the model's own, before any gain.
Usage:  python tools/multi_instrument_loop.py [steps] [resolution] [--gain-error 1.3 [--fit-gains] [--gain-rate 50]]"""
import argparse
import os
import sys

import numpy as np
import torch

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(R, '2024-hl-spi3s-sunerf_amd'))
from sunerf.model.model import NeRF_DT                                            # noqa: E402
from sunerf.model.stellar_model import SimpleStar                                 # noqa: E402
from sunerf.model.sunerf import DensityTemperatureSuNeRFModule, fit_steps         # noqa: E402
from sunerf.rendering.density_temperature import DensityTemperatureRadiativeTransfer   # noqa: E402
from sunerf_hip.rays import observer_rays                                         # noqa: E402
from sunerf_hip.response import ResponseSet                                       # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('steps', type=int, nargs='?', default=300)
ap.add_argument('resolution', type=int, nargs='?', default=64)
ap.add_argument('--gain-error', type=float, default=None, help="hidden factor on the second instrument's views")
ap.add_argument('--fit-gains', action='store_true', help="a further fit with the second instrument's gains free")
ap.add_argument('--gain-rate', type=float, default=50.0, help='gain_rate of the likelihood: how much faster than the network the gains move')
args = ap.parse_args()
if args.fit_gains and args.gain_error is None:
    ap.error('--fit-gains needs --gain-error F')
steps, res = args.steps, args.resolution
g9 = np.load(os.path.join(R, 'tests', 'golden', 'g9_simple_star.npz'))
aia = ResponseSet.aia((g9['aia_logte'], g9['aia_tresp']), exposure=2.9)
AIA_CODES = (171, 193, 211)
grid = np.linspace(5.2, 7.4, 25) + 0.02 * np.sin(np.arange(25))                # the second instrument's own (non-uniform) grid
second = ResponseSet([(c, f'second {c}', grid, h * np.exp(-((grid - mu) / 0.3) ** 2) + 0.01 * h)
                      for c, mu, h in ((171, 5.95, 3e-25), (195, 6.15, 4e-25), (284, 6.35, 1e-25), (304, 5.6, 5e-26))])
rset = ResponseSet([ch for ch in aia.channels() if ch[0] in AIA_CODES]).concat(second, code_offset=10000)
A, B = [float(c) for c in AIA_CODES], [float(c) for c in rset.codes[3:]]


def sampling():          # fresh dicts: the rendering pops 'type' out of the ones it is given
    return dict(sampling_config={'type': 'stratified', 'n_samples': 32, 'perturb': False},
                hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 32})


torch.manual_seed(0)
star = DensityTemperatureRadiativeTransfer(Rs_per_ds=1.0, model=SimpleStar, response_set=rset, pixel_intensity_factor=1e10,
                                           model_config={'channels': rset, 'T0': 2.0e6}, **sampling()).cuda()


def thin(rendering, trainable):
    """Absorption of the size of g9's (optical depths below 1), fixed, like tools/simple_star_step.py."""
    with torch.no_grad():
        for m in (rendering.coarse_model, rendering.fine_model):
            for i, p in enumerate(m.log_absortpion.values()):
                p.fill_((i + 1) * 1e-9)
                p.requires_grad_(trainable)
            m.volumetric_constant.requires_grad_(trainable)


thin(star, False)


def view(phi, codes):
    o, d = observer_rays(res, theta=-0.1, phi=phi)
    wl = torch.tensor(codes + [0.] * (len(rset) - len(codes)), device='cuda')[:len(rset)].repeat(o.shape[0], 1).contiguous()
    t = torch.zeros(o.shape[0], 1, device='cuda')
    with torch.no_grad():
        image = star(o, d, t, wl)['image']
    return {'tracing': {'rays': torch.stack([o, d], 1), 'time': t, 'target_image': image, 'wavelength': wl}}


first, other, held_out = view(0.0, A), view(1.2, B), view(0.6, A + B)


def likelihood(free):
    """Every channel a detector that counts 1e4 photons at the mean intensity of the first view, read noise 1 DN."""
    from sunerf_hip.instrument import Instrument
    from sunerf_hip.likelihood import NoiseLikelihood
    unit = 1e4 / first['tracing']['target_image'][:, :len(A)].mean().item()
    return NoiseLikelihood(Instrument(unit=unit, read_noise=1.0), codes=rset, mode='observed', free=free, gain_rate=args.gain_rate)


def fit(batches, like=None):
    torch.manual_seed(1)
    lm = DensityTemperatureSuNeRFModule(Rs_per_ds=1.0, seconds_per_dt=1.0, image_scaling_config={}, model=NeRF_DT,
                                        response_set=rset, pixel_intensity_factor=1e10, lambda_regularization=0.0, likelihood=like,
                                        model_config={'d_filter': 128, 'channels': rset, 'base_log_density': 17.0,
                                                      'base_log_temperature': 6.0}, **sampling()).cuda()
    thin(lm.rendering, False)
    lm.strict_finite_check = False
    losses = fit_steps(lm, [batches[i % len(batches)] for i in range(steps)])
    tr = held_out['tracing']
    with torch.no_grad():
        got = lm.rendering(tr['rays'][:, 0].contiguous(), tr['rays'][:, 1].contiguous(), tr['time'], tr['wavelength'])['image']
    want = tr['target_image']
    mse = ((got - want) ** 2).mean(0)
    psnr = 10 * torch.log10(want.amax(0) ** 2 / mse.clamp_min(1e-30))
    return losses[0].item(), losses[-1].item(), psnr.cpu().tolist()


print(f'{steps} steps, {res} x {res} rays per view, NeRF_DT 8 x 128, 32 + 32 samples; held-out view PSNR [dB] per channel')
print(f'{"training rays":>28s} ' + ' '.join(f'{c:>7d}' for c in rset.codes) + '   loss first -> last')
for name, batches in (('both instruments', [first, other]), ('AIA only', [first])):
    l0, l1, psnr = fit(batches)
    print(f'{name:>28s} ' + ' '.join(f'{p:7.2f}' for p in psnr) + f'   {l0:.3e} -> {l1:.3e}')
if args.gain_error is not None:
    wrong = {'tracing': {**other['tracing'], 'target_image': other['tracing']['target_image'] * args.gain_error}}
    print(f"second instrument's views x {args.gain_error} (hidden); noise likelihood, 'observed' mode; gain_rate {args.gain_rate}")
    runs = [('gains frozen at 1', ())] + ([('second instrument free', [int(c) for c in B])] if args.fit_gains else [])
    for name, free in runs:
        like = likelihood(free)
        l0, l1, psnr = fit([first, wrong], like)
        print(f'{name:>28s} ' + ' '.join(f'{p:7.2f}' for p in psnr) + f'   {l0:.3e} -> {l1:.3e}')
        print(f'{"gains":>28s} ' + ' '.join(f'{g:7.4f}' for g in like.gains().cpu().tolist()))
