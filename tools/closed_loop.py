"""The reference's validation experiment in small (evaluation/image_render.py:264-293, stash/metrics_simulation.py): a ground-truth
field is rendered from K viewpoints, a model is trained on those frames, an unseen viewpoint is compared -- every stage on the
device.  ``--views`` frames from as many longitudes go into an ``ObservationSet`` without leaving the device; view ``K // 6`` is
held out; the module is trained with ``fit_steps`` on the pool (``reshuffle='rays'``: a fresh permutation of all rays per epoch);
the held-out view is scored with ``validation_metrics`` before and after.

``--module dt`` (default): ``SimpleStar`` frames (7 AIA channels, the DT integral) rendered by a ``ModelLoader``
(``add_rendered_view``), ``DensityTemperatureSuNeRFModule`` (NeRF_DT 8 x ``--d-filter``); the AIA response table comes from the
data fixture tests/golden/g9_simple_star.npz.  ``--module emission``: frames of the analytic target of tools/mini_train.py
(limb-darkened disk + exponential corona) evaluated on the views' own rays, ``EmissionSuNeRFModule``.  One JSON line.

``--baseline``: also the reprojection baseline of the held-out view (``ObservationSet.baseline_metrics``: the synchronic map of
the training views seen from the held-out pose), scored as ``validation_metrics`` scores the model -- the same
images, the MSE over all channels, the SSIM of channel 0 -- and printed next to the model's scores.

``--instrument SPEC`` (``sunerf_hip.instrument.Instrument.from_spec``, e.g.
``fwhm=2.5,bin=2,exposure=2.9,dn_per_photon=1.2,read_noise=1.2,unit=200``): the loop is run a second time with every training
view rendered at ``bin`` times the frame's resolution and passed through the instrument -- PSF, binning, photon and read noise,
seed = the view's index -- before ``ObservationSet.add_view``.  ``unit`` counts photons per second for an image value of one
(the frames are of order one).  The held-out view stays the clean render, so its score says what the noise costs the
reconstruction; it is printed next to the clean run's.

``--through-instrument`` (with ``--instrument``): a third run trains on the same observed views THROUGH the instrument
(DESIGN.md 8p): ``ObservationSet.patch_pool`` hands out patches of ``--patch`` detector pixels as the rays of their sub-pixel
windows, PSF halo included, and the loss compares ``instrument(render)`` with the observed pixels -- forward-model deconvolution.
A step renders ``patches_per_batch hw ww`` rays (``rays_per_step`` in the report) against ``--batch`` of the ray runs;
``--through-steps`` sets its step count apart from ``--steps`` for a comparison at equal rays rendered.  Every instrument run is
also scored on the clean held-out view rendered at ``bin`` times the resolution (``after_fine``): what the model knows about the
scene in front of the telescope.

``--likelihood observed|model`` (with ``--instrument``): the instrument runs -- on rays and, with ``--through-instrument``, on
patches -- train on the noise likelihood of that instrument (``sunerf_hip.likelihood.NoiseLikelihood``, gains frozen at 1) in
place of the MSE; their reports carry ``likelihood`` and the reduced chi-square of the last step.

``--lambda-ssim L`` (with ``--through-instrument``): the patch run adds ``L (dssim(coarse) + dssim(fine))`` to its loss, the
structural term of DESIGN.md 8r with a window of ``--ssim-window`` detector pixels (the emission module on its asinh-stretched
images; the DT module on its images of order one, data range 1); its report carries ``lambda_ssim`` and the mean SSIM of the last
step's patches.  Ray runs have no neighbouring pixels and ignore it.

``--deconvolve N|auto`` (with ``--instrument``): a further run, the classical alternative to training through the instrument
(DESIGN.md 8s).  The same observed training views are deconvolved first -- ``Instrument.deconvolve``, Richardson-Lucy against
the instrument's PSF, binning and noise model, ``N`` updates, or ``auto``: at most 200, stopped per channel by the discrepancy
rule -- added on the ``bin`` times finer frame ``Instrument.latent_grid`` describes, and trained on rays with the pixel loss (a
deconvolved pixel no longer follows the detector's noise model, so ``--likelihood`` does not apply to this run).  Its report
carries the updates applied and the deviance per valid pixel of every view and channel.

``--cosmic-rays RATE,AMP [--despike median|nan]`` (with ``--instrument``): a further ray run on the same observed training views
with particle hits (``sunerf_hip.despike.add_cosmic_rays``: tracks of 1 to 4 pixels on ``RATE`` of the pixels, ``AMP`` times the
pixel's sigma each, seeded by the view).  Without ``--despike`` the views are trained on as they are; with it they go through
``Instrument.despike`` first -- ``median`` inpaints the flagged pixels, ``nan`` drops their rays from the pool.  Its
report (``cosmic_rays``) carries the pixels hit, flagged and rightly flagged of every view.

``--fit-psf FWHM0`` (with ``--through-instrument``; a Gaussian ``--instrument``): the PSF as a trainable part of the model
(DESIGN.md 8t).  Three patch runs on the same observed views, one seed each: the right PSF (the ``through_instrument`` run above),
a wrong PSF held fixed (a Gaussian of ``FWHM0`` in place of the instrument's own width), and the wrong PSF fitted -- a
``FittedInstrument`` over ``TrainablePSF.gaussian(FWHM0, rate=--psf-rate)`` handed to the module as ``psf_models``, so that the
optimiser of the network moves ``log_fwhm`` too.  The report (``fit_psf``) carries the fitted ``fwhm`` per step count and the
held-out scores of the two runs beside those of the right PSF.

``--pointing-error PX [--coalign]``: the pointing of the views taken on trust, and what co-alignment does about it.
Every training view's ``crpix`` is displaced by a uniform draw in +-``PX`` pixels per axis (``default_rng(0)``) -- the images stay
what the true pointing sees.  A further ray run trains on the wrong pointing; with ``--coalign`` one more trains after
``ObservationSet.coalign_views`` (``--coalign-passes`` passes against the reprojection baseline, no anchor) has moved the grids.
The report (``pointing``) carries the held-out scores of each run beside the true pointing's and the RMS residual pointing error
in pixels before and after ``coalign_views``.  One seed each.

    python tools/closed_loop.py [--module dt|emission] [--views 8] [--size 64] [--steps 300] [--batch 2048] [--d-filter 256] [--baseline]
                                [--instrument SPEC [--through-instrument] [--patch 16] [--patches-per-batch N] [--through-steps K]]
                                [--likelihood observed|model] [--lambda-ssim L [--ssim-window 7]] [--deconvolve N|auto] [--skip-clean]
                                [--cosmic-rays RATE,AMP [--despike median|nan]]
                                [--fit-psf FWHM0 [--psf-rate 20]]
                                [--pointing-error PX [--coalign [--coalign-passes 2] [--max-shift 8]]]
"""
import argparse
import json
import math
import os
import re
import sys
import time

import numpy as np
import torch

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(R, '2024-hl-spi3s-sunerf_amd'))
from sunerf.evaluation.loader import ModelLoader                                  # noqa: E402
from sunerf.model.model import NeRF_DT                                            # noqa: E402
from sunerf.model.stellar_model import SimpleStar                                 # noqa: E402
from sunerf.model.sunerf import DensityTemperatureSuNeRFModule, EmissionSuNeRFModule, fit_steps   # noqa: E402
from sunerf.rendering.density_temperature import DensityTemperatureRadiativeTransfer   # noqa: E402
from sunerf_hip import ops                                                        # noqa: E402
from sunerf_hip.feed import training_batches                                      # noqa: E402
from sunerf_hip.instrument import Instrument                                      # noqa: E402
from sunerf_hip.likelihood import NoiseLikelihood                                 # noqa: E402
from sunerf_hip.observations import ObservationSet, hold_out_index, resampled_grid   # noqa: E402

WL = [94., 131., 171., 193., 211., 304., 335.]


def held_out_scores(module, obs, batch_size):
    (val,) = obs.validation_batches(batch_size)
    module.validation_dataset_mapping = {0: 'test_image'}
    module.validation_epoch_end([module.validation_step(b, i) for i, b in enumerate(val['batches'])])
    scores = {k: float(v) for k, v in module.validation_metrics(val['image_shape']).items()}
    stored = module.validation_outputs['test_image']
    scores['mean_target'], scores['mean_fine_image'] = stored['target_image'].mean().item(), stored['fine_image'].mean().item()
    return scores


def baseline_scores(module, obs):
    """What the surface assumption alone reaches on the held-out view, under the scoring of ``validation_metrics``."""
    def as_scored(planes):                                                 # (C, H, W) -> the images the callback scores
        image = planes.permute(1, 2, 0)
        return module._validation_images(image, image)[0].permute(2, 0, 1)
    scores = obs.baseline_metrics(data_range=1.0, normalize=as_scored)
    loss = scores['mse'].mean()
    return {'baseline.loss': loss.item(), 'baseline.ssim': scores['ssim'][0].item(), 'baseline.psnr': (-10. * torch.log10(loss)).item()}


def observed_view(instrument, render, grid, index, n_views, deconvolve=None, cosmic=None):
    """``(planes, grid of the planes)``: ``render(grid)`` -> planes (C, H, W) of view ``index`` on ``grid``; a training view of an
    instrument run is rendered ``bin`` times finer over the same field of view and observed, the held-out view and a clean run
    are not.  ``deconvolve`` (``iterations``, ``stop``, ``log``): the observed view is deconvolved and lies on the latent grid.
    ``cosmic`` (``rate``, ``amplitude``, ``despike``, ``log``): the observed view takes particle hits of ``amplitude`` sigma on
    ``rate`` of its pixels and is, with ``despike`` 'median' or 'nan', cleaned by ``Instrument.despike`` before it is used."""
    if instrument is None or index == hold_out_index(n_views):
        return render(grid), grid
    h, w = grid['shape']
    fine = resampled_grid(grid, (h * instrument.bin, w * instrument.bin))
    image = instrument.observe(render(fine).contiguous(), seed=index)['image']
    if cosmic is not None:
        from sunerf_hip.despike import add_cosmic_rays
        image, truth = add_cosmic_rays(image, cosmic['rate'], cosmic['amplitude'], sigma=instrument.errors(image, channel_axis=0), seed=index)
        entry = {'view': index, 'hit': int(truth.sum())}
        if cosmic['despike'] is not None:
            out = instrument.despike(image, fill=cosmic['despike'])
            flagged = (out['mask'] & 1) != 0
            entry.update(flagged=int(flagged.sum()), hits_flagged=int((flagged & truth).sum()), passes=out['passes'].tolist(),
                         converged=out['converged'].tolist(), unfilled=out['n_unfilled'].tolist())
            image = out['image']
        cosmic['log'].append(entry)
    if deconvolve is None:
        return image, grid
    out = instrument.deconvolve(image, iterations=deconvolve['iterations'], stop=deconvolve['stop'])
    deconvolve['log'].append({'view': index, 'iterations': out['iterations'].tolist(), 'deviance': out['deviance'].tolist(),
                              'stopped': out['stopped'].tolist()})
    return out['image'], instrument.latent_grid(grid)


def density_temperature_problem(args, grid, poses, instrument=None, mode=None, deconvolve=None, psf_models=None, cosmic=None):
    fx = np.load(os.path.join(R, 'tests', 'golden', 'g9_simple_star.npz'))
    table = (fx['aia_logte'], fx['aia_tresp'])
    cfg = dict(sampling_config={'type': 'stratified', 'n_samples': 64, 'perturb': True},
               hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 128, 'perturb': False})
    star = DensityTemperatureRadiativeTransfer(Rs_per_ds=1, model=SimpleStar, model_config={}, response_table=table,
                                               **{k: dict(v) for k, v in cfg.items()}).cuda()
    with torch.no_grad():
        for m in (star.coarse_model, star.fine_model):
            for w in ops.AIA_WAVELENGTHS:
                m.log_absortpion[str(w)].copy_(torch.from_numpy(fx[f'la__{w}']))
            m.volumetric_constant.copy_(torch.from_numpy(fx['vol_c']))
    truth = ModelLoader(rendering=star, model=star.fine_model, ref_map=grid)
    first = truth.render_observer_image(poses[0][0], poses[0][1], 0.0, wl=np.array(WL), as_numpy=False)['image']
    scale = 1.0 / first.abs().max().item()           # images of order one, as the reference's loaders normalise them
    obs = ObservationSet(Rs_per_ds=1.0, seconds_per_dt=1.0, device='cuda')

    def render_of(lat, lon):
        def render(g):
            frame = truth.render_observer_image(lat, lon, 0.0, wl=np.array(WL), resolution=g['shape'], as_numpy=False)['image']
            return frame.permute(2, 0, 1) * scale
        return render
    for index, (lat, lon) in enumerate(poses):
        if instrument is None:
            obs.add_rendered_view(truth, lat, lon, 0.0, wl=np.array(WL), scale=scale)
            continue
        planes, view_grid = observed_view(instrument, render_of(lat, lon), grid, index, len(poses), deconvolve, cosmic)
        obs.add_view(planes, lat, lon, time=0.0, grid=view_grid, wavelengths=np.array(WL))
    module = DensityTemperatureSuNeRFModule(Rs_per_ds=1.0, seconds_per_dt=1.0, image_scaling_config={}, model=NeRF_DT,
                                            pixel_intensity_factor=1e10, response_table=table,
                                            model_config={'d_filter': args.d_filter},
                                            lr_config={'start': 5e-4, 'end': 5e-5, 'iterations': args.steps},
                                            likelihood=None if mode is None else NoiseLikelihood(instrument, codes=[int(w) for w in WL], mode=mode),
                                            lambda_ssim=args.lambda_ssim, ssim_window=args.ssim_window,
                                            ssim_data_range=1.0 if args.lambda_ssim > 0 else None, psf_models=psf_models,
                                            **{k: dict(v) for k, v in cfg.items()}).cuda()
    return obs, module, render_of, np.array(WL)


def emission_problem(args, grid, poses, instrument=None, mode=None, deconvolve=None, psf_models=None, cosmic=None):
    from sunerf.evaluation.loader import linear_plate_scale_axes
    from sunerf_hip.rays import grid_rays, pose_spherical
    obs = ObservationSet(Rs_per_ds=1.0, seconds_per_dt=1.0, device='cuda')

    def render_of(lat, lon):
        def render(g):
            tx, ty = linear_plate_scale_axes(g, None, 'cuda')
            o, d = grid_rays(tx, ty, pose_spherical(-lon, lat, 215.03215567054764))
            b = torch.linalg.cross(o, d).norm(dim=-1) / d.norm(dim=-1)                    # impact parameter in solar radii
            image = torch.where(b < 1, 0.25 * torch.sqrt((1 - b * b).clamp_min(0)) + 0.06, 0.06 * torch.exp(-(b - 1) / 0.12))
            return image.reshape(1, *g['shape'])
        return render
    for index, (lat, lon) in enumerate(poses):
        planes, view_grid = observed_view(instrument, render_of(lat, lon), grid, index, len(poses), deconvolve, cosmic)
        obs.add_view(planes[0], lat, lon, time=0.0, grid=view_grid)
    module = EmissionSuNeRFModule(Rs_per_ds=1.0, seconds_per_dt=1.0, image_scaling_config={'vmax': 1, 'a': 0.005},
                                  sampling_config={'type': 'stratified', 'n_samples': 64, 'perturb': True},
                                  hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 128, 'perturb': True},
                                  model_config={'d_filter': args.d_filter},
                                  lr_config={'start': 5e-4, 'end': 5e-5, 'iterations': args.steps},
                                  likelihood=None if mode is None else NoiseLikelihood(instrument, mode=mode),
                                  lambda_ssim=args.lambda_ssim, ssim_window=args.ssim_window, psf_models=psf_models).cuda()
    return obs, module, render_of, None


def fine_scores(module, render, grid, pose, wavelengths, factor, batch_size):
    """The held-out pose rendered clean at ``factor`` times the resolution over the same field of view, scored like the
    held-out view itself."""
    h, w = grid['shape']
    fine = resampled_grid(grid, (h * factor, w * factor))
    obs = ObservationSet(Rs_per_ds=1.0, seconds_per_dt=1.0, device='cuda')
    planes = render(fine).contiguous()
    obs.add_view(planes if wavelengths is not None else planes[0], pose[0], pose[1], time=0.0, grid=fine, wavelengths=wavelengths)
    obs.hold_out(0)
    return held_out_scores(module, obs, batch_size)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--module', choices=('dt', 'emission'), default='dt')
    ap.add_argument('--views', type=int, default=8)
    ap.add_argument('--size', type=int, default=64)
    ap.add_argument('--steps', type=int, default=300)
    ap.add_argument('--batch', type=int, default=2048)
    ap.add_argument('--d-filter', type=int, default=256)
    ap.add_argument('--baseline', action='store_true')
    ap.add_argument('--instrument', metavar='SPEC', default=None)
    ap.add_argument('--through-instrument', action='store_true', help='a third run trained on patches through the instrument')
    ap.add_argument('--patch', type=int, default=16, help='detector pixels per patch and axis')
    ap.add_argument('--patches-per-batch', type=int, default=None, help='default: what brings a batch nearest to 8192 rays')
    ap.add_argument('--through-steps', type=int, default=None, help='steps of the through-instrument run (default: --steps)')
    ap.add_argument('--skip-clean', action='store_true', help='leave out the run on clean views')
    ap.add_argument('--likelihood', choices=('observed', 'model'), default=None,
                    help="the instrument runs train on the instrument's noise likelihood in place of the MSE")
    ap.add_argument('--lambda-ssim', type=float, default=0.0, help='weight of the structural (D-SSIM) term of the patch run')
    ap.add_argument('--ssim-window', type=int, default=7, help='side of the SSIM window in detector pixels (odd, 3 .. 11)')
    ap.add_argument('--deconvolve', metavar='N|auto', default=None,
                    help='a further run on Richardson-Lucy deconvolved views: N updates, or auto: the discrepancy rule')
    ap.add_argument('--fit-psf', type=float, metavar='FWHM0', default=None,
                    help='two further patch runs from a Gaussian PSF of this width: held fixed, and fitted beside the network')
    ap.add_argument('--cosmic-rays', metavar='RATE,AMP', default=None,
                    help='a further ray run on observed views with particle hits: RATE of the pixels, AMP sigma each')
    ap.add_argument('--despike', choices=('median', 'nan'), default=None, help='with --cosmic-rays: Instrument.despike the views first')
    ap.add_argument('--psf-rate', type=float, default=20.0, help='rate of the TrainablePSF: its log_fwhm moves at rate x the learning rate')
    ap.add_argument('--pointing-error', type=float, metavar='PX', default=None,
                    help="a further run with every training view's crpix displaced by a uniform draw in +-PX pixels")
    ap.add_argument('--coalign', action='store_true', help='with --pointing-error: one more run after ObservationSet.coalign_views')
    ap.add_argument('--coalign-passes', type=int, default=2)
    ap.add_argument('--max-shift', type=int, default=8, help='the window of coalign_views in pixels')
    args = ap.parse_args()
    if args.coalign and args.pointing_error is None:
        ap.error('--coalign needs --pointing-error PX')
    if args.pointing_error is not None and not args.pointing_error >= 0:
        ap.error('--pointing-error takes a number of pixels >= 0')
    if args.fit_psf is not None and not args.through_instrument:
        ap.error('--fit-psf needs --through-instrument')
    if args.fit_psf is not None and (not args.fit_psf > 0 or 'fwhm=' not in args.instrument or 'beta=' in args.instrument):
        ap.error('--fit-psf takes a width > 0 and needs a Gaussian --instrument SPEC (fwhm=..., no beta=)')
    if args.lambda_ssim > 0 and not args.through_instrument:
        ap.error('--lambda-ssim needs --through-instrument: only patch batches have neighbouring pixels')
    if args.likelihood is not None and args.instrument is None:
        ap.error('--likelihood needs --instrument SPEC')
    if args.through_instrument and args.instrument is None:
        ap.error('--through-instrument needs --instrument SPEC')
    cosmic = None
    if args.cosmic_rays is not None:
        if args.instrument is None:
            ap.error('--cosmic-rays needs --instrument SPEC')
        try:
            rate, amplitude = (float(v) for v in args.cosmic_rays.split(','))
        except ValueError:
            ap.error('--cosmic-rays takes RATE,AMP: the fraction of pixels hit and the amplitude in sigma')
        if not 0 <= rate <= 1 or not amplitude > 0:
            ap.error('--cosmic-rays takes a RATE in [0, 1] and an AMP above 0')
        cosmic = {'rate': rate, 'amplitude': amplitude, 'despike': args.despike, 'log': []}
    elif args.despike is not None:
        ap.error('--despike needs --cosmic-rays RATE,AMP')
    deconvolve = None
    if args.deconvolve is not None:
        if args.instrument is None:
            ap.error('--deconvolve needs --instrument SPEC')
        if args.deconvolve != 'auto' and not (args.deconvolve.isdigit() and int(args.deconvolve) <= 10000):
            ap.error('--deconvolve takes a number of updates (at most 10000) or auto')
        deconvolve = {'iterations': 200, 'stop': 'discrepancy', 'log': []} if args.deconvolve == 'auto' else \
            {'iterations': int(args.deconvolve), 'stop': None, 'log': []}
    grid = {'shape': (args.size, args.size), 'cdelt': (2.2 * 960. / args.size, 2.2 * 960. / args.size),
            'meta': {'t_obs': '2022-01-01T00:00:00.000'}}
    poses = [(0.1 * (k % 3 - 1), 0.3 - 6.2832 / args.views * k) for k in range(args.views)]
    report = {} if args.skip_clean else run(args, grid, poses, None)
    if args.pointing_error is not None:
        report['pointing'] = pointing_runs(args, grid, poses, report)
    if args.instrument is not None:
        keys = ('steps', 'rays_per_step', 'loss_first_10', 'loss_last_10', 'train_seconds', 'before', 'after', 'after_fine')
        if args.likelihood is not None:
            keys += ('likelihood', 'reduced_chi2')
        seen = run(args, grid, poses, Instrument.from_spec(args.instrument))
        clean = '' if args.skip_clean else (f"clean views PSNR {report['after']['validation.psnr']:.2f} dB, SSIM "
                                            f"{report['after']['validation.ssim']:.4f}; ")
        print(f"held-out view {seen['held_out'][0]}: {clean}views seen through the instrument ({args.instrument}) PSNR "
              f"{seen['after']['validation.psnr']:.2f} dB, SSIM {seen['after']['validation.ssim']:.4f}", file=sys.stderr)
        report['instrument'] = {'spec': args.instrument, **{k: seen[k] for k in keys}}
        if args.through_instrument:
            through = run(args, grid, poses, Instrument.from_spec(args.instrument), through=True)
            print(f"trained through the instrument, {through['steps']} steps of {through['rays_per_step']} rays: PSNR "
                  f"{through['after']['validation.psnr']:.2f} dB, SSIM {through['after']['validation.ssim']:.4f}; at bin times the "
                  f"resolution {through['after_fine']['validation.psnr']:.2f} dB against {seen['after_fine']['validation.psnr']:.2f} dB "
                  f"of ray training ({seen['steps']} steps of {seen['rays_per_step']} rays)", file=sys.stderr)
            more = ('patch', 'patches', 'dropped', 'halo_overhead') + (('lambda_ssim', 'train_ssim') if args.lambda_ssim > 0 else ())
            report['through_instrument'] = {k: through[k] for k in keys + more}
            if args.fit_psf is not None:
                report['fit_psf'] = fit_psf_runs(args, grid, poses, through, keys)
        if deconvolve is not None:
            dec = run(args, grid, poses, Instrument.from_spec(args.instrument), deconvolve=deconvolve)
            applied = [n for view in deconvolve['log'] for n in view['iterations']]
            print(f"views deconvolved first ({args.deconvolve}: {min(applied)} .. {max(applied)} updates), {dec['steps']} steps of "
                  f"{dec['rays_per_step']} rays: PSNR {dec['after']['validation.psnr']:.2f} dB, SSIM {dec['after']['validation.ssim']:.4f}; at "
                  f"bin times the resolution {dec['after_fine']['validation.psnr']:.2f} dB against "
                  f"{seen['after_fine']['validation.psnr']:.2f} dB of ray training on the observed views", file=sys.stderr)
            report['deconvolved'] = {'deconvolve': args.deconvolve, 'views': deconvolve['log'], **{k: dec[k] for k in keys if k in dec}}
        if cosmic is not None:
            hit = run(args, grid, poses, Instrument.from_spec(args.instrument), cosmic=cosmic)
            n_hit, n_found = sum(v['hit'] for v in cosmic['log']), sum(v.get('hits_flagged', 0) for v in cosmic['log'])
            cleaned = 'as they are' if args.despike is None else f"despiked (fill='{args.despike}', {n_found} of {n_hit} hit pixels flagged)"
            print(f"views with particle hits ({args.cosmic_rays}: {n_hit} pixels hit), {cleaned}: PSNR {hit['after']['validation.psnr']:.2f} dB, "
                  f"SSIM {hit['after']['validation.ssim']:.4f} against {seen['after']['validation.psnr']:.2f} dB, "
                  f"{seen['after']['validation.ssim']:.4f} without hits", file=sys.stderr)
            report['cosmic_rays'] = {'cosmic_rays': args.cosmic_rays, 'despike': args.despike, 'views': cosmic['log'],
                                     **{k: hit[k] for k in keys if k in hit}}
    print(json.dumps({'closed_loop': report}))


def pointing_runs(args, grid, poses, true_run):
    """The runs of ``--pointing-error``: wrong pointing as it is and, with ``--coalign``, after ``coalign_views``."""
    keys = ('steps', 'loss_first_10', 'loss_last_10', 'train_seconds', 'before', 'after')
    out = {'pointing_error_px': args.pointing_error}
    if true_run:
        out['true_pointing'] = {'after': true_run['after']}
    for name, coalign in (('wrong_pointing', False),) + ((('coaligned', True),) if args.coalign else ()):
        pointing = {'px': args.pointing_error, 'coalign': coalign, 'passes': args.coalign_passes, 'max_shift': args.max_shift}
        result = run(args, grid, poses, None, pointing=pointing)
        out[name] = {**{k: result[k] for k in keys}, **pointing['log']}
        rms = pointing['log']['rms_error_px_before'] if not coalign else pointing['log']['rms_error_px_after']
        print(f"pointing error +-{args.pointing_error} px, {name}: RMS pointing error {rms:.3f} px; PSNR "
              f"{result['after']['validation.psnr']:.2f} dB, SSIM {result['after']['validation.ssim']:.4f}"
              + (f" (true pointing: {true_run['after']['validation.psnr']:.2f} dB, {true_run['after']['validation.ssim']:.4f})" if true_run else ''),
              file=sys.stderr)
    return out


def displace_pointing(obs, pointing):
    """Moves the crpix of every training view by a seeded draw in +-px (the images stay); with ``coalign`` the set then co-aligns
    itself.  ``pointing['log']`` takes the RMS distance of crpix from the truth, in pixels, before and after."""
    from sunerf.evaluation.loader import linear_plate_scale_axes
    from sunerf_hip.coalign import shifted_grid
    rng = np.random.default_rng(0)
    truth = {i: obs.views[i].grid['crpix'] for i in obs.training_views}

    def rms():
        d = np.array([[obs.views[i].grid['crpix'][k] - truth[i][k] for k in (0, 1)] for i in truth])
        return float(np.sqrt((d ** 2).sum(axis=1).mean()))
    for i in truth:
        ex, ey = rng.uniform(-pointing['px'], pointing['px'], 2)
        view = obs.views[i]
        view.grid = shifted_grid(view.grid, ey, ex)
        view.tx, view.ty = linear_plate_scale_axes(view.grid, None, obs.device)
    log = pointing['log'] = {'rms_error_px_before': rms()}
    if pointing['coalign']:
        history = obs.coalign_views(passes=pointing['passes'], max_shift=pointing['max_shift'])
        log['rms_error_px_after'] = rms()
        log['passes'] = [{str(i): {'shift': list(r['shift']), 'status': r['status'], 'score': r['score']} for i, r in h.items()} for h in history]


def fit_psf_runs(args, grid, poses, right, keys):
    """The two further patch runs of ``--fit-psf``: the views are those the true instrument observed; the patches are seen through
    a Gaussian of ``FWHM0``, held fixed in one run and fitted in the other."""
    from sunerf_hip.psf_fit import FittedInstrument, TrainablePSF
    true = Instrument.from_spec(args.instrument)
    true_fwhm = float(re.search(r'fwhm=([^,]+)', args.instrument).group(1))
    wrong_spec = re.sub(r'fwhm=[^,]+', f'fwhm={args.fit_psf}', args.instrument)
    wrong = run(args, grid, poses, true, through=True, model_instrument=Instrument.from_spec(wrong_spec))
    radius = re.search(r'radius=([^,]+)', args.instrument)
    psf = TrainablePSF.gaussian(args.fit_psf, int(radius.group(1)) if radius else math.ceil(3 * max(args.fit_psf, true_fwhm)),
                                rate=args.psf_rate).cuda()
    scalars = {name: getattr(true, name) for name in ('unit', 'exposure', 'dn_per_photon', 'read_noise', 'pedestal', 'saturation')}
    fitted_instrument = FittedInstrument(psf, bin=true.bin, bin_mode=true.bin_mode, boundary=true.boundary, quantise=true.quantise, **scalars)
    fitted = run(args, grid, poses, true, through=True, model_instrument=fitted_instrument, psf_model=psf)
    out = {'true_fwhm': true_fwhm, 'start_fwhm': args.fit_psf, 'psf_rate': args.psf_rate,
           'right_psf': {k: right[k] for k in ('after', 'after_fine')},
           'wrong_psf_fixed': {k: wrong[k] for k in keys},
           'wrong_psf_fitted': {**{k: fitted[k] for k in keys}, 'fwhm_by_step': fitted['fwhm_by_step']}}
    for name in ('right_psf', 'wrong_psf_fixed', 'wrong_psf_fitted'):
        print(f"fit-psf, {name}: PSNR {out[name]['after']['validation.psnr']:.2f} dB, SSIM {out[name]['after']['validation.ssim']:.4f}; at bin "
              f"times the resolution {out[name]['after_fine']['validation.psnr']:.2f} dB", file=sys.stderr)
    print(f"fit-psf: FWHM {args.fit_psf} -> {fitted['fwhm_by_step'][-1][1]:.4f} (the instrument's: {true_fwhm})", file=sys.stderr)
    return out


def _recording_fwhm(batches, psf_model, steps, record):
    """``batches`` as they are; ``record`` takes (steps done, fwhm on the device) at eight step counts and at the end."""
    every = max(1, steps // 8)
    done = 0
    for batch in batches:
        if done % every == 0:
            record.append((done, psf_model.fwhm[0].clone()))
        yield batch
        done += 1
    record.append((done, psf_model.fwhm[0].clone()))


def run(args, grid, poses, instrument, through=False, deconvolve=None, model_instrument=None, psf_model=None, cosmic=None, pointing=None):
    """``instrument`` observes the views; ``model_instrument`` (default: the same) is what a patch run sees its renders through;
    ``psf_model``: the TrainablePSF of a FittedInstrument, trained beside the network; ``cosmic``: see ``observed_view``;
    ``pointing``: see ``displace_pointing``."""
    torch.manual_seed(0)
    problem = density_temperature_problem if args.module == 'dt' else emission_problem
    mode = args.likelihood if instrument is not None and deconvolve is None else None
    obs, module, render_of, wavelengths = problem(args, grid, poses, instrument, mode, deconvolve, psf_models=psf_model, cosmic=cosmic)
    obs.hold_out('reference')
    if pointing is not None:
        displace_pointing(obs, pointing)
    steps = args.steps
    if through:
        steps = args.steps if args.through_steps is None else args.through_steps
        pool = obs.patch_pool(instrument if model_instrument is None else model_instrument, patch=args.patch,
                              patches_per_batch=args.patches_per_batch, seed=0)
        rays_per_step = pool.rays_per_batch
    else:
        pool = obs.pool(batch_size=args.batch, seed=0, reshuffle='rays')
        rays_per_step = args.batch
    module.strict_finite_check = False
    before = held_out_scores(module, obs, 1 << 14)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    batches, fwhm_record = training_batches(pool, steps), []
    if psf_model is not None:
        batches = _recording_fwhm(batches, psf_model, steps, fwhm_record)
    losses = torch.stack(fit_steps(module, batches))
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    module.check_finite(module.optimizer)
    after = held_out_scores(module, obs, 1 << 14)
    extra = {}
    if module.likelihood is not None:
        extra.update(likelihood=module.likelihood.mode, reduced_chi2=module.likelihood.reduced_chi2(module.last_channel_stats).cpu().tolist())
    if instrument is not None:
        held = obs.held_out[0]
        extra['after_fine'] = fine_scores(module, render_of(*poses[held]), grid, poses[held], wavelengths, instrument.bin, 1 << 14)
    if through:
        extra.update(patch=pool.patch, patches=pool.n_patches, dropped=pool.dropped, halo_overhead=pool.halo_overhead)
        if module.last_ssim is not None:
            extra.update(lambda_ssim=module.lambda_ssim, train_ssim=(1.0 - module.last_ssim[:2]).cpu().tolist())
        if psf_model is not None:
            extra['fwhm_by_step'] = [[done, float(fwhm)] for done, fwhm in fwhm_record]
        return {'held_out': obs.held_out, 'steps': steps, 'rays_per_step': rays_per_step,
                'loss_first_10': losses[:10].mean().item(), 'loss_last_10': losses[-10:].mean().item(), 'train_seconds': seconds,
                'before': before, 'after': after, **extra}
    baseline = baseline_scores(module, obs) if args.baseline else None
    if baseline is not None and instrument is None:
        print(f"held-out view {obs.held_out[0]}: model PSNR {after['validation.psnr']:.2f} dB, SSIM {after['validation.ssim']:.4f}; "
              f"reprojection baseline PSNR {baseline['baseline.psnr']:.2f} dB, SSIM {baseline['baseline.ssim']:.4f}", file=sys.stderr)
    return {
        'module': args.module, 'views': args.views, 'held_out': obs.held_out, 'size': args.size, 'channels': pool.data['target_image'].shape[1], 'training_rays': pool.n_rays,
        'steps': args.steps, 'rays_per_step': rays_per_step, 'batch': args.batch, 'd_filter': args.d_filter,
        'epochs_built': pool.built_epoch + 1,
        'loss_first_10': losses[:10].mean().item(), 'loss_last_10': losses[-10:].mean().item(), 'train_seconds': seconds,
        'before': before, 'after': after, **extra, **({} if baseline is None else {'baseline': baseline})}


if __name__ == '__main__':
    main()
