"""Mirror of the reference's ``sunerf/model/sunerf.py``: the Lightning-module API surface on the fused renderer.

``pytorch_lightning`` is optional: when it is importable the modules subclass ``LightningModule`` (so
``run_emission.py`` works unchanged); otherwise a minimal base with the same hook names is used and
``fit_steps`` below drives ``training_step`` / ``configure_optimizers`` / ``on_train_batch_end`` directly.
"""
import math
import os

import torch
from torch import nn
from torch.optim.lr_scheduler import ExponentialLR

from sunerf.model.model import NeRF
from sunerf.rendering.base_tracing import SuNeRFRendering
from sunerf.rendering.emission import EmissionRadiativeTransfer
from sunerf.rendering.density_temperature import DensityTemperatureRadiativeTransfer
from sunerf.train.scaling import ImageAsinhScaling
from sunerf_hip.train import ClipAdam, env_flag, training_loss

try:  # pragma: no cover - depends on the environment
    from pytorch_lightning import LightningModule
except Exception:  # ModuleNotFoundError in this image
    class LightningModule(nn.Module):
        """Stand-in with the hooks the reference modules use (log is a dict; no trainer)."""

        def __init__(self):
            super().__init__()
            self.logged = {}

        def log(self, name, value, **kwargs):
            self.logged[name] = value


class BaseSuNeRFModule(LightningModule):
    """sunerf.py:15-59."""

    def __init__(self, Rs_per_ds, seconds_per_dt, rendering: SuNeRFRendering, validation_dataset_mapping=None,
                 lr_config=None, likelihood=None, psf_models=None):
        super().__init__()
        self.Rs_per_ds = Rs_per_ds
        self.seconds_per_dt = seconds_per_dt
        self.rendering = rendering
        self.validation_dataset_mapping = validation_dataset_mapping
        self.validation_outputs = {}
        self.lr_config = {'start': 1e-4, 'end': 1e-5, 'iterations': 1e6} if lr_config is None else lr_config
        # a sunerf_hip.likelihood.NoiseLikelihood replaces the MSE of training_step by the detector model's
        # noise likelihood; a child module, so that checkpoints carry its log_gain.  None: the reference's loss.
        self.likelihood = likelihood
        # sunerf_hip.psf_fit.TrainablePSF models, one or a sequence: the PSFs of the FittedInstruments the patch
        # batches observe through, trained beside the network; a child ModuleList, so that checkpoints carry them.  None: nothing
        # is registered.
        if psf_models is None:
            self.psf_models = None
        else:
            self.psf_models = nn.ModuleList([psf_models] if isinstance(psf_models, nn.Module) else list(psf_models))
        self.last_channel_stats = None
        self._init_ssim()

    # the structural term of a patch batch: lambda_ssim (dssim(coarse) + dssim(fine)) beside the pixel loss; the
    # subclasses set the three attributes before this constructor runs.  Off (0.0) by default: nothing is launched then.
    lambda_ssim, ssim_window, ssim_data_range = 0.0, 7, None

    def _init_ssim(self):
        from sunerf_hip.ssim_loss import check_shape
        self.last_ssim = None
        if not float(self.lambda_ssim) >= 0.0:
            raise ValueError(f'lambda_ssim must be >= 0, got {self.lambda_ssim}')
        check_shape(self.ssim_window, self.ssim_window)
        if self.lambda_ssim > 0 and self._ssim_scaling()[0] is None:
            raise ValueError('lambda_ssim > 0 needs ssim_data_range: the images of this module have no natural scale')
        if self.lambda_ssim > 0 and self.likelihood is not None and bool(self.likelihood.free.any()):
            raise ValueError('lambda_ssim > 0 cannot be combined with a likelihood that has free gains: the structural term sees '
                             'the prediction, not the gained prediction')

    def _ssim_scaling(self):
        """``(data_range, asinh_scaling)`` of the structural term: this module's images as they are, in the user's range."""
        return self.ssim_data_range, None

    def _ssim_spec(self, tracing):
        """The patch geometry the structural term needs, or None where the term is off (a ray batch, or lambda_ssim = 0); raises
        before anything is rendered when the patches are smaller than the window."""
        self.last_ssim = None
        if not self.lambda_ssim > 0 or 'patch' not in tracing:
            return None
        spec = tracing['patch']
        if spec['P'] < self.ssim_window:
            raise ValueError(f"patches of {spec['P']} x {spec['P']} detector pixels are smaller than ssim_window = {self.ssim_window}")
        return spec

    def _with_ssim(self, loss, coarse, fine, target, spec):
        """``loss + lambda_ssim (dssim(coarse) + dssim(fine))`` on the rows the pixel loss got; ``loss`` itself where the term is
        off.  ``last_ssim``: the kernel's four statistics; the log carries the mean SSIM of the two images."""
        if spec is None:
            return loss
        from sunerf_hip.ssim_loss import ssim_loss
        data_range, asinh_scaling = self._ssim_scaling()
        term, stats, _ = ssim_loss(coarse, fine, target, spec['n'], spec['P'], data_range, window=self.ssim_window,
                                   asinh_scaling=asinh_scaling)
        self.last_ssim = stats
        self.log('train_ssim', {'coarse': 1.0 - stats[0], 'fine': 1.0 - stats[1]})
        return loss + (self.lambda_ssim * term).to(loss.dtype)

    def _trainable_parameters(self):
        """What the optimiser updates: the rendering's parameters, when any gain of the likelihood is free its log_gain, and the
        parameters of the psf_models that require a gradient."""
        params = list(self.rendering.parameters())
        if self.likelihood is not None and any(p.requires_grad for p in self.likelihood.parameters()):
            params += list(self.likelihood.parameters())
        if self.psf_models is not None:
            params += [p for p in self.psf_models.parameters() if p.requires_grad]
        return params

    def _likelihood_step(self, coarse, fine, target, codes, outputs, ssim_spec=None):
        """The loss section of a training step under ``self.likelihood``: no asinh scaling (the weighting replaces it)."""
        from sunerf_hip.likelihood import likelihood_loss
        loss, stats, self.last_channel_stats = likelihood_loss(
            coarse, fine, target, outputs['regularization'], self.likelihood, codes=codes, lambda_image=self.lambda_image,
            lambda_regularization=self.lambda_regularization, finite_check=_other_outputs(outputs))
        return self._finish_step(self._with_ssim(self._with_smoothness(loss), coarse, fine, target, ssim_spec), stats)

    def configure_optimizers(self):
        # sunerf.py:31: Adam(lr = start).  ClipAdam is the same update on one flat buffer (and can take the gradient
        # clip that run_emission.py:72 configures on the Trainer: fit_steps below sets optimizer.max_norm).
        self.optimizer = ClipAdam(self._trainable_parameters(), lr=self.lr_config['start'])
        self.optimizer.nonfinite_source = self._step_nonfinite_count      # (Lightning's step(closure) passes no count)
        self.scheduler = ExponentialLR(self.optimizer, gamma=(self.lr_config['end'] / self.lr_config['start']) ** (
                1 / self.lr_config['iterations']))
        return [self.optimizer], [self.scheduler]

    def configure_gradient_clipping(self, optimizer, *optimizer_idx, gradient_clip_val=None, gradient_clip_algorithm=None):
        """Lightning's ``gradient_clip_val`` (run_emission.py:72) as the clip FUSED into ``ClipAdam.step``: after the gradient
        all-reduce, on the total gradient, as the reference's ``dp`` run clips it.  Lightning's default would clip each rank's
        local gradient inside the closure, before the all-reduce.  Lightning 1.x passes ``optimizer_idx`` as the second
        positional argument, 2.x does not; both pass the clip settings as keywords."""
        if len(optimizer_idx) > 1:
            raise TypeError('configure_gradient_clipping takes gradient_clip_val / gradient_clip_algorithm as keywords')
        if not isinstance(optimizer, ClipAdam):
            raise TypeError(f'configure_gradient_clipping: expected the ClipAdam of configure_optimizers, got {type(optimizer)}')
        if gradient_clip_val and gradient_clip_algorithm == 'value':
            raise NotImplementedError("gradient_clip_algorithm='value' is not supported by the fused optimiser step: use 'norm'")
        optimizer.max_norm = float(gradient_clip_val) if gradient_clip_val else None

    def _with_smoothness(self, loss):
        """``loss + lambda_smoothness (coarse.smoothness() + fine.smoothness())`` for field models that have the prior
        (``GridField``: tomography's regulariser); the loss itself with the default ``lambda_smoothness = 0``."""
        lam = getattr(self, 'lambda_smoothness', 0.0)
        models = (self.rendering.coarse_model, self.rendering.fine_model)
        if lam > 0 and all(hasattr(m, 'smoothness') for m in models):
            loss = loss + lam * (models[0].smoothness() + models[1].smoothness())
        # the temporal prior of a grid with a time axis (``DynamicGridField``), likewise only when asked for
        lam_t = getattr(self, 'lambda_temporal', 0.0)
        if lam_t > 0 and all(hasattr(m, 'temporal_smoothness') for m in models):
            loss = loss + lam_t * (models[0].temporal_smoothness() + models[1].temporal_smoothness())
        return loss

    def _step_nonfinite_count(self):
        """This step's non-finite output count (device scalar) for ``ClipAdam.step(closure)``."""
        stats = getattr(self, 'last_stats', None)
        return None if stats is None else stats[5:6]

    # sunerf.py:105-107 asserts on NaN / Inf in every step, which costs a device -> host round trip.  True (default)
    # keeps that behaviour with ONE 4-byte read per step; False defers the check to ``check_finite()`` (the optimiser
    # step is skipped on the device for a step that saw non-finite outputs, so the weights stay intact meanwhile).
    strict_finite_check = True

    def _finish_step(self, loss, stats):
        self.last_stats = stats
        # under data parallelism the assert must be taken by every rank together (a rank that raised alone would leave the
        # others waiting in the all-reduce): there it is made after the optimiser step, on the all-reduced count
        if self.strict_finite_check and not _data_parallel():
            self.check_finite()
        self.log('loss', loss)
        self.log('train', {'coarse': stats[1], 'fine': stats[2], 'regularization': stats[3], 'psnr': stats[4]})
        return loss

    def check_finite(self, optimizer=None):
        """The reference's NaN / Inf assert (sunerf.py:105-107) as one 4-byte read: of this rank's counter, or -- given
        the optimiser after its step -- of the count summed over all ranks."""
        count = optimizer.nonfinite if optimizer is not None else getattr(self, 'last_stats', [None] * 6)[5]
        if count is not None:
            assert float(count) == 0, '! [Numerical Alert] an output contains NaN or Inf.'

    def on_train_batch_end(self, *args, **kwargs):
        # Under data parallelism the reference's NaN / Inf assert (sunerf.py:105-107) is taken HERE, after the optimiser step, on
        # the count the gradient all-reduce has summed over the ranks -- by every driver that ends a batch through this hook
        # (Lightning's closure-driven automatic optimisation as well as fit_steps below); _finish_step cannot do it before the
        # step without leaving the other ranks alone in the collective.
        optimizer = getattr(self, 'optimizer', None)
        if self.strict_finite_check and _data_parallel() and optimizer is not None:
            self.check_finite(optimizer)
        if self.strict_finite_check:
            from sunerf_hip import ops as _ops
            _ops.pipe_status()          # a pipelined backward launch that gave up (csrc/bwd_pipe.hip) is reported, not hidden
        if self.scheduler.get_last_lr()[0] > 5e-5:
            self.scheduler.step()
        self.log('Learning Rate', self.scheduler.get_last_lr()[0])

    def validation_epoch_end(self, outputs_list):
        """sunerf.py:42-54: concatenates the per-batch dicts of every validation set and files them under the set's name.
        Accepts a list of batch dicts (one validation set) or a list of such lists; nothing is stored when any set is empty."""
        per_set = outputs_list
        if per_set and isinstance(per_set[0], dict):
            per_set = [per_set]
        if not per_set or not all(len(batches) for batches in per_set):
            if per_set:
                self.validation_outputs = {}
            return
        self.validation_outputs = {
            self.validation_dataset_mapping[i]: {key: torch.cat([b[key] for b in batches]) for key in batches[0]}
            for i, batches in enumerate(per_set)}

    def validation_metrics(self, image_shape, name=None):
        """The scores the reference's TestImageCallback / TestMultiThermalImageCallback log (callback.py:46-56, 84-86), on the
        device: ``{'validation.loss', 'validation.ssim', 'validation.psnr'}`` as 0-d fp64 tensors of the validation set
        ``name`` (default: the first stored set), or None when nothing is stored.  The stored ``fine_image`` and
        ``target_image`` (N, C) are reshaped to ``image_shape`` (H, W) x C; the loss is the MSE over all channels, the SSIM that
        of channel 0 (data_range 1), psnr = -10 log10(loss).  Images are scored as fp32 after ``_validation_images``."""
        if not self.validation_outputs:
            return None
        name = next(iter(self.validation_outputs)) if name is None else name
        if name not in self.validation_outputs:
            return None
        from sunerf_hip.metrics import image_metrics
        outputs = self.validation_outputs[name]
        height, width = (int(v) for v in image_shape)
        fine, target = outputs['fine_image'], outputs['target_image']
        if height * width != fine.shape[0] or target.shape[0] != fine.shape[0]:
            raise ValueError(f'validation_metrics: image_shape {height} x {width} does not hold the {fine.shape[0]} stored rays')
        fine, target = self._validation_images(fine.reshape(height, width, -1), target.reshape(height, width, -1))
        scores = image_metrics(fine.permute(2, 0, 1), target.permute(2, 0, 1), 1.0)      # one call, every channel
        loss = scores['mse'].mean()
        return {'validation.loss': loss, 'validation.ssim': scores['ssim'][0], 'validation.psnr': -10. * torch.log10(loss)}

    def _validation_images(self, fine, target):
        """The images the callback scores, from the stored (H, W, C) outputs: as they are (TestMultiThermalImageCallback)."""
        return fine, target

    def on_load_checkpoint(self, checkpoint):
        """sunerf.py:56-59: non-strict restore (checkpoints written before a module gained a buffer still load)."""
        self.validation_outputs = {}
        self.load_state_dict(checkpoint['state_dict'], strict=False)


def _data_parallel() -> bool:
    import torch.distributed as dist
    return dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1


def _other_outputs(outputs):
    """Outputs that only take part in the finite check (the images and the regularization are read by the loss anyway)."""
    skip = ('coarse_image', 'fine_image', 'regularization', 'image')     # 'image' is fine_image (base_tracing.py:107)
    return [v for k, v in outputs.items() if k not in skip]


def _observed_windows(tracing, outputs):
    """The patch branch of a training step: the rendered windows seen through the batch's instrument.
    ``(coarse, fine, target)`` as ``[n P P, C]`` detector pixels; the regularization stays that of all rendered rays."""
    spec = tracing['patch']
    n, hw, ww, instrument = spec['n'], spec['hw'], spec['ww'], spec['instrument']

    def observe(image):
        windows = image.reshape(n, hw, ww, -1).permute(0, 3, 1, 2).contiguous()
        return instrument.expected_windows(windows).permute(0, 2, 3, 1).reshape(-1, windows.shape[1])
    target = tracing['target_image'].permute(0, 2, 3, 1).reshape(-1, spec['C'])
    return observe(outputs['coarse_image']), observe(outputs['fine_image']), target.contiguous()


def _patch_codes(tracing):
    """The codes of a patch batch's detector pixels ``[n P P, C]``: those of their patch -- the ``wavelength`` row of the first
    ray of each window, expanded over ``P x P``."""
    spec = tracing['patch']
    n, per_window, pixels = spec['n'], spec['hw'] * spec['ww'], spec['P'] * spec['P']
    first = tracing['wavelength'].reshape(n, per_window, -1)[:, 0]
    return first[:, None, :].expand(n, pixels, first.shape[-1]).reshape(n * pixels, -1).contiguous()


def save_state(sunerf: BaseSuNeRFModule, data_module, save_path):
    """sunerf.py:62-74: pickles the rendering module + data configuration (the ``.snf`` file)."""
    output_path = '/'.join(save_path.split('/')[0:-1])
    os.makedirs(output_path, exist_ok=True)
    torch.save({'rendering': sunerf.rendering, 'data_config': data_module.config, 'Rs_per_ds': data_module.Rs_per_ds,
                'seconds_per_dt': data_module.seconds_per_dt, 'ref_time': data_module.ref_time}, save_path)


class EmissionSuNeRFModule(BaseSuNeRFModule):
    """sunerf.py:77-149."""

    def __init__(self, Rs_per_ds, seconds_per_dt, image_scaling_config, lambda_image=1.0, lambda_regularization=1.0,
                 sampling_config=None, hierarchical_sampling_config=None, model_config=None, model=NeRF,
                 lambda_smoothness=0.0, lambda_temporal=0.0, lambda_ssim=0.0, ssim_window=7, **kwargs):
        self.lambda_image = lambda_image
        self.lambda_regularization = lambda_regularization
        self.lambda_smoothness = lambda_smoothness
        self.lambda_temporal = lambda_temporal
        self.lambda_ssim, self.ssim_window = lambda_ssim, ssim_window
        rendering = EmissionRadiativeTransfer(Rs_per_ds=Rs_per_ds, sampling_config=sampling_config,
                                              hierarchical_sampling_config=hierarchical_sampling_config,
                                              model_config=model_config, model=model)
        super().__init__(Rs_per_ds=Rs_per_ds, seconds_per_dt=seconds_per_dt, rendering=rendering, **kwargs)
        self.image_scaling = ImageAsinhScaling(**image_scaling_config)
        self.mse_loss = nn.MSELoss()

    def _ssim_scaling(self):
        """The structural term always sees the images under the module's asinh stretch, whose range is 1 -- under the MSE and
        under a likelihood alike."""
        return 1.0, (self._asinh_constants() if hasattr(self, 'image_scaling') else None)

    def _asinh_constants(self):
        """(vmax, a) of the image scaling as host floats, read from the module's buffers once (not per step: a device ->
        host copy each)."""
        key = (self.image_scaling.vmax.data_ptr(), self.image_scaling.vmax._version, self.image_scaling.a._version)
        if getattr(self, '_asinh_key', None) != key:
            self._asinh_key = key
            self._asinh = (float(self.image_scaling.vmax), float(self.image_scaling.a))
        return self._asinh

    def training_step(self, batch, batch_nb):
        tracing = batch['tracing']
        rays, time, target_image = tracing['rays'], tracing['time'], tracing['target_image']
        ssim_spec = self._ssim_spec(tracing)
        if 'patch' in tracing:          # windows of detector-pixel patches: the loss compares instrument(render) with the target
            rays = rays.reshape(-1, 2, 3)
            outputs = self.rendering(rays[:, 0].contiguous(), rays[:, 1].contiguous(), time)
            coarse, fine, target = _observed_windows(tracing, outputs)
            if self.likelihood is not None:
                return self._likelihood_step(coarse, fine, target, None, outputs, ssim_spec)
            loss, stats = training_loss(coarse, fine, target, outputs['regularization'], self.lambda_image,
                                        self.lambda_regularization, asinh_scaling=self._asinh_constants(),
                                        finite_check=_other_outputs(outputs))
            return self._finish_step(self._with_ssim(self._with_smoothness(loss), coarse, fine, target, ssim_spec), stats)
        rays_o, rays_d = rays[:, 0].contiguous(), rays[:, 1].contiguous()
        outputs = self.rendering(rays_o, rays_d, time)
        if self.likelihood is not None:
            return self._likelihood_step(outputs['coarse_image'], outputs['fine_image'], target_image.reshape(-1, 1), None, outputs)
        # sunerf.py:105-125 in one kernel: finite check of all outputs, asinh scaling, 2 x MSE, regularization mean, psnr
        loss, stats = training_loss(outputs['coarse_image'], outputs['fine_image'], target_image.reshape(-1, 1),
                                    outputs['regularization'], self.lambda_image, self.lambda_regularization,
                                    asinh_scaling=self._asinh_constants(),
                                    finite_check=_other_outputs(outputs))
        return self._finish_step(self._with_smoothness(loss), stats)

    def _validation_images(self, fine, target):
        """TestImageCallback's ImageNormalize(vmin=0, vmax=1, stretch=AsinhStretch(0.005), clip=True) (callback.py:35, 46-48;
        astropy mpl_normalize.py:157-173, stretch.py:31-44, 499-504) in fp64: asinh(clip(x, 0, 1) / a) / asinh(1 / a)."""
        a = 0.005

        def normalize(x):
            return torch.asinh(x.double().clamp(0., 1.) / a) / math.asinh(1. / a)
        return normalize(fine), normalize(target)

    def validation_step(self, batch, batch_nb, **kwargs):
        dataloader_idx = kwargs['dataloader_idx'] if 'dataloader_idx' in kwargs else 0
        if dataloader_idx == 0:
            rays, time, target_image = batch['rays'], batch['time'], batch['target_image']
            rays_o, rays_d = rays[:, 0].contiguous(), rays[:, 1].contiguous()
            with torch.no_grad():
                outputs = self.rendering(rays_o, rays_d, time)
            distance = rays_o.pow(2).sum(-1).pow(0.5)
            return {'target_image': target_image, 'fine_image': outputs['fine_image'],
                    'coarse_image': outputs['coarse_image'], 'height_map': outputs['height_map'],
                    'absorption_map': outputs['absorption_map'], 'z_vals_stratified': outputs['z_vals_stratified'],
                    'z_vals_hierarchical': outputs['z_vals_hierarchical'], 'distance': distance}


class DensityTemperatureSuNeRFModule(BaseSuNeRFModule):
    """sunerf.py:152-224."""

    def __init__(self, Rs_per_ds, seconds_per_dt, image_scaling_config, model, loss=nn.MSELoss(), lambda_image=1.0,
                 lambda_regularization=1.0, sampling_config=None, hierarchical_sampling_config=None,
                 pixel_intensity_factor=1e17, model_config=None, lambda_smoothness=0.0, lambda_temporal=0.0, lambda_ssim=0.0,
                 ssim_window=7, ssim_data_range=None, **kwargs):
        self.lambda_image = lambda_image
        self.lambda_regularization = lambda_regularization
        self.lambda_smoothness = lambda_smoothness
        self.lambda_temporal = lambda_temporal
        self.lambda_ssim, self.ssim_window, self.ssim_data_range = lambda_ssim, ssim_window, ssim_data_range
        rendering_kwargs = {k: kwargs.pop(k) for k in ('response_table', 'response_path', 'response_set') if k in kwargs}
        rendering = DensityTemperatureRadiativeTransfer(Rs_per_ds=Rs_per_ds, sampling_config=sampling_config,
                                                        hierarchical_sampling_config=hierarchical_sampling_config,
                                                        model_config=model_config, model=model,
                                                        pixel_intensity_factor=pixel_intensity_factor, **rendering_kwargs)
        super().__init__(Rs_per_ds=Rs_per_ds, seconds_per_dt=seconds_per_dt, rendering=rendering, **kwargs)
        self.loss = loss

    def training_step(self, batch, batch_nb):
        tracing = batch['tracing']
        rays, time, target_image, wavelengths = (tracing['rays'], tracing['time'], tracing['target_image'],
                                                 tracing['wavelength'])
        ssim_spec = self._ssim_spec(tracing)
        if 'patch' in tracing:          # windows of detector-pixel patches: the loss compares instrument(render) with the target
            rays = rays.reshape(-1, 2, 3)
            outputs = self.rendering.forward(rays[:, 0].contiguous(), rays[:, 1].contiguous(), time, wavelengths)
            coarse, fine, target_image = _observed_windows(tracing, outputs)
            outputs = {**outputs, 'coarse_image': coarse, 'fine_image': fine}
            codes = _patch_codes(tracing) if self.likelihood is not None else None
        else:
            rays_o, rays_d = rays[:, 0].contiguous(), rays[:, 1].contiguous()
            outputs = self.rendering.forward(rays_o, rays_d, time, wavelengths)
            codes = wavelengths
        if self.likelihood is not None:
            return self._likelihood_step(outputs['coarse_image'], outputs['fine_image'], target_image, codes, outputs, ssim_spec)
        if not isinstance(self.loss, nn.MSELoss) or self.loss.reduction != 'mean':
            if ssim_spec is not None:
                raise NotImplementedError('lambda_ssim > 0 is built for the MSE and the likelihood, not for a user-supplied loss module')
            return self._training_step_generic_loss(outputs, target_image)
        loss, stats = training_loss(outputs['coarse_image'], outputs['fine_image'], target_image,
                                    outputs['regularization'], self.lambda_image, self.lambda_regularization,
                                    asinh_scaling=None, finite_check=_other_outputs(outputs))
        loss = self._with_ssim(self._with_smoothness(loss), outputs['coarse_image'], outputs['fine_image'], target_image, ssim_spec)
        return self._finish_step(loss, stats)

    def _training_step_generic_loss(self, outputs, target_image):
        """A user-supplied loss module other than nn.MSELoss (sunerf.py:159 takes any callable): torch ops."""
        finite = torch.stack([torch.isfinite(v).all() for v in outputs.values()]).all()
        assert bool(finite), '! [Numerical Alert] an output contains NaN or Inf.'
        coarse_loss = self.loss(outputs['coarse_image'], target_image)
        fine_loss = self.loss(outputs['fine_image'], target_image)
        regularization_loss = outputs['regularization'].mean()
        loss = (self.lambda_image * (coarse_loss + fine_loss) + self.lambda_regularization * regularization_loss)
        with torch.no_grad():
            psnr = -10. * torch.log10(fine_loss)
        self.log('loss', loss)
        self.log('train', {'coarse': coarse_loss, 'fine': fine_loss, 'regularization': regularization_loss, 'psnr': psnr})
        return loss

    def validation_step(self, batch, batch_nb, **kwargs):
        dataloader_idx = kwargs['dataloader_idx'] if 'dataloader_idx' in kwargs else 0
        if dataloader_idx == 0:
            rays, time, target_image, wavelengths = batch['rays'], batch['time'], batch['target_image'], batch['wavelength']
            rays_o, rays_d = rays[:, 0].contiguous(), rays[:, 1].contiguous()
            with torch.no_grad():
                outputs = self.rendering(rays_o, rays_d, time, wavelengths)
            distance = rays_o.pow(2).sum(-1).pow(0.5)
            return {'target_image': target_image, 'fine_image': outputs['fine_image'],
                    'coarse_image': outputs['coarse_image'], 'height_map': outputs['height_map'],
                    'absorption_map': outputs['absorption_map'], 'z_vals_stratified': outputs['z_vals_stratified'],
                    'z_vals_hierarchical': outputs['z_vals_hierarchical'], 'distance': distance}


def fit_steps(module: BaseSuNeRFModule, batches, gradient_clip_val=0.5):
    """Minimal trainer loop with the semantics run_emission.py configures on the Lightning Trainer
    (run_emission.py:65-75): backward, clip_grad_norm_(0.5), Adam step, on_train_batch_end."""
    (optimizer,), _ = module.configure_optimizers()
    optimizer.max_norm = gradient_clip_val          # clip fused into the optimiser step (norm and coefficient stay on device)
    # Early all-reduce of the fine model's slice while the coarse backward still runs: one backward per model and step here, so
    # it is legal -- but it has only ever run with RCCL at world size 1 (no multi-GPU lease so far), so it stays opt-in
    # (SUNERF_OVERLAP=1) until a 2..8-GPU record exists; bench.py follows the same switch.
    optimizer.overlap = env_flag('SUNERF_OVERLAP')
    losses = []
    for i, batch in enumerate(batches):
        optimizer.zero_grad()
        loss = module.training_step(batch, i)
        loss.backward()
        stats = getattr(module, 'last_stats', None)
        optimizer.step(skip_if_positive=None if stats is None else stats[5:6])
        module.on_train_batch_end()     # (takes the all-rank finite check under data parallelism)
        losses.append(loss.detach())
    return losses
