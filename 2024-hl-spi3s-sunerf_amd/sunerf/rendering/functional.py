"""Glue between the module API and the HIP kernels: forward orchestration and the autograd boundary."""
import torch

from sunerf_hip import ops
from sunerf_hip.response import ResponseSet
from sunerf_hip.train import bucket_of


def _mlp_params(model):
    """``[W0, b0, W1, b1, ...]`` of a NeRF's ``nn.Linear`` layers: the order every MLP node takes its parameters in."""
    return [t for lin in model.linears() for t in (lin.weight, lin.bias)]


def _differentiable(params):
    return torch.is_grad_enabled() and any(p.requires_grad for p in params)


class _MlpOnPoints(torch.autograd.Function):
    """``NeRF.forward`` on free-standing query points (model.py:44-57) as an autograd node: the fused render kernel fed with the
    points themselves (32 per chunk, no ray, its integral unused), differentiable w.r.t. the model's parameters and the points.
    When the points need a gradient the backward is one fp32 call (:func:`_input_backward`) that also forms the parameter
    gradients, and the forward writes no activation stash."""

    @staticmethod
    def forward(ctx, model, points, *params):
        ctx.input_grad = ctx.needs_input_grad[1]
        training = any(ctx.needs_input_grad[2:]) and not ctx.input_grad
        packed = model.packed()
        out = ops.mlp_points_fwd(packed, points, training=training)
        if training:
            ctx.packed, ctx.params, ctx.n_padded = packed, params, out['n_padded']
            ctx.save_for_backward(out['stash'], points)
        elif ctx.input_grad:
            ctx.packed, ctx.params = packed, params
            ctx.save_for_backward(points)
        return out['raw'][:, :packed.d_out] if packed.d_out < 2 else out['raw']

    @staticmethod
    def backward(ctx, g_raw):
        if ctx.input_grad:
            points, = ctx.saved_tensors
            g_points, param_grads = _input_backward(ctx, g_raw, ('points', points))
            return (None, g_points[0]) + param_grads
        stash, points = ctx.saved_tensors
        if points.shape[0] != ctx.n_padded:      # the kernels work on whole 32-point chunks: zero points with zero gradient
            points = torch.cat([points, points.new_zeros(ctx.n_padded - points.shape[0], 4)])
        query = ('points', points)
        g = g_raw.new_zeros(ctx.n_padded, 2)
        g[:g_raw.shape[0], :g_raw.shape[1]] = g_raw
        g = g.view(ctx.n_padded // 32, 32, 2)
        absmax = g.abs().max().reshape(1).view(torch.int32)      # bit pattern of max |g_raw| (sunerf_common.h: gradient scale)
        return (None,) * 2 + _mlp_param_grads(ctx.params, lambda gW, gb, accumulate: ops.mlp_backward(
            ctx.packed, g, absmax, stash, gW, gb, accumulate=accumulate, query=query))


def _input_backward(ctx, g_raw, query, wanted=(True, True, True, True)):
    """The backward of an MLP node whose query (points, or rays / times / z) needs a gradient: ONE call of the fp32 input-gradient
    kernel (:func:`sunerf_hip.ops.mlp_input_backward`), with the parameter gradients in it when a parameter needs them.  Returns
    ``(input gradients as a tuple, parameter gradients as _mlp_param_grads returns them)``.  Second derivatives are not built: under
    ``create_graph=True`` this raises instead of returning gradients without a graph."""
    if torch.is_grad_enabled():
        raise RuntimeError('second derivatives of a NeRF w.r.t. its query points / rays are not implemented (the fp32 input-gradient '
                           'backward is once-differentiable): call backward / autograd.grad without create_graph=True')
    g_raw = g_raw.contiguous().float()
    n_params = len(ctx.params)
    if not any(ctx.needs_input_grad[-n_params:]):
        g_in = ops.mlp_input_backward(ctx.packed, g_raw, query, wanted=wanted)
        return (g_in if isinstance(g_in, tuple) else (g_in,)), (None,) * n_params
    got = []
    param_grads = _mlp_param_grads(ctx.params, lambda gW, gb, accumulate: got.append(ops.mlp_input_backward(
        ctx.packed, g_raw, query, gW, gb, accumulate=accumulate, wanted=wanted)))
    return (got[0] if isinstance(got[0], tuple) else (got[0],)), param_grads


def mlp_points(model, x: torch.Tensor) -> torch.Tensor:
    """NeRF.forward on arbitrary query points (M, 4) -> (M, d_out) (model.py:44-57): the fused kernel's free-standing-points
    mode (``sunerf_mlp_points_fwd``), every lane of it a query point.  Differentiable w.r.t. the model's parameters and the
    points like the reference's module call (a loss on free-standing points trains; ``torch.autograd.grad(out, x)`` works)."""
    flat = x.reshape(-1, 4)
    params = _mlp_params(model)
    if _differentiable(params + [flat]):
        return _MlpOnPoints.apply(model, flat, *params)
    packed = model.packed()
    raw = ops.mlp_points_fwd(packed, flat)['raw']
    return raw[:, :packed.d_out] if packed.d_out < 2 else raw


def _mlp_param_grads(params, launch):
    """Autograd's gradients for the MLP parameters ``params`` (W0, b0, W1, b1, ...) of a node.  ``launch(grad_weights,
    grad_biases, accumulate)`` runs the weight-gradient kernels (``ops.mlp_backward`` / ``ops.emission_render_bwd``).

    When every parameter already owns a contiguous fp32 ``.grad`` on its device (``ClipAdam`` / ``GradBucket`` keep them as
    views of one flat buffer), the kernels add their result straight into it and the node reports "no gradient" for the
    parameters -- instead of returning 18 fresh tensors per model that autograd would then add to ``.grad`` with 18 tiny
    kernels (a third of the step at the reference's default batch of 1024 rays).  Else fresh fp32 tensors are returned."""
    grads = [p.grad for p in params]
    if all(g is not None and g.dtype == torch.float32 and g.device == p.device and g.is_contiguous() and g.shape == p.shape
           for p, g in zip(params, grads)):
        launch(grads[0::2], grads[1::2], True)
        _announce(params)
        return (None,) * len(params)
    grads = [torch.empty(p.shape, dtype=torch.float32, device=p.device) for p in params]
    launch(grads[0::2], grads[1::2], False)
    return tuple(grads)


def _scalar_head_slice(scalars):
    """The slice of a flat gradient bucket that the given 0-d parameters occupy back to back (``ClipAdam`` tags every parameter with
    ``(owner, offset, numel)``), or None: lets eight scalar gradients be accumulated with one launch instead of eight."""
    tags = [bucket_of(p) for p in scalars]
    if any(t is None for t in tags):
        return None
    owner, first = tags[0][0], tags[0][1]
    for i, (p, (o, off, k)) in enumerate(zip(scalars, tags)):
        if o is not owner or off != first + i or k != 1:
            return None
        # the parameter's .grad must still BE its slot of the bucket: a replaced / cleared .grad is copied over (or zeroed
        # into) the slot by the optimiser's step, which would lose what is added here
        if not p.requires_grad or p.grad is None or p.grad.data_ptr() != owner.flat_grads[off:off + 1].data_ptr():
            return None
    return owner.flat_grads[first:first + len(tags)]


def _scalar_head_grads(needs_vc, needs_la, vol_c_param, la_params, g_vc, g_la):
    """Autograd's share of the DT integral's scalar-head gradients (``g_vc`` (1,), ``g_la`` (7,)) for the DT passes
    (``_DtPass``, ``_FieldDtPass``): added straight into the parameters' slots of a flat gradient bucket when they have them
    (autograd then gets None), else returned per parameter.  Returns ``(g_vol_c, (g_la per channel))``."""
    n_la = len(la_params)
    la_slot = _scalar_head_slice(la_params) if all(needs_la) else None
    vc_slot = _scalar_head_slice([vol_c_param]) if needs_vc else None
    if la_slot is not None:
        la_slot.add_(g_la)
        g_la_out = (None,) * n_la
    else:
        g_la_out = tuple(g_la[i] if needs_la[i] else None for i in range(n_la))
    if vc_slot is not None:
        vc_slot.add_(g_vc)
        g_vc_out = None
    else:
        g_vc_out = g_vc.reshape(()) if needs_vc else None
    return g_vc_out, g_la_out


def _announce(params):
    """The gradients of ``params`` are final in their flat bucket: let its owner start the all-reduce of that slice while the
    other model's backward still runs (``ClipAdam(overlap=True)``)."""
    owner = bucket_of(params[0])
    if owner is not None:
        owner[0].segment_ready(params)


_EPILOGUES = ('height_map', 'absorption_map', 'regularization')


def _pass_outputs(ctx, out, third, want_epilogues):
    """The outputs of a fused emission / DT pass node: ``(image, weights, out[third][, height_map, absorption_map,
    regularization])``, all but ``image`` and ``regularization`` marked non-differentiable."""
    outs = tuple(out[k] for k in ('image', 'weights', third) + (_EPILOGUES if want_epilogues else ()))
    ctx.mark_non_differentiable(*outs[1:5])
    return outs


def _pass_dict(outs, third):
    """:func:`_pass_outputs`' tuple as the pass's dict, its third output named ``third``."""
    return dict(zip(('image', 'weights', third) + _EPILOGUES, outs))


class _EmissionPass(torch.autograd.Function):
    """One fused render pass (coarse or fine) as an autograd node.

    Differentiable outputs: ``image`` and ``regularization`` (the two the training loss of sunerf.py:110-120 uses);
    gradients are produced for the MLP parameters only -- the reference's graph has no path to the rays
    (sampling.py:120 detaches the resampled z).  ``weights`` / ``absorption`` / maps are marked non-differentiable."""

    @staticmethod
    def forward(ctx, model, rays_o, rays_d, times, z_vals, reg_radius, want_epilogues, *params):
        training = any(ctx.needs_input_grad[7:])
        ctx.set_materialize_grads(False)      # unused / non-differentiable outputs: None instead of (N,S) zero tensors
        packed = model.packed()
        out = ops.emission_render_fwd(packed, rays_o, rays_d, times, z_vals, reg_radius,
                                      want_epilogues=want_epilogues, training=training)
        if training:
            ctx.packed, ctx.reg_radius, ctx.params = packed, reg_radius, params
            ctx.save_for_backward(rays_o, rays_d, z_vals, out['raw'], out['stash'], times)
        return _pass_outputs(ctx, out, 'absorption', want_epilogues)

    @staticmethod
    def backward(ctx, g_image, g_weights, g_absorption, g_hm=None, g_am=None, g_reg=None):
        rays_o, rays_d, z_vals, raw, stash, times = ctx.saved_tensors
        n, s = z_vals.shape
        if g_image is None and g_reg is None:
            return (None,) * (7 + len(ctx.params))
        if g_image is None:
            g_image = torch.zeros(n, dtype=torch.float32, device=z_vals.device)
        return (None,) * 7 + _mlp_param_grads(ctx.params, lambda gW, gb, accumulate: ops.emission_render_bwd(
            ctx.packed, rays_o, rays_d, z_vals, raw, stash, g_image, g_reg, 0.0, ctx.reg_radius, gW, gb,
            accumulate=accumulate, times=times))


def _field_emission_pass(model, rays_o, rays_d, times, z_vals, reg_radius, want_epilogues, want_raw=False):
    """:func:`emission_pass` for a field module with ``field_on_rays`` (``GridField``: no MLP): the field through its own node,
    the integral of emission.py:14-54 on its ``raw`` (``_EmissionIntegral``) and the three epilogues in torch, as
    ``SuNeRFRendering.forward`` forms them (base_tracing.py:99-110).  The fused pass' keys; ``image`` and ``regularization``
    carry the gradient to whatever parameters ``field_on_rays`` is differentiable in, the rest is detached like the fused
    pass' non-differentiable outputs."""
    raw = _field_raw(model, rays_o, rays_d, z_vals, times)
    if raw.shape[-1] != 2:
        raise ValueError(f'an emission field answers (ln emission, absorption logit) per sample, got {raw.shape[-1]} channels')
    image, weights, absorption = _EmissionIntegral.apply(raw, z_vals, rays_d)
    out = {'image': image, 'weights': weights.detach(), 'absorption': absorption.detach()}
    if want_raw:
        out['raw'] = raw.detach()
    if want_epilogues:
        points = rays_o[:, None, :] + rays_d[:, None, :] * z_vals[..., None]
        distance = points.pow(2).sum(-1).pow(0.5)
        out['height_map'] = (out['weights'] * distance).sum(-1)
        out['absorption_map'] = (1 - out['absorption']).sum(-1)
        out['regularization'] = torch.relu(distance - reg_radius) * (1 - absorption)
    return out


def emission_pass(model, rays_o, rays_d, times, z_vals, reg_radius, want_epilogues):
    """Dict of one pass' outputs; goes through autograd when gradients are enabled and the model is trainable."""
    if hasattr(model, 'field_on_rays'):
        return _field_emission_pass(model, rays_o, rays_d, times, z_vals, reg_radius, want_epilogues)
    params = _mlp_params(model)
    if _differentiable(params):
        outs = _EmissionPass.apply(model, rays_o, rays_d, times, z_vals, reg_radius, want_epilogues, *params)
        return _pass_dict(outs, 'absorption')
    return ops.emission_render_fwd(model.packed(), rays_o, rays_d, times, z_vals, reg_radius,
                                   want_epilogues=want_epilogues)


class _MlpOnRays(torch.autograd.Function):
    """``NeRF.forward`` (model.py:44-57) on the samples ``o + d z`` of a ray batch as an autograd node: the raw network output
    (N, S, d_output), differentiable w.r.t. the model's parameters and w.r.t. ``rays_o``, ``rays_d``, ``times`` and ``z_vals``.
    This is what the generic ``SuNeRFRendering._render`` (base_tracing.py:118-129) hands to a subclass's ``raw2outputs``: the
    MLP runs in the fused render kernel (whose own integral outputs are ignored) and its backward in the data / weight gradient
    kernels, fed with whatever gradient the subclass's torch code sends back -- or, when an input needs a gradient, in one call
    of the fp32 input-gradient kernel (:func:`_input_backward`; the forward then writes no activation stash)."""

    @staticmethod
    def forward(ctx, model, rays_o, rays_d, times, z_vals, *params):
        ctx.input_grad = any(ctx.needs_input_grad[1:5])
        training = any(ctx.needs_input_grad[5:]) and not ctx.input_grad
        packed = model.packed()
        out = ops.emission_render_fwd(packed, rays_o, rays_d, times, z_vals, 0.0, want_raw=True, training=training)
        if training:
            ctx.packed, ctx.params = packed, params
            ctx.save_for_backward(out['stash'], rays_o, rays_d, times, z_vals)
        elif ctx.input_grad:
            ctx.packed, ctx.params = packed, params
            ctx.save_for_backward(rays_o, rays_d, times, z_vals)
        return out['raw'][..., :packed.d_out] if packed.d_out < 2 else out['raw']

    @staticmethod
    def backward(ctx, g_raw):
        if ctx.input_grad:
            rays_o, rays_d, times, z_vals = ctx.saved_tensors
            wanted = tuple(ctx.needs_input_grad[1:5])
            (g_o, g_d, g_t, g_z), param_grads = _input_backward(ctx, g_raw, ('rays', rays_o, rays_d, times, z_vals), wanted)
            if g_t is not None:
                g_t = g_t.reshape(times.shape)
            return (None, g_o, g_d, g_t, g_z) + param_grads
        stash, rays_o, rays_d, times, z_vals = ctx.saved_tensors
        query = ('rays', rays_o, rays_d, times, z_vals)
        if g_raw.shape[-1] < 2:
            g_raw = torch.cat([g_raw, torch.zeros_like(g_raw)], -1)
        g_raw = g_raw.contiguous().float()
        # bit pattern of max |g_raw|: the scale the fp16 backward arithmetic is normalised with (sunerf_common.h)
        absmax = g_raw.abs().max().reshape(1).view(torch.int32)
        return (None,) * 5 + _mlp_param_grads(ctx.params, lambda gW, gb, accumulate: ops.mlp_backward(
            ctx.packed, g_raw, absmax, stash, gW, gb, accumulate=accumulate, query=query))


def mlp_on_rays(model, rays_o, rays_d, times, z_vals) -> torch.Tensor:
    """(N, S, d_output) raw output of ``model`` (a ``NeRF``) at the samples of the rays; goes through autograd when gradients are
    enabled and the model is trainable or a ray tensor (``rays_o``, ``rays_d``, ``times``, ``z_vals``) requires grad."""
    params = _mlp_params(model)
    if _differentiable(params + [rays_o, rays_d, times, z_vals]):
        return _MlpOnRays.apply(model, rays_o, rays_d, times, z_vals, *params)
    raw = ops.emission_render_fwd(model.packed(), rays_o, rays_d, times, z_vals, 0.0, want_raw=True)['raw']
    return raw[..., :model.packed().d_out] if model.packed().d_out < 2 else raw


class _EmissionIntegral(torch.autograd.Function):
    """``EmissionRadiativeTransfer.raw2outputs`` (emission.py:14-54) on a given raw tensor: differentiable w.r.t. ``raw`` through
    all three outputs (image, weights, regularizing_quantity), like the reference's autograd graph."""

    @staticmethod
    def forward(ctx, raw, z_vals, rays_d):
        image, weights, absorption = ops.emission_integral_fwd(raw.detach(), z_vals, rays_d)
        ctx.save_for_backward(raw.detach(), z_vals, rays_d)
        ctx.set_materialize_grads(False)
        return image, weights, absorption

    @staticmethod
    def backward(ctx, g_image, g_weights, g_absorption):
        raw, z_vals, rays_d = ctx.saved_tensors
        if g_image is None and g_weights is None and g_absorption is None:
            return None, None, None
        return ops.emission_integral_bwd(raw, z_vals, rays_d, g_image, g_weights, g_absorption), None, None


def emission_raw2outputs(raw, z_vals, rays_d):
    image, weights, absorption = _EmissionIntegral.apply(raw, z_vals, rays_d)
    return {'image': image, 'weights': weights, 'regularizing_quantity': absorption}


def _absorption_scalars(log_abs, tables):
    """The ``log_absortpion`` scalars the integral takes, in its channel order.  ``tables`` is the AIA pair ``(logte [7,101],
    response [7,101])`` -- the seven AIA names, the kernels of sunerf_hip.h -- or a ``ResponseSet``: one scalar per channel of the
    set, by its code, for the kernels of sunerf_hip_response.h."""
    if isinstance(tables, ResponseSet):
        missing = [k for k in tables.keys if k not in log_abs]
        if missing:
            raise ValueError(f'the model has no log_absortpion scalar for the response set\'s channels {", ".join(missing)} '
                           f'(it has {", ".join(log_abs.keys())}): build it with channels=<the set or its codes>')
        return [log_abs[k] for k in tables.keys]
    return [log_abs[str(w)] for w in ops.AIA_WAVELENGTHS]


class _DtIntegral(torch.autograd.Function):
    """``DensityTemperatureRadiativeTransfer.raw2outputs`` (density_temperature.py:192-271) on given inferences (base offsets
    already added, as ``NeRF_DT.forward`` returns them).  Differentiable through all three outputs -- ``image``, ``weights``
    and ``regularizing_quantity`` -- w.r.t. the inferences, and through ``image`` w.r.t. the seven absorption scalars and the
    volumetric constant, like the reference's graph (a subclass's loss reaches ``weights`` through ``height_map`` and
    ``regularizing_quantity`` through its ``regularization``, base_tracing.py:99-110)."""

    @staticmethod
    def forward(ctx, tables, pixel_factor, inferences, z_vals, rays_d, wavelengths, vol_c, *la):
        la_vec = torch.stack([p.detach() for p in la])
        zeros = torch.zeros_like(rays_d)
        if isinstance(tables, ResponseSet):
            out = ops.dt_response_fwd(inferences.detach(), z_vals, zeros, rays_d, wavelengths, tables, la_vec, vol_c, 0.0, 0.0,
                                      pixel_factor, 0.0)
        else:
            out = ops.dt_integral_fwd(inferences.detach(), z_vals, zeros, rays_d, wavelengths, tables[0], tables[1], la_vec, vol_c,
                                      0.0, 0.0, pixel_factor, 0.0)
        ctx.tables, ctx.pixel_factor = tables, pixel_factor
        ctx.save_for_backward(inferences.detach(), z_vals, rays_d, wavelengths, la_vec, vol_c.detach())
        ctx.set_materialize_grads(False)
        return out['image'], out['weights'], out['reg_q']

    @staticmethod
    def backward(ctx, g_image, g_weights, g_q):
        inferences, z_vals, rays_d, wavelengths, la_vec, vol_c = ctx.saved_tensors
        if g_image is None and g_weights is None and g_q is None:
            return (None,) * (7 + la_vec.shape[0])
        if g_image is None:
            g_image = torch.zeros(z_vals.shape[0], wavelengths.shape[1], dtype=torch.float32, device=z_vals.device)
        entry, tables = ((ops.dt_response_bwd_full, (ctx.tables,)) if isinstance(ctx.tables, ResponseSet) else
                         (ops.dt_integral_bwd_full, (ctx.tables[0], ctx.tables[1])))
        g_raw, g_la, g_vc, _ = entry(inferences, z_vals, torch.zeros_like(rays_d), rays_d, wavelengths, *tables, la_vec, vol_c,
                                     0.0, 0.0, ctx.pixel_factor, 0.0, g_image.contiguous(), None,
                                     None if g_weights is None else g_weights.contiguous(),
                                     None if g_q is None else g_q.contiguous())
        return (None, None, g_raw, None, None, None, g_vc.reshape(())) + tuple(g_la[i] for i in range(g_la.shape[0]))


def dt_raw2outputs(tables, pixel_factor, inferences, log_abs, vol_c, z_vals, rays_d, wavelengths):
    la = _absorption_scalars(log_abs, tables)
    if not torch.is_grad_enabled() or not any(t.requires_grad for t in [inferences, vol_c] + la):
        la_vec = torch.stack([p.detach() for p in la])
        if isinstance(tables, ResponseSet):
            out = ops.dt_response_fwd(inferences.detach(), z_vals, torch.zeros_like(rays_d), rays_d, wavelengths, tables, la_vec,
                                      vol_c, 0.0, 0.0, pixel_factor, 0.0)
        else:
            out = ops.dt_integral_fwd(inferences.detach(), z_vals, torch.zeros_like(rays_d), rays_d, wavelengths, tables[0],
                                      tables[1], la_vec, vol_c, 0.0, 0.0, pixel_factor, 0.0)
        return {'image': out['image'], 'weights': out['weights'], 'regularizing_quantity': out['reg_q']}
    image, weights, reg_q = _DtIntegral.apply(tables, pixel_factor, inferences, z_vals, rays_d, wavelengths, vol_c, *la)
    return {'image': image, 'weights': weights, 'regularizing_quantity': reg_q}


def _dt_forward(model, tables, pixel_factor, raw, rays_o, rays_d, z_vals, wavelengths, reg_radius, want_epilogues, la, vol_c):
    """The DT integral of ``raw`` (N, S, 2), ``model``'s raw output or field, with its base offsets: the forward of every DT
    pass, with or without autograd.  ``la``: the stacked absorption scalars, (7,) or one per channel of a ``ResponseSet``."""
    if isinstance(tables, ResponseSet):
        return ops.dt_response_fwd(raw, z_vals, rays_o, rays_d, wavelengths, tables, la, vol_c, model.base_log_density,
                                   model.base_log_temperature, pixel_factor, reg_radius, want_epilogues=want_epilogues)
    return ops.dt_integral_fwd(raw, z_vals, rays_o, rays_d, wavelengths, tables[0], tables[1], la, vol_c,
                               model.base_log_density, model.base_log_temperature, pixel_factor, reg_radius,
                               want_epilogues=want_epilogues)


def _dt_backward(ctx, saved, g_image, g_reg):
    """``ops.dt_integral_bwd`` of a DT pass node whose forward set ``ctx.dt = (tables, pixel_factor, reg_radius,
    base_log_density, base_log_temperature)`` and saved ``saved = (rays_o, rays_d, z_vals, wavelengths, raw, la, vol_c)``
    -> (g_raw, g_la, g_vc, absmax)."""
    rays_o, rays_d, z_vals, wavelengths, raw, la, vol_c = saved
    tables, pixel_factor, reg_radius, base_d, base_t = ctx.dt
    if g_image is None:
        g_image = torch.zeros(z_vals.shape[0], wavelengths.shape[1], dtype=torch.float32, device=z_vals.device)
    if isinstance(tables, ResponseSet):
        return ops.dt_response_bwd(raw, z_vals, rays_o, rays_d, wavelengths, tables, la, vol_c, base_d, base_t, pixel_factor,
                                   reg_radius, g_image.contiguous(), g_reg)
    return ops.dt_integral_bwd(raw, z_vals, rays_o, rays_d, wavelengths, tables[0], tables[1], la, vol_c, base_d, base_t,
                               pixel_factor, reg_radius, g_image.contiguous(), g_reg)


class _DtPass(torch.autograd.Function):
    """One fused density/temperature pass: render kernel (MLP) -> DT integral kernel.  Differentiable outputs: ``image``
    (N,W) and ``regularization``; gradients for the MLP parameters, the 7 ``log_absortpion`` scalars and
    ``volumetric_constant``."""

    @staticmethod
    def forward(ctx, model, tables, pixel_factor, rays_o, rays_d, times, z_vals, wavelengths, reg_radius, want_epilogues,
                vol_c, *params):
        n_la = len(tables) if isinstance(tables, ResponseSet) else len(ops.AIA_WAVELENGTHS)
        la = torch.stack([p.detach() for p in params[:n_la]])
        training = any(ctx.needs_input_grad[10:])
        ctx.set_materialize_grads(False)
        packed = model.packed()
        # (the DT image goes with rho^2 = exp(2 raw_0): twice the emission image's sensitivity to the raw output)
        mlp = ops.emission_render_fwd(packed, rays_o, rays_d, times, z_vals, 0.0, want_raw=True, training=training,
                                      probe_sensitivity=2.0)
        out = _dt_forward(model, tables, pixel_factor, mlp['raw'], rays_o, rays_d, z_vals, wavelengths, reg_radius,
                          want_epilogues, la, vol_c)
        if training:
            ctx.packed, ctx.la_params, ctx.vol_c_param, ctx.mlp_params = packed, params[:n_la], vol_c, params[n_la:]
            ctx.dt = (tables, pixel_factor, reg_radius, model.base_log_density, model.base_log_temperature)
            ctx.save_for_backward(rays_o, rays_d, z_vals, wavelengths, mlp['raw'], la, vol_c.detach(), mlp['stash'], times)
        return _pass_outputs(ctx, out, 'reg_q', want_epilogues)

    @staticmethod
    def backward(ctx, g_image, g_weights, g_q, g_hm=None, g_am=None, g_reg=None):
        *saved, stash, times = ctx.saved_tensors
        rays_o, rays_d, z_vals = saved[:3]
        query = ('rays', rays_o, rays_d, times, z_vals)
        g_raw, g_la, g_vc, absmax = _dt_backward(ctx, saved, g_image, g_reg)
        n_la = len(ctx.la_params)
        g_vc_out, g_la_out = _scalar_head_grads(ctx.needs_input_grad[10], ctx.needs_input_grad[11:11 + n_la], ctx.vol_c_param,
                                                ctx.la_params, g_vc, g_la)
        g_mlp = _mlp_param_grads(ctx.mlp_params, lambda gW, gb, accumulate: ops.mlp_backward(
            ctx.packed, g_raw, absmax, stash, gW, gb, accumulate=accumulate, query=query))
        return (None,) * 10 + (g_vc_out,) + g_la_out + g_mlp


def _field_raw(model, rays_o, rays_d, z_vals, times):
    """``model.field_on_rays`` at the samples of the rays; a time-dependent field (``MHDModel``) is handed the rays' times."""
    if getattr(model, 'time_dependent', False):
        return model.field_on_rays(rays_o, rays_d, z_vals, times)
    return model.field_on_rays(rays_o, rays_d, z_vals)


def dt_pass(model, tables, pixel_factor, rays_o, rays_d, times, z_vals, wavelengths, reg_radius, want_epilogues):
    """Dict of one DT pass' outputs (image (N,W), weights, regularizing_quantity[, maps, regularization])."""
    la = _absorption_scalars(model.log_absortpion, tables)
    if hasattr(model, 'field_on_rays'):
        # analytic field (SimpleStar) or simulation cube (MHDModel) instead of an MLP: same integral (stellar_model.py,
        # mhd_model.py, image_render.py:244-269)
        sp = star_parameters(model) if hasattr(model, 'stellar_parameters') else []
        fp = list(model.field_parameters()) if hasattr(model, 'field_parameters') else []     # a GridFieldDT's values
        if _differentiable(la + sp + fp + [model.volumetric_constant]):
            # a star's field through its own node, on the device-side parameters even when they are frozen
            raw = star_field(model, rays_o, rays_d, z_vals) if sp else _field_raw(model, rays_o, rays_d, z_vals, times)
            outs = _FieldDtPass.apply(model, tables, pixel_factor, raw, rays_o, rays_d, z_vals, wavelengths, reg_radius,
                                      want_epilogues, model.volumetric_constant, *la)
            return _pass_dict(outs, 'regularizing_quantity')
        with torch.no_grad():
            raw = _field_raw(model, rays_o, rays_d, z_vals, times)
            out = _dt_forward(model, tables, pixel_factor, raw, rays_o, rays_d, z_vals, wavelengths, reg_radius,
                              want_epilogues, torch.stack([p.detach() for p in la]), model.volumetric_constant)
        out['regularizing_quantity'] = out.pop('reg_q')
        return out
    outs = _DtPass.apply(model, tables, pixel_factor, rays_o, rays_d, times, z_vals, wavelengths, reg_radius, want_epilogues,
                         model.volumetric_constant, *la, *_mlp_params(model))
    return _pass_dict(outs, 'regularizing_quantity')


# ---- trainable SimpleStar (stellar_model.py:5-102) ------------------------------------------------------------------------
STAR_KEYS = ('Rs', 'h0', 'T0', 'rho_0')     # the order of the reference's ``stellar_parameters`` and of the C ABI's params[4]


def star_parameters(star):
    """The four stellar parameters of a ``SimpleStar``, in ``STAR_KEYS`` order."""
    return [star.stellar_parameters[k] for k in STAR_KEYS]


def _star_param_array(sp):
    """(4,) device array of the stellar parameters for the kernels: the slice of the optimiser's flat parameter buffer the four
    occupy back to back (``ClipAdam``; no copy, and what its step kernel writes is what the next render reads), else a stack."""
    tags = [bucket_of(p) for p in sp]
    if all(t is not None for t in tags):
        owner, first = tags[0][0], tags[0][1]
        flat = owner.flat_params[first:first + len(sp)]
        if all(o is owner and off == first + i and k == 1 and p.data_ptr() == flat[i:i + 1].data_ptr()
               for i, (p, (o, off, k)) in enumerate(zip(sp, tags))):
            return flat
    return torch.stack([p.detach() for p in sp])


class _StarField(torch.autograd.Function):
    """``SimpleStar.forward`` at the samples ``o + d z`` (stellar_model.py:53-102): raw (N, S, 2) = (ln rho, log10 T),
    differentiable w.r.t. the four stellar parameters (not w.r.t. the rays or z).  Their gradients are accumulated by the
    kernel straight into their slots of a flat gradient bucket when they have them (then autograd gets None), else returned
    per parameter."""

    @staticmethod
    def forward(ctx, t_photosphere, rays_o, rays_d, z_vals, *sp):
        params = _star_param_array(sp)
        raw = ops.simple_star_field_dev(rays_o, rays_d, z_vals, params, t_photosphere)
        ctx.t_photosphere, ctx.sp = t_photosphere, sp
        ctx.save_for_backward(rays_o, rays_d, z_vals, params)
        ctx.set_materialize_grads(False)
        return raw

    @staticmethod
    def backward(ctx, g_raw):
        needs = ctx.needs_input_grad[4:]
        if g_raw is None or not any(needs):       # (None: a DT pass without an image / regularization gradient)
            return (None,) * 8
        rays_o, rays_d, z_vals, params = ctx.saved_tensors
        g_raw = g_raw.contiguous().float()
        slot = _scalar_head_slice(ctx.sp)
        if slot is not None:
            ops.simple_star_bwd(rays_o, rays_d, z_vals, params, ctx.t_photosphere, g_raw, out=slot)
            return (None,) * 8
        g = ops.simple_star_bwd(rays_o, rays_d, z_vals, params, ctx.t_photosphere, g_raw)
        return (None,) * 4 + tuple(g[i] if needs[i] else None for i in range(4))


def star_field(star, rays_o, rays_d, z_vals):
    """(N, S, 2) field of ``star`` (a ``SimpleStar``) at the samples of the rays through autograd."""
    return _StarField.apply(star.t_photosphere, rays_o, rays_d, z_vals, *star_parameters(star))


class _FieldDtPass(torch.autograd.Function):
    """The DT integral of a field module's ``raw`` (``SimpleStar``, ``MHDModel``: no MLP) as the node of a pass.
    Differentiable outputs: ``image`` (N,W) and ``regularization``; gradients for ``raw`` (a ``SimpleStar``'s comes from
    :func:`star_field`, whose node turns it into the stellar parameters' gradients), the 7 ``log_absortpion`` scalars and
    ``volumetric_constant`` (added straight into an optimiser's flat bucket when they have slots there).  No gradient w.r.t.
    the rays or z (the resampled z is detached in the reference, sampling.py:120)."""

    @staticmethod
    def forward(ctx, field, tables, pixel_factor, raw, rays_o, rays_d, z_vals, wavelengths, reg_radius, want_epilogues, vol_c,
                *la_params):
        la = torch.stack([p.detach() for p in la_params])
        ctx.set_materialize_grads(False)
        out = _dt_forward(field, tables, pixel_factor, raw, rays_o, rays_d, z_vals, wavelengths, reg_radius,
                          want_epilogues, la, vol_c)
        ctx.la_params, ctx.vol_c_param = la_params, vol_c
        ctx.dt = (tables, pixel_factor, reg_radius, field.base_log_density, field.base_log_temperature)
        ctx.save_for_backward(rays_o, rays_d, z_vals, wavelengths, raw, la, vol_c.detach())
        return _pass_outputs(ctx, out, 'reg_q', want_epilogues)

    @staticmethod
    def backward(ctx, g_image, g_weights, g_q, g_hm=None, g_am=None, g_reg=None):
        n_la = len(ctx.la_params)
        if g_image is None and g_reg is None:
            return (None,) * (11 + n_la)
        g_raw, g_la, g_vc, _ = _dt_backward(ctx, ctx.saved_tensors, g_image, g_reg)
        g_vc_out, g_la_out = _scalar_head_grads(ctx.needs_input_grad[10], ctx.needs_input_grad[11:11 + n_la], ctx.vol_c_param,
                                                ctx.la_params, g_vc, g_la)
        return (None,) * 3 + (g_raw if ctx.needs_input_grad[3] else None,) + (None,) * 6 + (g_vc_out,) + g_la_out



# ---- white-light Thomson scattering (thompson.py:17-109) -----------------------------------------------------------------
LN10 = 2.302585092994046        # a NeRF's channel 0 is log10 rho (thompson.py:39: rho = 10 ** raw[..., 0])
THOMSON_KEYS = ('pixel_B', 'pixel_density', 'distance_from_sun', 'distance_from_obs', 'weights')


def _thomson_dict(outs):
    out = dict(zip(THOMSON_KEYS, outs))
    out['image'] = out['pixel_B']
    out['regularizing_quantity'] = torch.ones_like(out['weights'])     # optically thin: no absorption, no regularization
    return out


class _ThomsonIntegral(torch.autograd.Function):
    """``ThompsonScattering.raw2outputs`` (thompson.py:17-109, defects resolved) on a given raw tensor (N, S, C): differentiable
    w.r.t. ``raw`` through all five outputs (sunerf_thomson_integral_fwd / _bwd)."""

    @staticmethod
    def forward(ctx, raw, z_vals, rays_o, rays_d, constants, kappa):
        out = ops.thomson_integral_fwd(raw.detach(), z_vals, rays_o, rays_d, constants, kappa)
        ctx.constants, ctx.kappa = constants, kappa
        ctx.save_for_backward(raw.detach(), z_vals, rays_o, rays_d)
        ctx.set_materialize_grads(False)
        return tuple(out[k] for k in THOMSON_KEYS)

    @staticmethod
    def backward(ctx, g_b, g_den, g_sun, g_obs, g_w):
        raw, z_vals, rays_o, rays_d = ctx.saved_tensors
        if all(g is None for g in (g_b, g_den, g_sun, g_obs, g_w)):
            return (None,) * 6
        g_raw, _ = ops.thomson_integral_bwd(raw, z_vals, rays_o, rays_d, ctx.constants, ctx.kappa, g_b, g_den, g_sun, g_obs, g_w)
        return (g_raw,) + (None,) * 5


def thomson_raw2outputs(raw, z_vals, rays_o, rays_d, constants, kappa):
    """``{pixel_B (N,2), pixel_density, distance_from_sun, distance_from_obs (N,), weights (N,S), image (= pixel_B),
    regularizing_quantity (ones)}`` for the log density ``raw[..., 0]``, rho = exp(kappa raw0).  ``constants``: the module's
    (solar_radius, limb_darkening_coeff, C_0) buffers.  Through autograd when ``raw`` requires a gradient."""
    constants = tuple(constants)
    if torch.is_grad_enabled() and raw.requires_grad:
        return _thomson_dict(_ThomsonIntegral.apply(raw, z_vals, rays_o, rays_d, constants, kappa))
    out = ops.thomson_integral_fwd(raw.detach(), z_vals, rays_o, rays_d, constants, kappa)
    return _thomson_dict([out[k] for k in THOMSON_KEYS])


class _ThomsonPass(torch.autograd.Function):
    """One fused white-light pass of a NeRF: render kernel (MLP) -> Thomson integral kernel.  Differentiable outputs:
    ``pixel_B``, ``pixel_density`` and the two distances; gradients for the MLP parameters (``weights`` is marked
    non-differentiable, as in the fused emission / DT passes)."""

    @staticmethod
    def forward(ctx, model, constants, rays_o, rays_d, times, z_vals, *params):
        training = any(ctx.needs_input_grad[6:])
        ctx.set_materialize_grads(False)
        packed = model.packed()
        # (the image goes with rho = 10^raw_0: ln 10 times the emission image's sensitivity to the raw output)
        mlp = ops.emission_render_fwd(packed, rays_o, rays_d, times, z_vals, 0.0, want_raw=True, training=training,
                                      probe_sensitivity=LN10)
        out = ops.thomson_integral_fwd(mlp['raw'], z_vals, rays_o, rays_d, constants, LN10)
        if training:
            ctx.packed, ctx.constants, ctx.params = packed, constants, params
            ctx.save_for_backward(rays_o, rays_d, z_vals, mlp['raw'], mlp['stash'], times)
        ctx.mark_non_differentiable(out['weights'])
        return tuple(out[k] for k in THOMSON_KEYS)

    @staticmethod
    def backward(ctx, g_b, g_den, g_sun, g_obs, g_w=None):
        if all(g is None for g in (g_b, g_den, g_sun, g_obs)):
            return (None,) * (6 + len(ctx.params))
        rays_o, rays_d, z_vals, raw, stash, times = ctx.saved_tensors
        query = ('rays', rays_o, rays_d, times, z_vals)
        g_raw, absmax = ops.thomson_integral_bwd(raw, z_vals, rays_o, rays_d, ctx.constants, LN10, g_b, g_den, g_sun, g_obs)
        return (None,) * 6 + _mlp_param_grads(ctx.params, lambda gW, gb, accumulate: ops.mlp_backward(
            ctx.packed, g_raw, absmax, stash, gW, gb, accumulate=accumulate, query=query))


def thomson_pass(model, constants, rays_o, rays_d, times, z_vals):
    """Dict of one white-light pass' outputs (the keys of :func:`thomson_raw2outputs`).  A ``NeRF`` runs fused (log10 rho);
    a field module with ``field_on_rays`` (SimpleStar, MHDModel: ln rho) is evaluated by its own kernel and then integrated,
    differentiable w.r.t. whatever parameters its ``field_on_rays`` carries gradients for."""
    constants = tuple(constants)
    if hasattr(model, 'field_on_rays'):
        raw = _field_raw(model, rays_o, rays_d, z_vals, times)
        return thomson_raw2outputs(raw, z_vals, rays_o, rays_d, constants, 1.0)
    params = _mlp_params(model)
    if _differentiable(params):
        return _thomson_dict(_ThomsonPass.apply(model, constants, rays_o, rays_d, times, z_vals, *params))
    raw = ops.emission_render_fwd(model.packed(), rays_o, rays_d, times, z_vals, 0.0, want_raw=True,
                                  probe_sensitivity=LN10)['raw']
    out = ops.thomson_integral_fwd(raw, z_vals, rays_o, rays_d, constants, LN10)
    return _thomson_dict([out[k] for k in THOMSON_KEYS])
