"""Two ranks sharing one MI355X over gloo, the way a training run reaches the optimiser:

* through ``sunerf.run_mi355x``, which seeds every rank differently (so each builds a different network): ``ClipAdam`` must
  broadcast rank 0's parameters, and the packed-weight cache of the sanity pass must not keep serving the old weights;
* through Lightning 1.9's automatic optimisation (``optimizer.step(closure)``, the clip hook inside the closure): the clip must act
  on the all-reduced total gradient as in the reference's ``dp`` run, and the non-finite count must reach the all-reduce so that
  ``on_train_batch_end`` raises on every rank.

tests/test_gpu_dist.py seeds every rank alike and calls ClipAdam.step with the count itself, which hid both defects."""
import datetime
import os
import subprocess
import sys
import textwrap

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, '2024-hl-spi3s-sunerf_amd')
STEPS = 3
N_RAYS = 64
LAMBDA_IMAGE = 4.0      # Lightning drive: puts every rank's local gradient norm above the clip value 0.5 (asserted)


def _setup_paths():
    for p in (PKG, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
        if p not in sys.path:
            sys.path.insert(0, p)


def _emission_module(lambda_image=1.0):
    from sunerf.model.sunerf import EmissionSuNeRFModule
    return EmissionSuNeRFModule(Rs_per_ds=1.0, seconds_per_dt=1.0, image_scaling_config={'vmax': 1, 'a': 0.005},
                                lambda_image=lambda_image,
                                sampling_config={'type': 'stratified', 'n_samples': 32, 'perturb': False},
                                hierarchical_sampling_config={'type': 'hierarchical', 'n_samples': 32},
                                model_config={'d_filter': 64}, lr_config={'start': 1e-3, 'end': 1e-4, 'iterations': 100}).cuda()


def _whole_batch():
    """64 rays; targets far from the images, on opposite sides (asinh-scaled ~-1.6 for rays 0-31, ~+1.6 for rays 32-63), so
    the two ranks' local gradient norms differ (by ~5x at the start)."""
    from sunerf_hip.rays import observer_rays
    o, d = observer_rays(8, device='cuda')
    gen = torch.Generator().manual_seed(17)
    t = torch.rand(N_RAYS, 1, generator=gen)
    target = torch.cat([-20.0 - 20.0 * torch.rand(N_RAYS // 2, 1, generator=gen),
                        20.0 + 20.0 * torch.rand(N_RAYS // 2, 1, generator=gen)])
    return {'tracing': {'rays': torch.stack([o, d], 1), 'time': t.cuda(), 'target_image': target.cuda()}}


def _shard(batch, rank, world):
    from sunerf_hip.dist import shard_range
    b, e = shard_range(N_RAYS, rank, world)
    return {'tracing': {k: v[b:e].contiguous() for k, v in batch['tracing'].items()}}


def _params(module):
    return [p.detach().cpu().clone() for p in module.rendering.parameters()]


def _assert_matches_single_process(got, ref, init):
    """The tolerance of test_gpu_dist.py::test_two_rank_fused_step_equals_single_process: the sharded step sums the gradient in
    another order than the single process, so agreement is to a small fraction of how far the weights moved."""
    for a, b, p0 in zip(got, ref, init):
        moved = (b - p0).abs().max().item()
        assert (a - b).abs().max().item() <= 0.05 * moved + 1e-7, ((a - b).abs().max().item(), moved)


# ---------------------------------------------------------------------------------------------------------------- run_mi355x
STUB = '''
import os, sys
import torch
import torch.distributed as dist
sys.path.insert(0, {tests!r})
from test_gpu_replicas import _emission_module, _params, _shard, _whole_batch
from sunerf.model.sunerf import fit_steps

if __name__ == '__main__':
    rank, world = dist.get_rank(), dist.get_world_size()
    module = _emission_module()               # NOT seeded here: sunerf.run_mi355x seeded this rank with SUNERF_SEED + rank
    rec = {{'built': _params(module), 'steps': []}}
    whole = _whole_batch()
    o, d = whole['tracing']['rays'][:, 0].contiguous(), whole['tracing']['rays'][:, 1].contiguous()
    t = whole['tracing']['time']
    with torch.no_grad():                     # Lightning's sanity pass: packs the weights this rank built
        rec['image_before'] = module.rendering(o, d, t)['fine_image'].cpu()
    configure, end = module.configure_optimizers, module.on_train_batch_end

    def configure_and_record():
        out = configure()
        rec['configured'] = _params(module)
        return out

    def end_and_record(*args, **kwargs):
        end(*args, **kwargs)
        rec['steps'].append(_params(module))
        if len(rec['steps']) == 1:
            with torch.no_grad():
                rec['image_after_first_step'] = module.rendering(o, d, t)['fine_image'].cpu()
    module.configure_optimizers, module.on_train_batch_end = configure_and_record, end_and_record
    fit_steps(module, [_shard(whole, rank, world)] * {steps})
    torch.save(rec, os.path.join(sys.argv[1], f'replica{{rank}}.pt'))
'''


def test_ranks_seeded_apart_train_one_model(tmp_path):
    script = tmp_path / 'replica_stub.py'
    script.write_text(textwrap.dedent(STUB.format(tests=os.path.join(ROOT, 'tests'), steps=STEPS)))
    env = dict(os.environ, SUNERF_DIST_BACKEND='gloo',
               PYTHONPATH=os.pathsep.join([PKG, os.path.join(ROOT, 'oracle'), os.environ.get('PYTHONPATH', '')]))
    subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr',
                    '127.0.0.1', '--master-port', '29583', '-m', 'sunerf.run_mi355x', str(script), str(tmp_path)],
                   check=True, env=env, timeout=300, cwd=str(tmp_path))
    r0, r1 = (torch.load(tmp_path / f'replica{r}.pt') for r in (0, 1))
    assert any(not torch.equal(a, b) for a, b in zip(r0['built'], r1['built']))      # the ranks really were seeded apart
    assert not torch.equal(r0['image_before'], r1['image_before'])
    for key in ['configured'] + [i for i in range(STEPS)]:
        x0 = r0[key] if key == 'configured' else r0['steps'][key]
        x1 = r1[key] if key == 'configured' else r1['steps'][key]
        for a, b in zip(x0, x1):
            assert torch.equal(a, b), key                                             # bit-identical replicas
    for a, b in zip(r1['configured'], r0['built']):
        assert torch.equal(a, b)                                                      # rank 0's weights, on every rank
    assert torch.equal(r0['image_after_first_step'], r1['image_after_first_step'])   # the packed cache followed
    _setup_paths()
    single = _emission_module()
    with torch.no_grad():
        for p, w in zip(single.rendering.parameters(), r0['built']):
            p.copy_(w)
    from sunerf.model.sunerf import fit_steps
    fit_steps(single, [_whole_batch()] * STEPS)
    _assert_matches_single_process(r0['steps'][-1], _params(single), r0['built'])


# ---------------------------------------------------------------------------------------------------------- Lightning 1.9 drive
def _lightning_1_9_step(module, optimizer, batch, batch_idx, local_norms):
    """Lightning 1.9.3's automatic optimisation for one batch, as plainly as it can be written (Trainer(gradient_clip_val=0.5),
    run_emission.py:72): ``optimizer.step(closure)``; the closure runs ``training_step``, ``zero_grad``, ``backward``, then
    PrecisionPlugin._after_closure calls ``configure_gradient_clipping(optimizer, optimizer_idx, gradient_clip_val=0.5,
    gradient_clip_algorithm='norm')`` -- whose LightningModule default clips the optimiser's LOCAL gradients -- and after the
    step the loop calls ``on_train_batch_end``."""
    from sunerf.model.sunerf import LightningModule
    hook = getattr(type(module), 'configure_gradient_clipping', None)

    def closure():
        loss = module.training_step(batch, batch_idx)
        optimizer.zero_grad()
        loss.backward()
        local_norms.append(torch.linalg.vector_norm(optimizer.flat_grads).item())
        if hook is not None and hook is not getattr(LightningModule, 'configure_gradient_clipping', None):
            module.configure_gradient_clipping(optimizer, 0, gradient_clip_val=0.5, gradient_clip_algorithm='norm')
        else:
            torch.nn.utils.clip_grad_norm_([p for g in optimizer.param_groups for p in g['params']], 0.5)
        return loss
    optimizer.step(closure=closure)
    module.on_train_batch_end(None, batch, batch_idx)


def _nan_in(outputs):
    out = dict(outputs)
    out['height_map'] = out['height_map'].clone()
    out['height_map'].view(-1)[3] = float('nan')
    return out


def _worker_lightning(rank, world, port, out_dir):
    _setup_paths()
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    batch = _shard(_whole_batch(), rank, world)
    rec = {}
    # 1. three clean steps
    torch.manual_seed(5)
    module = _emission_module(LAMBDA_IMAGE)
    (optimizer,), _ = module.configure_optimizers()
    norms = []
    for i in range(STEPS):
        _lightning_1_9_step(module, optimizer, batch, i, norms)
    rec['params'], rec['local_norms'], rec['total_norm'] = _params(module), norms, optimizer.norm[0].item()
    # 2. step 1: a NaN in rank 1's target (the loss and the gradients are NaN, no OUTPUT is); step 2: a NaN in one of rank 1's
    #    outputs (what the reference asserts on, sunerf.py:105-107; counted by the loss kernel's finite check)
    torch.manual_seed(5)
    module = _emission_module(LAMBDA_IMAGE)
    (optimizer,), _ = module.configure_optimizers()
    render = module.rendering.forward
    log = []
    for i in range(3):
        b = batch
        if rank == 1 and i == 1:
            tgt = batch['tracing']['target_image'].clone()
            tgt[3, 0] = float('nan')
            b = {'tracing': dict(batch['tracing'], target_image=tgt)}
        module.rendering.forward = (lambda *a, **k: _nan_in(render(*a, **k))) if rank == 1 and i == 2 else render
        raised = None
        try:
            _lightning_1_9_step(module, optimizer, b, i, [])
        except AssertionError as e:
            raised = str(e)
        log.append({'skipped': optimizer.skipped_last_step(), 'steps': optimizer.step_count, 'raised': raised,
                    'params': _params(module)})
    rec['nan'] = log
    torch.save(rec, os.path.join(out_dir, f'lightning{rank}.pt'))
    dist.destroy_process_group()


def test_lightning_drive_clips_the_total_gradient_and_raises_on_every_rank(tmp_path):
    world = 2
    mp.spawn(_worker_lightning, args=(world, 29587, str(tmp_path)), nprocs=world, join=True)
    r0, r1 = (torch.load(tmp_path / f'lightning{r}.pt') for r in (0, 1))
    # the premise: every rank's local gradient exceeds the clip value in every step, by different amounts
    assert min(r0['local_norms'] + r1['local_norms']) > 0.5, (r0['local_norms'], r1['local_norms'])
    for a, b in zip(r0['params'], r1['params']):
        assert torch.equal(a, b)
    _setup_paths()
    from sunerf.model.sunerf import fit_steps
    torch.manual_seed(5)
    single = _emission_module(LAMBDA_IMAGE)
    init = _params(single)
    fit_steps(single, [_whole_batch()] * STEPS, gradient_clip_val=0.5)       # clips the TOTAL gradient
    assert abs(r0['total_norm'] - single.optimizer.norm[0].item()) <= 1e-4 * single.optimizer.norm[0].item()
    _assert_matches_single_process(r0['params'], _params(single), init)
    # non-finite values on one rank: the step is skipped on both; the output NaN raises on both
    for log in (r0['nan'], r1['nan']):
        assert [x['skipped'] for x in log] == [False, True, True]
        assert [x['steps'] for x in log] == [1, 1, 1]
        assert log[0]['raised'] is None
        assert log[2]['raised'] is not None and 'Numerical Alert' in log[2]['raised']
        for s in (1, 2):
            for a, b in zip(log[0]['params'], log[s]['params']):
                assert torch.equal(a, b)
    for s0, s1 in zip(r0['nan'], r1['nan']):
        for a, b in zip(s0['params'], s1['params']):
            assert torch.equal(a, b)
