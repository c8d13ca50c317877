"""Container only (skipped where the reference checkout is absent): the training-set files in the REFERENCE's own reader, and
the reference's own hold-out / flatten / time-broadcast lines against the numpy restatement.

The reference side runs in a child interpreter whose ``sunerf`` package is the reference's (as tests/test_export_to_reference.py
does).  No reference code is committed: the child reads ``sunerf/data/loader/single_channel.py`` of the checkout and executes
its lines 34-48 (select test image ... ``images.reshape(-1, 1)``) on arrays the parent hands over.

The files come from ``ObservationSet.write_npy`` where a ROCm device is present; without one they are written from the
restatement the GPU suite holds the kernel to bit for bit (tests/test_gpu_observations.py), through the same
``np.lib.format.open_memmap`` route and under the same names."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import observations_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(not os.path.isdir('/root/reference'), reason='needs the reference checkout (container only)')

CHILD = r'''
import sys, textwrap, numpy as np
sys.path.insert(0, sys.argv[1])                      # oracle/ (ref_import)
import ref_import
ref_import.import_reference()
from sunerf.data import dataset
assert dataset.__file__.startswith('/root/reference/'), dataset.__file__
work, batch_size = sys.argv[2], int(sys.argv[3])
names = {'rays': 'rays_batches.npy', 'time': 'times_batches.npy', 'target_image': 'images_batches.npy'}
data = dataset.MmapDataset({k: work + '/' + v for k, v in names.items()}, batch_size=batch_size)
out = {'n_batches': np.int64(len(data))}
for i in range(len(data)):
    for k, v in data[i].items():
        out['batch%d__%s' % (i, k)] = v
# the reference's own lines: hold-out index, masks, flatten, time broadcast (single_channel.py:34-48)
source = open('/root/reference/sunerf/data/loader/single_channel.py').read().split('\n')[33:48]
assert 'test_idx = len(images) // 6' in source[1] and 'images = images.reshape(-1, 1)' in source[-1], source
inp = np.load(sys.argv[4])
scope = {'np': np, 'images': inp['images'], 'rays': inp['rays'], 'times': inp['times']}
exec(textwrap.dedent('\n'.join(source)), scope)
for k in ('rays', 'times', 'images', 'valid_rays', 'valid_times', 'valid_images', 'test_idx'):
    out['lines__' + k] = np.asarray(scope[k])
np.savez(sys.argv[5], **out)
'''


def _views(n_views=7, height=6, width=5):
    """Equal-shaped single-channel views (the reference stacks them into one array, single_channel.py:29-30)."""
    rng = np.random.default_rng(8)
    views = []
    for k in range(n_views):
        views.append(dict(planes=rng.uniform(0, 1, size=(1, height, width)).astype(np.float32), wavelengths=[1.0], downscale=1,
                          time=np.float32(0.125 * k), rays_o=rng.normal(size=(height * width, 3)).astype(np.float32),
                          rays_d=rng.normal(size=(height * width, 3)).astype(np.float32)))
    return views


def test_files_open_in_the_references_dataset_and_its_flatten_lines_agree(tmp_path):
    from sunerf_hip.observations import FILE_NAMES, hold_out_index
    views = _views()
    held = hold_out_index(len(views))
    train = [v for i, v in enumerate(views) if i != held]
    work, batch_size, seed = str(tmp_path / 'work'), 32, 6
    want = ref.assemble(train, None, seed, 0)
    batches = None
    if torch.cuda.is_available():
        from sunerf_hip.observations import ObservationSet
        obs = ObservationSet(device='cuda')
        axis = np.linspace(-4e-3, 4e-3, 6)
        for k, v in enumerate(views):
            obs.add_view(v['planes'], 0.1 * k, 0.7 * k, 215.0, float(v['time']), tx=axis[:5], ty=axis)
        obs.hold_out('reference')
        obs.write_npy(work, seed=seed)
        pool = obs.pool(batch_size=batch_size, seed=seed)
        batches = [{k: v.cpu().numpy() for k, v in pool.batch(i).items()} for i in range(len(pool))]
        assert np.array_equal(pool.data['target_image'].cpu().numpy(), want['target_image'])      # same records as the restatement
    else:
        os.makedirs(work)
        for key in ('rays', 'time', 'target_image'):
            f = np.lib.format.open_memmap(os.path.join(work, FILE_NAMES[key]), mode='w+', dtype=np.float32, shape=want[key].shape)
            f[:] = want[key]
            f.flush()
        n = want['rays'].shape[0]
        batches = [{k: want[k][b:b + batch_size] for k in ('rays', 'time', 'target_image')} for b in range(0, n, batch_size)]
    inputs, outputs = str(tmp_path / 'in.npz'), str(tmp_path / 'out.npz')
    np.savez(inputs, images=np.stack([v['planes'][0] for v in views]),
             rays=np.stack([np.stack([v['rays_o'], v['rays_d']], 1).reshape(6, 5, 2, 3) for v in views]),
             times=np.array([v['time'] for v in views], dtype=np.float32))
    env = {k: v for k, v in os.environ.items() if k != 'PYTHONPATH'}
    res = subprocess.run([sys.executable, '-c', CHILD, os.path.join(ROOT, 'oracle'), work, str(batch_size), inputs, outputs],
                         env=env, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert res.returncode == 0, res.stderr[-3000:]
    got = np.load(outputs)
    # (1) the reference's MmapDataset reads the files: batch i is the pool's batch i
    assert int(got['n_batches']) == len(batches) == -(-want['rays'].shape[0] // batch_size)
    for i, batch in enumerate(batches):
        for key, value in batch.items():
            if key in ('rays', 'time', 'target_image'):
                assert np.array_equal(got[f'batch{i}__{key}'].view(np.int32), np.ascontiguousarray(value).view(np.int32)), (i, key)
    # (2) the reference's hold-out / flatten / broadcast lines give the restatement's unshuffled arrays
    assert int(got['lines__test_idx']) == held
    plain = ref.assemble(train, None, 0, 0, permute=False)
    assert np.array_equal(got['lines__rays'], plain['rays']) and np.array_equal(got['lines__times'], plain['time'])
    assert np.array_equal(got['lines__images'], plain['target_image'])
    one = ref.assemble([views[held]], None, 0, 0, permute=False)
    assert np.array_equal(got['lines__valid_rays'].reshape(-1, 2, 3), one['rays'])
    assert np.array_equal(got['lines__valid_images'].reshape(-1, 1), one['target_image'])
    assert (got['lines__valid_times'] == views[held]['time']).all()
