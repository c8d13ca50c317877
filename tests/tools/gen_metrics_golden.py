"""Writes tests/golden/skimage/g14_ssim_skimage.npz: fp32 image pairs and scikit-image's own SSIM of them, the pin for the fp64
restatement tests/metrics_reference.py and, through it and directly, for csrc/metrics.hip.

Needs numpy and scikit-image only (run it with an interpreter that has scikit-image; the test suite does not):
    python tests/tools/gen_metrics_golden.py
Every case stores ``<name>__target`` and ``<name>__pred`` (fp32, (H, W) or (C, H, W)) and
``<name>__ssim_r1`` / ``<name>__ssim_r255`` = ``structural_similarity(target, pred, data_range=R)`` with the defaults,
per channel for a stack.  ``names`` lists the cases, ``skimage_version`` the library that computed them.
The file lives in a sub-directory of tests/golden: the top level holds the fixtures oracle/gen_golden.py regenerates from
the reference, and this one does not come from there."""
import os

import numpy as np
import skimage
from skimage.metrics import structural_similarity

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'golden', 'skimage', 'g14_ssim_skimage.npz')


def _pair(rng, shape, scale=1.0):
    """A smooth field with noise as the target, the target plus a smaller perturbation as the prediction, in [0, scale]."""
    yy, xx = np.meshgrid(np.linspace(0, 1, shape[-2]), np.linspace(0, 1, shape[-1]), indexing='ij')
    base = 0.5 + 0.3 * np.sin(5 * xx + 3 * yy) * np.cos(4 * yy)
    target = np.clip(base + 0.1 * rng.standard_normal(shape), 0, 1) * scale
    pred = np.clip(target / scale + 0.05 * rng.standard_normal(shape), 0, 1) * scale
    return target.astype(np.float32), pred.astype(np.float32)


def main():
    rng = np.random.default_rng(14)
    cases = {}
    for h, w in ((7, 7), (7, 40), (40, 7), (13, 29), (64, 64), (97, 131)):
        cases[f'r{h}x{w}'] = _pair(rng, (h, w))
    cases['stack3x37x53'] = _pair(rng, (3, 37, 53))
    const = np.full((16, 16), 0.25, np.float32)
    cases['constant'] = (const, np.full((16, 16), 0.75, np.float32))
    same = _pair(rng, (20, 24))[0]
    cases['identical'] = (same, same.copy())
    cases['three_r'] = _pair(rng, (32, 32), scale=3.0)
    out = {'names': np.array(sorted(cases)), 'skimage_version': np.array(skimage.__version__)}
    for name, (target, pred) in cases.items():
        out[f'{name}__target'], out[f'{name}__pred'] = target, pred
        for r in (1, 255):
            if target.ndim == 3:
                s = np.array([structural_similarity(target[c], pred[c], data_range=r) for c in range(target.shape[0])])
            else:
                s = np.float64(structural_similarity(target, pred, data_range=r))
            out[f'{name}__ssim_r{r}'] = s
    np.savez(OUT, **out)
    print(f'wrote {OUT} ({os.path.getsize(OUT)} bytes), scikit-image {skimage.__version__}')


if __name__ == '__main__':
    main()
