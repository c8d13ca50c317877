"""The closed scene of tests/test_noise_gate_host.py (a drifting blob and a travelling sine under shot noise, 16 x 40 x 48) noise
gated on the device: the RMS error against the truth before and after, for blocks of 1, 8 and 16 frames in both modes, next to the
fp64 restatement's figure.  One JSON line.

    python tools/noise_gate_loop.py
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, '2024-hl-spi3s-sunerf_amd'), os.path.join(ROOT, 'tests')]


def main():
    import noise_gate_reference as nr
    from sunerf_hip.noise_gate import noise_gate
    from test_noise_gate_host import closed_scene
    frames, truth, params = closed_scene()
    x = torch.from_numpy(frames).cuda()
    rms = lambda img: float(np.sqrt(np.mean((img - truth) ** 2)))          # noqa: E731
    rows = []
    for bt in (1, 8, 16):
        for mode, gamma in (('gate', 3.0), ('wiener', 1.5)):
            got = noise_gate(x, a=params[:, 0], b=params[:, 1], block_t=bt, mode=mode, n_sigma=gamma)
            want, _ = nr.noise_gate(frames, params=params, bt=bt, mode=nr.GATE if mode == 'gate' else nr.WIENER, gamma=gamma)
            rows.append({'block_t': bt, 'mode': mode, 'n_sigma': gamma, 'rms_device': round(rms(got['image'].cpu().numpy().astype(np.float64)), 4),
                         'rms_restatement': round(rms(want), 4), 'kept': int(got['n_kept'][0]), 'coefficients': int(got['n_coefficients'][0])})
    print(json.dumps({'scene': list(frames.shape), 'rms_before': round(rms(frames.astype(np.float64)), 4), 'rows': rows}))


if __name__ == '__main__':
    main()
