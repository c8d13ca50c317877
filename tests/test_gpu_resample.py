"""Hierarchical resampler (csrc/sampler.hip: sunerf_hier_resample, sunerf_sample_pdf) against orc.hierarchical_z /
orc.sample_pdf at the training shapes: 64 -> 128 (headline), 128 -> 128 (config 5), 128 -> 256 (more than 64 KiB of LDS),
400 -> 80 (163 584 B, the largest LDS that fits) and the minimum 3 -> 1; N = 1, 31, 33 (partial workgroups of 32 rays) and
4099.  Weight rows include all-zero and one-hot rows; positions u are shared and per ray.  The insertion-sort merge (new
samples not ascending, or coarse z not ascending) is driven through the C entry point, which ops.hier_resample bypasses by
sorting per-ray u.  Samples are compared with test_gpu_stages._resample_close; z_comb must be sorted, hold the same
multiset as sort(cat(z, new_z)) and be bit-identical across reruns."""
import pytest
import torch

import sunerf_oracle as orc
from test_gpu_stages import _resample_close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    from sunerf_hip import ops as _ops
    return _ops


def make_rays(n, sc, seed, descending_pairs=False):
    gen = torch.Generator().manual_seed(seed)
    near = 213.5 + 0.6 * torch.rand(n, 1, generator=gen)
    far = near + 1.5 + 1.5 * torch.rand(n, 1, generator=gen)
    t = torch.linspace(0., 1., sc) + (torch.rand(n, sc, generator=gen) - 0.5) * (0.8 / (sc - 1))   # jitter inside the bin
    z = near * (1 - t) + far * t
    if descending_pairs:                                   # non-ascending coarse z in every other ray
        k = torch.randint(sc - 1, (n,), generator=gen)
        rows = torch.arange(n)[torch.arange(n) % 2 == 0]
        a, b = z[rows, k[rows]].clone(), z[rows, k[rows] + 1].clone()
        z[rows, k[rows]], z[rows, k[rows] + 1] = b, a
    w = torch.rand(n, sc, generator=gen) ** 4
    w[torch.arange(n) % 5 == 1] = 0.                       # all-zero rows
    # one-hot rows: every 16th.  At u = 1 such a row's last CDF step sits at the reference's 1e-5 threshold, so one sample
    # per row may take either branch (test_gpu_stages._resample_close): more of them would exceed its 0.1 % budget
    hot = torch.arange(n)[torch.arange(n) % 16 == 3]
    w[hot] = 0.
    w[hot, torch.randint(1, sc - 1, (hot.numel(),), generator=gen)] = 1.   # one-hot rows (inside the pdf's w[1:-1])
    return z.float().contiguous(), w.float().contiguous()


def hier_resample_c(ops, z, w, u):
    """sunerf_hier_resample as it is: per-ray u handed over unsorted."""
    from sunerf_hip import lib as _l
    n, sc = z.shape
    sf = u.shape[-1]
    new_z = torch.empty(n, sf, device='cuda')
    z_comb = torch.empty(n, sc + sf, device='cuda')
    _l.call(z.device, 'sunerf_hier_resample', ops._ptr(z), ops._ptr(w), ops._ptr(u), int(u.dim() == 2), n, sc, sf,
            ops._ptr(new_z), ops._ptr(z_comb), ops._stream(z.device))
    return new_z, z_comb


def check(z, nz, zc, nz_o, zc_o, again):
    _resample_close(nz, nz_o, z)
    _resample_close(zc, zc_o, z)
    zc = zc.cpu()
    assert bool((zc[:, 1:] >= zc[:, :-1]).all()), 'z_comb not sorted'
    assert torch.equal(torch.sort(torch.cat([z, nz.cpu()], -1), -1).values, zc), 'z_comb is not sort(cat(z, new_z))'
    assert torch.equal(again[0].cpu(), nz.cpu()) and torch.equal(again[1].cpu(), zc), 'rerun differs'
    return (nz.cpu() - nz_o).abs().max().item()


@pytest.mark.parametrize('n', [1, 31, 33, 4099])
@pytest.mark.parametrize('sc,sf', [(3, 1), (64, 128), (128, 128), (128, 256), (400, 80)])
def test_hier_resample_training_shapes(ops, sc, sf, n):
    z, w = make_rays(n, sc, seed=sc * 131 + sf * 7 + n)
    zd, wd = z.cuda(), w.cuda()
    worst = {}
    u_shared = torch.linspace(0., 1., sf)
    u_ray = torch.rand(n, sf, generator=torch.Generator().manual_seed(n + sf))
    for name, u in (('shared u', u_shared), ('per-ray u', u_ray)):
        nz_o, zc_o = orc.hierarchical_z(z, w, sf, u=u)
        nz, zc = ops.hier_resample(zd, wd, u.cuda())
        worst[name] = check(z, nz, zc, nz_o, zc_o, ops.hier_resample(zd, wd, u.cuda()))
        # HierarchicalSampler.sample_pdf by itself on the same bins / pdf weights
        bins, pw = (0.5 * (z[:, 1:] + z[:, :-1])).contiguous(), w[:, 1:-1].contiguous()
        s = ops.sample_pdf(bins.cuda(), pw.cuda(), u.cuda())
        _resample_close(s, orc.sample_pdf(bins, pw, u), z)
        assert torch.equal(s, ops.sample_pdf(bins.cuda(), pw.cuda(), u.cuda()))
    # insertion-sort merge: per-ray u left unsorted (C entry point), and non-ascending coarse z
    nz_o, zc_o = orc.hierarchical_z(z, w, sf, u=u_ray)
    worst['unsorted u'] = check(z, *hier_resample_c(ops, zd, wd, u_ray.cuda()), nz_o, zc_o,
                                hier_resample_c(ops, zd, wd, u_ray.cuda()))
    zn, wn = make_rays(n, sc, seed=sc * 131 + sf * 7 + n, descending_pairs=True)
    for name, u in (('descending z', u_shared), ('descending z, unsorted u', u_ray)):
        nz_o, zc_o = orc.hierarchical_z(zn, wn, sf, u=u)
        worst[name] = check(zn, *hier_resample_c(ops, zn.cuda(), wn.cuda(), u.cuda()), nz_o, zc_o,
                            hier_resample_c(ops, zn.cuda(), wn.cuda(), u.cuda()))
    torch.cuda.synchronize()
    print(f'N={n} Sc={sc} Sf={sf}: max |new_z - oracle| ' + ', '.join(f'{k} {v:.1e}' for k, v in worst.items()))


def test_hier_resample_lds_limit(ops):
    """401 -> 80 needs 163 968 B of LDS: refused; 400 -> 80 (163 584 B) runs above."""
    z, w = make_rays(4, 401, seed=1)
    with pytest.raises(ValueError, match='unsupported'):
        ops.hier_resample(z.cuda(), w.cuda(), torch.linspace(0., 1., 80).cuda())
