"""SimpleStar on MI355X (csrc/dt.hip: ``simple_star_kernel``, ``simple_star_bwd_*``) at its mask boundaries ``r <= 1``,
``1 < r <= Rs`` and ``r > Rs``: samples ON 1 and Rs and one fp32 step to either side, through both forward entry points
and the backward, at the model's default parameters.

Rays with o = 0 and d = (1, 0, 0) make the radius equal z exactly (sqrt(fl(z^2)) = z for a correctly rounded root; the
oracle's torch root of these twelve values is asserted to agree).  Both pieces of the temperature are continuous at Rs -- at
the defaults the ramp's fp32 value at Rs IS T0 -- so the forward cannot tell which side owns Rs; the backward can: only ramp
samples contribute to d / dRs, and the sample at Rs carries most of it here.

Measured on MI355X: both entry points bit-equal; max |err| ln rho 1.9e-6, log10 T 4.8e-7 (bound 1e-5); ln rho(1 + ulp) -
ln rho(1) = 1.9e-6; gradients within 7.8e-8 of fp64 autograd (bound 1e-3).  A scratch build with ``radius < Rs`` for ``<=``
fails the backward test (d / dRs) and, as explained above, not the forward one."""
import math

import numpy as np
import pytest
import torch

import sunerf_oracle as orc

pytestmark = pytest.mark.gpu

STAR_KEYS = ('Rs', 'h0', 'T0', 'rho_0')          # the order of SimpleStar.stellar_parameters and of the kernels' params
T_PHOTOSPHERE = 5777.
BOUND = 1e-5                                     # test_simple_star_field_and_render_match_reference
GRAD_BOUND = 1e-3                                # the project's gradient gate


def _next(a, towards):
    return float(np.nextafter(np.float32(a), np.float32(towards)))


def _setup():
    from sunerf.model.stellar_model import SimpleStar
    star = SimpleStar()
    assert star.t_photosphere == T_PHOTOSPHERE
    params = torch.stack([star.stellar_parameters[k].detach() for k in STAR_KEYS]).float()
    rs = float(params[0])
    z = torch.tensor([[0., 0.5, _next(1, 0), 1., _next(1, 2), 1.1, _next(rs, 0), rs, _next(rs, math.inf), 3., 250., math.nan]],
                     dtype=torch.float32)
    o = torch.zeros(1, 3)
    d = torch.tensor([[1., 0., 0.]])
    return params, rs, o, d, z


def test_field_at_the_mask_boundaries():
    from sunerf_hip import ops
    params, rs, o, d, z = _setup()
    assert 1. < _next(1, 2) < 1.1 and 1. < _next(rs, 0) < rs < _next(rs, math.inf) < 1.1      # Rs = 1.02: 1.1 lies beyond it
    host = {k: float(v) for k, v in zip(STAR_KEYS, params)}
    raw_host = ops.simple_star_field(o.cuda(), d.cuda(), z.cuda(), host['rho_0'], host['h0'], host['T0'], host['Rs'], T_PHOTOSPHERE)
    raw_dev = ops.simple_star_field_dev(o.cuda(), d.cuda(), z.cuda(), params.cuda(), T_PHOTOSPHERE)
    assert raw_host.shape == (1, 12, 2)
    assert torch.equal(raw_host.view(torch.int32), raw_dev.view(torch.int32)), 'host-float and device-parameter entry points differ'
    got = raw_dev[0].cpu()

    pts = torch.stack([z[0], torch.zeros(12), torch.zeros(12)], -1)
    finite = slice(0, 11)
    assert torch.equal(torch.sqrt(pts[finite, 0] ** 2), z[0, finite])                          # the oracle's radius is z too
    want = orc.simple_star_field(pts, *(params[STAR_KEYS.index(k)] for k in ('rho_0', 'h0', 'T0', 'Rs')))
    err = (got[finite] - want[finite]).abs().max(0).values
    print(f'SimpleStar at its mask boundaries: max |err| ln rho {err[0]:.2e}, log10 T {err[1]:.2e} (bound {BOUND:.0e})')
    assert (err <= BOUND).all(), err
    # the NaN row: every mask of the reference fails, rho = T = 0 stay, log(0) = -inf -- in the oracle and in the kernel
    assert (want[11] == -math.inf).all() and (got[11] == -math.inf).all()

    # r <= 1 (0, 0.5, 1 - ulp, 1): the photosphere, bit for bit one value
    assert all(torch.equal(got[i].view(torch.int32), got[0].view(torch.int32)) for i in (1, 2, 3))
    assert abs(got[0, 0].item() - math.log(host['rho_0'])) <= BOUND and abs(got[0, 1].item() - math.log10(T_PHOTOSPHERE)) <= BOUND
    # 1 + ulp: on the other side of both masks; ln rho is continuous there, and T has started up the ramp (8.3 K per ulp)
    assert not torch.equal(got[4].view(torch.int32), got[3].view(torch.int32))
    step = (got[4, 0] - got[3, 0]).abs().item()
    print(f'ln rho(1 + ulp) - ln rho(1) = {step:.2e} (bound {BOUND:.0e}); log10 T(1 + ulp) - log10 T(1) = {(got[4, 1] - got[3, 1]).item():.3e}')
    assert step <= BOUND and got[4, 1] > got[3, 1]
    f = np.float32
    ramp = lambda r: (f(r) - f(1)) * ((f(host['T0']) - f(T_PHOTOSPHERE)) / (f(host['Rs']) - f(1))) + f(T_PHOTOSPHERE)      # noqa: E731
    for row in (4, 6, 7):         # 1 + ulp, Rs - ulp, Rs: the ramp
        assert abs(got[row, 1].item() - math.log10(float(ramp(z[0, row].item())))) <= BOUND, row
    assert got[6, 1] < got[7, 1]                                      # Rs - ulp is 8 K below Rs: still climbing
    # r > Rs (1.1, Rs + ulp, 3, 250): one log10 T, that of T0
    beyond = (5, 8, 9, 10)
    assert all(torch.equal(got[i, 1:].view(torch.int32), got[5, 1:].view(torch.int32)) for i in beyond)
    assert abs(got[5, 1].item() - math.log10(host['T0'])) <= BOUND
    assert float(ramp(rs)) == host['T0']       # why the forward cannot tell which side owns Rs (see the module docstring)
    assert (got[[4, 5, 6, 7, 8, 9, 10], 0] < got[3, 0]).all() and got[10, 0] < got[9, 0] < got[5, 0]      # the density falls outwards


def test_backward_at_the_mask_boundaries():
    from sunerf_hip import ops
    params, rs, o, d, z = _setup()
    gen = torch.Generator().manual_seed(13)
    g_raw = (torch.randn(1, 12, 2, generator=gen) + 0.5).float()
    assert g_raw[0, 7, 1].abs() > 0.1 and g_raw[0, 6, 1].abs() > 0.1          # the samples at Rs and below it weigh in d / dRs
    # fp64 autograd of the oracle field; z is exact in fp64 and so is the radius, so the masks are those of the fp32 kernel
    z64 = z[0].double()
    pts = torch.stack([z64, torch.zeros(12, dtype=torch.float64), torch.zeros(12, dtype=torch.float64)], -1)
    assert torch.equal(pts[:11].norm(dim=-1), z64[:11])
    leaves = {k: params[i].clone().requires_grad_(True) for i, k in enumerate(STAR_KEYS)}
    field = orc.simple_star_field(pts, leaves['rho_0'], leaves['h0'], leaves['T0'], leaves['Rs'])
    field.backward(g_raw[0].double())
    ref = torch.stack([leaves[k].grad.double() for k in STAR_KEYS])
    assert bool(torch.isfinite(ref).all()) and bool((ref != 0).all())
    # what the sample at Rs contributes to d / dRs on the oracle: a mask that gave Rs to the other side would lose it
    T0, tph = float(params[2]), T_PHOTOSPHERE
    at_rs = -g_raw[0, 7, 1].item() * (T0 - tph) / ((rs - 1.) * T0 * math.log(10.))
    assert abs(at_rs) > 0.05 * abs(ref[0].item()), (at_rs, ref[0].item())

    got = ops.simple_star_bwd(o.cuda(), d.cuda(), z.cuda(), params.cuda(), T_PHOTOSPHERE, g_raw.cuda()).cpu().double()
    err = (got - ref).abs() / ref.abs()
    for k, e, a, b in zip(STAR_KEYS, err.tolist(), got.tolist(), ref.tolist()):
        print(f'd/d{k:6s} kernel {a: .8e} oracle {b: .8e} rel err {e:.1e} (bound {GRAD_BOUND:.0e})')
    assert bool((err <= GRAD_BOUND).all()), err
