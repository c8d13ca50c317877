"""The three launching entry points of include/sunerf_hip_instrument.h stay inside their buffers: the checks of
tests/test_gpu_abi_extents.py (runs A and B with sentinel and NaN fills, guards, inputs untouched, outputs equal to the wrapper
by bits and independent of what they held, the empty call, the header's rejections) on cases built with ``abi_cases.Ctx`` /
``Case`` and the guarded arena of tests/abi_arena.py, with the extents the header states.

The cases live in this file's own table ``INSTRUMENT_CASES`` (tests/test_abi_tables_host.py holds it to the table's symbols)."""
import pytest
import torch

import abi_cases as ac
from abi_arena import OUT
from abi_cases import F32, I32, STREAM, U8, Case, Ctx

pytestmark = pytest.mark.gpu

TILES = ('instrument.hip: correlation tiles of T x T output pixels, T = min(32, (127 - max(kh, kw)) / bin + 1), 256 threads with up '
         'to four outputs each; noise and philox 256 elements per workgroup')
# (planes, height, width, psf rows, psf columns, bin, per-plane kernels, boundary): a kernel larger than the image, a single pixel,
# one tile plus one / two tiles plus one, a ragged batch with per-plane kernels, the identity kernel, a binned ragged frame
CORRELATE_SHAPES = [(1, 5, 7, 9, 9, 1, 0, 0), (1, 1, 1, 3, 3, 1, 0, 1), (1, 33, 65, 5, 5, 1, 0, 1), (3, 34, 67, 5, 5, 1, 1, 0),
                    (1, 33, 65, 1, 1, 1, 0, 0), (2, 37, 53, 7, 5, 3, 1, 1), (1, 40, 48, 89, 89, 8, 0, 1)]
# (planes, height, width, flags, with sigma, with saturated): one element, one workgroup plus one, a batch; NULL outputs
NOISE_SHAPES = [(1, 1, 1, 15, 1, 1), (1, 1, 4097, 3, 1, 1), (1, 1, 4097, 15, 0, 0), (3, 17, 23, 13, 1, 0), (2, 9, 31, 2, 0, 1)]
PHILOX_SHAPES = [1, 255, 257, 4099]


def correlate(shape, device):
    from sunerf_hip.instrument import Instrument
    c_, h, w, kh, kw, b, per_plane, boundary = shape
    c = Ctx(device)
    gen = ac._gen(100 * h + w + kh)
    image = c.IN('in', ac._rand(gen, c_, h, w) * 1000.0 - 100.0)
    psf = (ac._rand(gen, c_ if per_plane else 1, kh, kw).double() - 0.1).numpy()
    inst = Instrument(psf=psf if per_plane else psf[0], bin=b, boundary=('zero', 'nearest')[boundary])
    K, (ay, ax) = inst.effective_kernel()
    taps = c.IN('K', torch.from_numpy(K))
    out = c.OUT('out', F32, c_ * (h // b) * (w // b))

    def expected():
        return {'out': inst.expected(image.t.view(c_, h, w))}
    args = [image, c_, h, w, taps, K.shape[0], K.shape[1], K.shape[2], b, ay, ax, inst.scale, boundary, out, STREAM]
    return Case('sunerf_instrument_correlate_bin', shape, c.arena, args, expected, empty={1: 0},
                rejections=[({6: 97}, -2), ({7: 97}, -2), ({8: 9}, -2), ({12: 2}, -2)])          # header: the limits, the boundary


def noise(shape, device):
    from sunerf_hip.instrument import Instrument
    c_, h, w, flags, with_sigma, with_sat = shape
    c = Ctx(device)
    gen = ac._gen(h * 31 + w + flags)
    x = 10.0 ** (ac._rand(gen, c_, h, w) * 7.0 - 2.0)
    if h * w > 8:
        x.view(-1)[1] = float('nan')
        x.view(-1)[2] = float('inf')
        x.view(-1)[3] = -4.0
        x.view(-1)[4] = 0.0
        x.view(-1)[5] = 1e17
    expected_in = c.IN('expected', x)
    inst = Instrument(unit=[2.5, 1.0, 0.5][:c_], exposure=2.9, dn_per_photon=[1.2, 1.0, 2.0][:c_], read_noise=1.5, pedestal=100.0,
                      saturation=3000.0 if flags & 8 else float('inf'), quantise=bool(flags & 4))
    params = c.IN('params', torch.from_numpy(inst.params(c_)))
    image = c.OUT('image', F32, c_ * h * w)
    sigma = c.OUT('sigma', F32, c_ * h * w) if with_sigma else c.NULL('sigma', OUT)
    sat = c.OUT('saturated', U8, c_ * h * w) if with_sat else c.NULL('saturated', OUT)
    seed, offset = 0x123456789ABCDEF0 + h, (1 << 33) + 7

    def expected():
        assert inst.flags(bool(flags & 1), bool(flags & 2)) == flags
        i, s, t = inst.noise(expected_in.t.view(c_, h, w), seed, offset, bool(flags & 1), bool(flags & 2), bool(with_sigma), bool(with_sat))
        return {'image': i, **({'sigma': s} if with_sigma else {}), **({'saturated': t} if with_sat else {})}
    args = [expected_in, c_, h, w, params, seed, offset, flags, image, sigma, sat, STREAM]
    return Case('sunerf_instrument_noise', shape, c.arena, args, expected, empty={1: 0},
                rejections=[({7: 16}, -2), ({7: flags | 32}, -2)])          # header: unknown flag bits


def philox(shape, device):
    n = shape
    c = Ctx(device)
    gen = ac._gen(n)
    words = torch.randint(-2 ** 31, 2 ** 31, (n, 4), generator=gen, dtype=torch.int64).to(I32)
    ctr = c.IN('ctr', words)
    out = c.OUT('out', I32, n * 4)

    def expected():
        from sunerf_hip.instrument import philox as run
        return {'out': run(ctr.t.view(n, 4), 0xA4093822, 0x299F31D0)}
    return Case('sunerf_instrument_philox', shape, c.arena, [ctr, n, 0xA4093822, 0x299F31D0, out, STREAM], expected, empty={1: 0})


INSTRUMENT_CASES = {'sunerf_instrument_correlate_bin': (correlate, tuple(CORRELATE_SHAPES)),
                    'sunerf_instrument_noise': (noise, tuple(NOISE_SHAPES)),
                    'sunerf_instrument_philox': (philox, tuple(PHILOX_SHAPES))}
PAIRS = [(name, shape) for name, (_, shapes) in INSTRUMENT_CASES.items() for shape in shapes]


@pytest.mark.parametrize('name,shape', PAIRS, ids=[f'{n[7:]}-{ac.shape_id(s)}' for n, s in PAIRS])
def test_instrument_entry_point_stays_inside_its_buffers(name, shape):
    import test_gpu_abi_extents as extents
    extents.check_entry_point(INSTRUMENT_CASES[name][0], name, shape)
