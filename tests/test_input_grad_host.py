"""CPU-only checks of the input-gradient backward (csrc/bwd_exact.hip: sunerf_mlp_input_grad_exact; no GPU): both entry points are
declared and exported, the workspace query, and every argument error returns its documented code before anything is launched
(no device is touched: the pointers below are never dereferenced)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('sunerf_mlp_input_grad_exact_workspace_bytes', 'sunerf_mlp_input_grad_exact')
BADARG, UNSUPPORTED, WORKSPACE = -1, -2, -3


@pytest.fixture(scope='module')
def lib():
    import sunerf_hip
    if not os.path.exists(sunerf_hip.LIB_PATH):
        import subprocess
        subprocess.check_call(['bash', os.path.join(ROOT, '2024-hl-spi3s-sunerf_amd', 'csrc', 'build.sh')])
    return sunerf_hip.load()


def test_declared_and_exported(lib):
    import sunerf_hip
    header = open(os.path.join(ROOT, 'include', 'sunerf_hip.h')).read()
    declared = set(re.findall(r'\b(sunerf_\w+)\s*\(', header))
    for name in NEW:
        assert name in declared and name in sunerf_hip.symbols('core')
        assert getattr(lib, name) is not None
    assert lib.sunerf_abi_version() == 9


def test_workspace_size(lib):
    """Independent of the batch; the chunked kernel's workspace plus the chunk's encoder-feature gradient (84 fp32), per-sample point
    gradient (4 fp64) and the ray carry; zero outside the supported shapes."""
    for d in (64, 100, 256, 512):
        for nl in (2, 9, 16):
            base = lib.sunerf_mlp_backward_exact_chunked_workspace_bytes(d, nl)
            chunk = 16384 if d > 256 else 32768
            got = lib.sunerf_mlp_input_grad_exact_workspace_bytes(d, nl)
            assert got >= base + chunk * (84 * 4 + 4 * 8), (d, nl)
            assert got <= base + chunk * (84 * 4 + 4 * 8) + 4096, (d, nl)
    for d, nl in ((0, 9), (513, 9), (256, 1), (256, 17)):
        assert lib.sunerf_mlp_input_grad_exact_workspace_bytes(d, nl) == 0


def _fake(n):
    """n distinct non-null fake device addresses (never dereferenced: every call below fails its checks first)."""
    return [ctypes.c_void_p(0x1000 * (i + 1)) for i in range(n)]


def _arrays(nl, null_at=None):
    ptrs = [p.value for p in _fake(nl)]
    if null_at is not None:
        ptrs[null_at] = None
    return (ctypes.c_void_p * nl)(*ptrs)


def _call(lib, *, nl=3, d=64, d_out=2, rays=True, points=False, n=4, s=8, g_raw=True, ws=True, ws_bytes=None, params=True,
          gw=None, gb=None, out_points=False, out_rays=(True, True, True, True), W=None, B=None):
    p = ctypes.c_void_p(0x100000)
    ray_args = (p, p, p, p) if rays else (None, None, None, None)
    if ws_bytes is None:
        ws_bytes = lib.sunerf_mlp_input_grad_exact_workspace_bytes(d, nl) or (1 << 40)
    GW = gw if gw is not None else (_arrays(nl) if params else None)
    GB = gb if gb is not None else (_arrays(nl) if params else None)
    outs = [p if w else None for w in out_rays]
    return lib.sunerf_mlp_input_grad_exact(W if W is not None else _arrays(nl), B if B is not None else _arrays(nl), nl, d, d_out,
                                           *ray_args, p if points else None, n, s, p if g_raw else None, p if ws else None, ws_bytes,
                                           GW, GB, 0, p if out_points else None, *outs, None)


def test_argument_errors_without_gpu(lib):
    # null arrays / pointers
    assert lib.sunerf_mlp_input_grad_exact(None, _arrays(3), 3, 64, 2, None, None, None, None, None, 4, 8, None, None, 0, None,
                                           None, 0, None, None, None, None, None, None) == BADARG
    assert _call(lib, g_raw=False) == BADARG
    assert _call(lib, ws=False) == BADARG
    assert _call(lib, W=_arrays(3, null_at=1)) == BADARG
    assert _call(lib, B=_arrays(3, null_at=2)) == BADARG
    assert _call(lib, rays=False) == BADARG                                   # neither rays nor points
    # parameter gradients: both arrays or neither, and no null layer inside
    assert _call(lib, gw=_arrays(3), params=False) == BADARG
    assert _call(lib, gb=_arrays(3), params=False) == BADARG
    assert _call(lib, gw=_arrays(3, null_at=0)) == BADARG
    assert _call(lib, gb=_arrays(3, null_at=2)) == BADARG
    # sizes
    assert _call(lib, n=0) == BADARG
    assert _call(lib, s=0) == BADARG
    assert _call(lib, d_out=0) == BADARG
    assert _call(lib, d=0) == BADARG
    assert _call(lib, d=513) == UNSUPPORTED
    assert _call(lib, d_out=3) == UNSUPPORTED
    assert _call(lib, nl=1) == UNSUPPORTED
    assert _call(lib, nl=17) == UNSUPPORTED
    assert _call(lib, n=1 << 33, s=1 << 8) == UNSUPPORTED                   # N * S = 2^41 > 2^40
    # outputs: ray mode needs a ray gradient and no point gradient; points mode the reverse
    assert _call(lib, out_rays=(False, False, False, False)) == BADARG
    assert _call(lib, out_points=True) == BADARG
    assert _call(lib, rays=False, points=True, out_rays=(False, False, False, False)) == BADARG
    assert _call(lib, rays=False, points=True, out_points=True, out_rays=(False, False, True, False)) == BADARG
    # workspace one byte short
    need = lib.sunerf_mlp_input_grad_exact_workspace_bytes(64, 3)
    assert _call(lib, ws_bytes=need - 1) == WORKSPACE
    assert _call(lib, rays=False, points=True, out_points=True, out_rays=(False,) * 4, params=False, ws_bytes=need - 1) == WORKSPACE
    # the chunked kernel's own workspace is too small for the input gradients
    assert _call(lib, ws_bytes=lib.sunerf_mlp_backward_exact_chunked_workspace_bytes(64, 3)) == WORKSPACE


def test_chunked_entry_point_still_requires_parameter_gradients(lib):
    """The shared argument checks did not loosen sunerf_mlp_backward_exact_chunked: its gradient arrays stay mandatory."""
    p = ctypes.c_void_p(0x100000)
    ws = lib.sunerf_mlp_backward_exact_chunked_workspace_bytes(64, 3)
    assert lib.sunerf_mlp_backward_exact_chunked(_arrays(3), _arrays(3), 3, 64, 2, p, p, p, p, None, 4, 8, p, p, ws, None, None, 0,
                                                 None) == BADARG
    assert lib.sunerf_mlp_backward_exact_chunked(_arrays(3), _arrays(3), 3, 64, 2, p, p, p, p, None, 4, 8, p, p, ws - 1, _arrays(3),
                                                 _arrays(3), 0, None) == WORKSPACE
