"""CPU-only checks of the any-size fp32 backward (no GPU): its workspace does not depend on the batch, and the switch that selects it
parses like the other precision switches."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    import sunerf_hip
    if not os.path.exists(sunerf_hip.LIB_PATH):
        import subprocess
        subprocess.check_call(['bash', os.path.join(ROOT, '2024-hl-spi3s-sunerf_amd', 'csrc', 'build.sh')])
    return sunerf_hip.load()


def test_workspace_is_bounded_and_independent_of_the_batch(lib):
    """The query takes no sample count; every supported shape gets a non-zero size, below 2 GB at d_filter 512 even with the most
    layers -- where the small-batch kernel needs ~19 KB per sample (79 GB at 32768 x 128 rays x samples)."""
    for d in (64, 128, 256, 512):
        for nl in range(2, 17):
            assert lib.sunerf_mlp_backward_exact_chunked_workspace_bytes(d, nl) > 0, (d, nl)
    assert lib.sunerf_mlp_backward_exact_chunked_workspace_bytes(512, 16) < 2 << 30
    assert lib.sunerf_mlp_backward_exact_chunked_workspace_bytes(256, 9) < 1 << 30
    small = lib.sunerf_mlp_backward_exact_workspace_bytes(32768 * 128, 256, 9)
    assert small > 40 * lib.sunerf_mlp_backward_exact_chunked_workspace_bytes(256, 9)
    for d, nl in ((0, 9), (513, 9), (256, 1), (256, 17)):
        assert lib.sunerf_mlp_backward_exact_chunked_workspace_bytes(d, nl) == 0


def test_backward_precision_switch(monkeypatch):
    from sunerf_hip import ops
    monkeypatch.delenv('SUNERF_BACKWARD_PRECISION', raising=False)
    assert ops.backward_precision() == 'default'
    assert ops._stash_wanted(True) and not ops._stash_wanted(False)
    for v, want in (('default', 'default'), ('Exact', 'exact'), (' exact ', 'exact'), ('', 'default')):
        monkeypatch.setenv('SUNERF_BACKWARD_PRECISION', v)
        assert ops.backward_precision() == want, v
    monkeypatch.setenv('SUNERF_BACKWARD_PRECISION', 'exact')
    assert not ops._stash_wanted(True)
    for bad in ('fp32', 'fast', '1'):
        monkeypatch.setenv('SUNERF_BACKWARD_PRECISION', bad)
        with pytest.raises(ValueError):
            ops.backward_precision()
