"""The attention block's train step under y.sum() (one cotangent row for every token) at 24 x 8 = 192
(batch, head) pairs, the smallest count at which the out-projection's dX is handed to attn_bwd_proj
automatically: loss and every gradient are the same bits with the broadcast-row GEMM phase
(LJS_ATTN_BWD_PROJ_BCAST unset) and without it (= 0), and both launch attn_bwd_proj (run on a real
MI355X: -m gpu)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_block_step_equal_with_and_without_the_broadcast_phase(gpu_devices, monkeypatch):
    gpu_devices(1)
    from learning_jax_sharding_amd.ops import hip
    from learning_jax_sharding_amd.tree_util import tree_leaves
    from test_gpu_e2e import _run_block
    res, names, path = {}, {}, {}
    for on in (True, False):
        if on:
            monkeypatch.delenv("LJS_ATTN_BWD_PROJ_BCAST", raising=False)
        else:
            monkeypatch.setenv("LJS_ATTN_BWD_PROJ_BCAST", "0")
        _run_block((1, 1), B=24, S=256, M=96)   # (shadows, workspaces: the logged run launches the step only)
        with hip.launch_log() as log:
            res[on] = _run_block((1, 1), B=24, S=256, M=96)
        assert log.total <= 32, log.total
        names[on] = [r["name"] for r in log]
        path[on] = hip.attn_bwd_proj_last_path()
    assert "attn_bwd_proj" in names[True] and "attn_bwd_proj" in names[False], names
    assert names[True] == names[False]
    assert path == {True: 1, False: 0}
    assert res[True][0] == res[False][0]
    leaves = {on: tree_leaves(res[on][1]) for on in res}
    assert len(leaves[True]) == len(leaves[False]) > 0
    for a, b in zip(leaves[True], leaves[False]):
        assert not np.isnan(a).any()
        np.testing.assert_array_equal(a, b)
