"""attn_bwd_proj's plan does not know the broadcast-row GEMM phase: dy_ld = 0 and dy_ld = M plan the
one launch entry they always did, with LJS_ATTN_BWD_PROJ_BCAST set either way, and the choice between
the two kernel instances is no tenth row of the switch table (answered by the built library without a
GPU, as tests/test_attn_picks.py)."""
import os

import pytest

from learning_jax_sharding_amd.ops import hip


@pytest.fixture(scope="module")
def planned():
    if not os.path.exists(hip._LIBPATH):
        from learning_jax_sharding_amd.csrc import build
        build.build_all()
    hip.lib()


def _entry(B, H):
    return [{"name": "attn_bwd_proj", "grid": (B * H, 1, 1), "blocks": B * H, "block": 512, "acc_mode": None}]


@pytest.mark.parametrize("knob", [None, "0", "1"])
def test_plan_entry_is_the_same_for_a_row_and_for_rows(planned, monkeypatch, knob):
    if knob is None:
        monkeypatch.delenv("LJS_ATTN_BWD_PROJ_BCAST", raising=False)
    else:
        monkeypatch.setenv("LJS_ATTN_BWD_PROJ_BCAST", knob)
    try:
        for B, H, M, forced in ((64, 8, 640, None), (24, 8, 96, None), (1, 1, 32, True), (2, 3, 672, True),
                                (2, 3, 4096, True)):
            hip.set_attention_bwd_proj(forced)
            for ld in (0, M):
                plan = hip.attn_plan("bwd_proj", B, 256, 256, H, M=M, dy_ld=ld)
                assert plan["err"] == 0 and plan["launches"] == _entry(B, H) and plan["vst"][0] == 1, (B, H, M, ld, plan)
    finally:
        hip.set_attention_bwd_proj(None)


def test_switch_table_keeps_nine_rows(planned):
    L = hip.lib()
    assert len(hip._ATTN_SWITCHES) == 9 and L.ljs_attn_set(9, 1) != 0 and L.ljs_attn_get(9) == -1
    assert L.ljs_attn_bwd_proj_last_path() in (-1, 0, 1)
