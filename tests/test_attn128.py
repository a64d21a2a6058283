"""head_dim 128 attention without a GPU: the dispatch of ops/kernels._hip_attn under LJS_ATTN_D128 and
the launcher's plan step (hip.attn128_plan)."""
import warnings

import pytest
import torch


def test_hip_attn_dispatch_at_128(monkeypatch):
    from learning_jax_sharding_amd.ops import kernels as K
    monkeypatch.setattr(K, "use_hip", lambda t: True)
    monkeypatch.setattr(K, "_WARNED_DH", set())
    q = torch.zeros(1, 4, 2, 128, dtype=torch.bfloat16)
    kv = torch.zeros(1, 4, 1, 128, dtype=torch.bfloat16)
    strided = torch.zeros(1, 4, 2, 256, dtype=torch.bfloat16)[..., ::2]
    q64 = torch.zeros(1, 4, 2, 64, dtype=torch.bfloat16)
    monkeypatch.setenv("LJS_ATTN_D128", "1")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert K._hip_attn(q, kv, kv)
        assert not K._hip_attn(q, kv, kv, merge=True)     # the blockwise merge keeps its torch merge
        assert K._hip_attn(q64, q64, q64, merge=True)
    with pytest.warns(UserWarning, match="head_dim 128 operands"):
        assert not K._hip_attn(strided, strided, strided)
    with pytest.warns(UserWarning, match="take head_dim 64; head_dim 128 \\(v 64\\)"):
        assert not K._hip_attn(q, q, q64)
    monkeypatch.delenv("LJS_ATTN_D128")
    with pytest.warns(UserWarning, match="take head_dim 64; head_dim 128 \\(v 128\\) runs the torch attention"):
        assert not K._hip_attn(q, kv, kv)


@pytest.mark.parametrize("kind,B,Sq,Sk,H,Hkv,causal,name,blocks", [
    ("fwd", 2, 320, 320, 8, 2, True, "attn128_fwd<mask=1>", 3 * 8 * 2),
    ("fwd", 1, 256, 256, 2, 2, False, "attn128_fwd<mask=0>", 2 * 2),
    ("fwd", 1, 130, 257, 2, 2, False, "attn128_fwd<mask=1>", 2 * 2),
    ("bwd", 2, 320, 320, 8, 2, True, "attn128_bwd<mask=1>", (3 * 8 + 5 * 2) * 2),
    ("bwd", 1, 128, 512, 4, 1, False, "attn128_bwd<mask=0>", 4 + 8),
    ("bwd", 1, 1, 1, 1, 1, False, "attn128_bwd<mask=1>", 2)])
def test_attn128_plan(kind, B, Sq, Sk, H, Hkv, causal, name, blocks):
    from learning_jax_sharding_amd.ops import hip
    plan = hip.attn128_plan(kind, B, Sq, Sk, H, Hkv, causal=causal)
    assert plan["err"] == 0 and plan["launches"] == [{"name": name, "grid": (blocks, 1, 1), "blocks": blocks,
                                                      "block": 256}]


def test_attn128_plan_rejects():
    from learning_jax_sharding_amd.ops import hip
    bad = [hip.attn128_plan("fwd", 1, 256, 256, 3, 2),                        # H % Hkv != 0
           hip.attn128_plan("bwd", 1, 256, 0, 2, 2),                          # a non-positive size
           hip.attn128_plan("fwd", 1 << 15, 1 << 18, 64, 16, 16),             # 2^30 blocks
           hip.attn128_plan("bwd", 1 << 15, 1 << 17, 1 << 16, 16, 16),        # 2^29 blocks of each role: 2^30 together
           hip.attn128_plan("fwd", 1, 256, 256, 2, 2, addrs={"k": 4104}),     # a base off the 16-byte grid
           hip.attn128_plan("bwd", 1, 256, 256, 2, 2, strides={"dq": (256 * 260, 260, 128)}),
           hip.attn128_plan("fwd", 1, 256, 256, 2, 2, addrs={"q": 0})]        # a null operand
    assert all(p["err"] != 0 and p["launches"] == [] for p in bad)
    assert hip.attn128_plan("fwd", 1 << 15, 1 << 17, 1 << 16, 16, 16)["err"] == 0    # 2^29 blocks
