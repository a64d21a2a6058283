"""Chunked prefill at head dim 128 on the host: the switch, read at every call; host tensors; the plan."""
import warnings

import pytest
import torch

from learning_jax_sharding_amd.ops import hip, kernels as K


@pytest.mark.parametrize("switch", [None, "0", "1"])
def test_switch_decides_chunk_at_128_and_host_tensors_run_the_reference_silently(monkeypatch, switch):
    monkeypatch.setenv("LJS_ATTN_D128", switch) if switch else monkeypatch.delenv("LJS_ATTN_D128", raising=False)
    for op in ("chunk", "attn_chunk", "attn_chunk_q8"):
        assert hip.cache_op_supported(op, 128) is (switch == "1") and hip.cache_op_supported(op, 64)
    g = torch.Generator().manual_seed(3)
    q, kc, vc = (torch.randn(2, n, h, 128, generator=g).to(torch.bfloat16) for n, h in ((5, 4), (16, 2), (16, 2)))
    lens = torch.tensor([0, 9], dtype=torch.int32)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = K.cache_attend(q, (kc, vc), lens, 128 ** -0.5, "chunk")
    assert all(torch.equal(a, b) for a, b in zip(got, K.attn_chunk_reference(q, kc, vc, lens, 128 ** -0.5)))
    plans = [hip.plan_chunk(b, t, 8, 2, cus=256) for b, t in ((64, 33), (4, 33), (4, 16))]     # (it does not know the head dim)
    assert plans == [(128, (2, 2, 64)), (64, (3, 2, 4)), (64, (1, 2, 4))]    # two tiles; idle CUs otherwise; one 64-row tile
