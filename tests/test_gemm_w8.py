"""The W8A16 tile GEMM's host side (csrc/kernels/gemm_w8.hip through ops/hip.py, ops/linear.py and models.generate),
without a GPU: the "mxfp8-all" mode, ``generate``'s argument rules, a host prefill under the mode against the reference
on the quantised weights, and the plan."""
import itertools

import pytest
import torch

from test_decode import LM, lm_params, tokens
from test_skinny_mx import _mx

BF16 = torch.bfloat16


def test_generate_argument_rules(host_devices):
    from learning_jax_sharding_amd.models import TransformerLM, generate
    host_devices(1)
    tok = tokens()
    params, put = lm_params(LM, tok)
    ids = put(tok[:, :9].numpy())
    draft = (TransformerLM(**LM), params)
    with pytest.raises(ValueError, match="draft"):
        generate(TransformerLM(**LM), params, ids, 4, weight_quant="mxfp8", draft=draft)
    with pytest.raises(ValueError, match="weight_quant must be"):
        generate(TransformerLM(**LM), params, ids, 4, weight_quant="int4", draft=draft)
    # "mxfp8-all" with a draft passes validation (and, the draft being the target, every round accepts everything)
    spec = generate(TransformerLM(**LM), params, ids, 4, weight_quant="mxfp8-all", draft=draft, draft_tokens=2)
    assert torch.equal(spec, generate(TransformerLM(**LM), params, ids, 4, weight_quant="mxfp8-all"))


def test_host_prefill_reads_the_quantised_weights(host_devices):
    """A dense call of 36 rows: under "mxfp8-all" it is skinny_mx_reference on quantize_mx_ref of the bf16 transposed
    weight; under "mxfp8" it is the default call."""
    from learning_jax_sharding_amd.ops import kernels as K, linear as L
    gen = torch.Generator().manual_seed(5)
    x = torch.randn((4, 9, 128), generator=gen)
    w, b = torch.randn((128, 192), generator=gen), torch.randn((192,), generator=gen)
    with torch.no_grad():
        plain = K.linear(x, [w], b, BF16, relu=True)[0]
        with L.weight_quant("mxfp8"):
            assert torch.equal(K.linear(x, [w], b, BF16, relu=True)[0], plain)
        with L.weight_quant("mxfp8-all"):
            got = K.linear(x, [w], b, BF16, relu=True)[0]
    q, s, _ = _mx(w.to(BF16).t().contiguous())
    want = K.skinny_mx_reference(x.reshape(-1, 128), q, s, b, True).view(4, 9, 192)
    assert torch.equal(got, want) and not torch.equal(got, plain)
    with L.weight_quant(L.WEIGHT_QUANT_MXFP8_ALL):            # grad enabled: the default call
        assert torch.equal(K.linear(x, [w], b, BF16, relu=True)[0], plain)
    with pytest.raises(ValueError), L.weight_quant("int4"):
        pass


def test_plan_is_pure_and_picks_64_rows_for_small_m():
    from learning_jax_sharding_amd.ops import hip
    hip.lib()
    seen = {a: hip.gemm_w8_plan(*a) for a in itertools.product((1, 17, 64, 65, 512, 16384), (8, 136, 4096), (128, 1280),
                                                               (64, 256))}
    hip.set_gemm_w8_rows(128)
    try:
        assert all(hip.gemm_w8_plan(*a) == want for a, want in seen.items())      # a forced row count does not enter
    finally:
        hip.set_gemm_w8_rows(None)
    for (M, N, K, cus), (rows, blocks) in seen.items():
        small = M <= 64 or -(-M // 128) * -(-N // 128) < cus
        assert rows == (64 if small else 128) and blocks == -(-M // rows) * -(-N // 128), (M, N, K, cus, rows, blocks)
    assert hip.gemm_w8_plan(16384, 4096, 4096) == (128, 4096) and hip.gemm_w8_plan(72, 1536, 640) == (64, 24)
    for bad in ((0, 64, 128), (8, 64, 192), (8, 20, 128)):
        with pytest.raises(ValueError):
            hip.gemm_w8_plan(*bad)
        assert not hip.gemm_w8_supported(*bad, 256, 256, 8, 64, BF16)
    assert hip.gemm_w8_supported(4096, 64, 128, 128, 128, 4, 64, BF16)
    assert not hip.gemm_w8_supported(4096, 64, 128, 128, 128, 4, 64, BF16, q_addr=8)
    with pytest.raises(ValueError):
        hip.set_gemm_w8_rows(32)
