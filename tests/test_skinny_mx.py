"""The MX-fp8 skinny GEMM's host side (csrc/kernels/skinny_mx.hip through ops/hip.py, ops/linear.py and
models.generate), without a GPU: the torch reference against float64, the plan's purity and monotonicities,
``generate(weight_quant=...)`` argument errors, and a host decode step under the mode against the same step on
dequantised weights."""
import itertools

import pytest
import torch

from test_decode import LM, lm_params, tokens

BF16, F32 = torch.bfloat16, torch.float32


def _mx(wt):
    """(codes, scale bytes, dequantised f32) of ``fp8.quantize_mx_ref`` of the bf16 ``wt`` [N][K]."""
    from learning_jax_sharding_amd.ops import fp8
    qv, ex = fp8.quantize_mx_ref(wt)
    return qv.view(torch.uint8), (ex + 127).to(torch.uint8), fp8.dequantize_mx_ref(qv, ex)


@pytest.mark.parametrize("epi", ["plain", "bias-relu", "res"])
def test_reference_against_float64(epi):
    """Normal data; the bound is the rounding of a bf16 output: one ulp of the rounded float64 value."""
    from learning_jax_sharding_amd.ops.kernels import skinny_mx_reference
    M, N, K = 5, 24, 384
    gen = torch.Generator().manual_seed(3)
    x = torch.randn((M, K), generator=gen).to(BF16)
    q, s, w_hat = _mx(torch.randn((N, K), generator=gen).to(BF16))
    assert torch.equal(w_hat, w_hat.to(BF16).float())                       # exact bf16 values
    bias = torch.randn((N,), generator=gen) if epi == "bias-relu" else None
    res = torch.randn((M, N), generator=gen).to(BF16) if epi == "res" else None
    got = skinny_mx_reference(x, q, s, bias, epi == "bias-relu", res)
    want = x.double() @ w_hat.double().t()
    if bias is not None:
        want = (want + bias.double()).clamp_min(0.0)
    if res is not None:   # exactly the stated double rounding of the reference's own product, checked below
        y = skinny_mx_reference(x, q, s)
        assert torch.equal(got, (y.float() + res.float()).to(BF16))
        got = y
    rounded = want.to(BF16).double()
    ulp = 2.0 ** (torch.floor(torch.log2(rounded.abs().clamp_min(2.0 ** -126))) - 7)
    assert got.dtype == BF16 and ((got.double() - rounded).abs() <= ulp).all()


def test_plan_properties():
    from learning_jax_sharding_amd.ops import hip
    hip.lib()
    NS, KS, CUS = (16, 24, 256, 640, 3584, 32768), (128, 384, 640, 1792, 4096), (64, 256)
    seen = {a: hip.skinny_mx_plan(*a) for a in itertools.product((1, 8, 16), NS, KS, CUS)}
    hip.set_skinny_waves(4)
    try:
        for args, want in seen.items():          # pure: a forced wave count and a second pass change nothing
            assert hip.skinny_mx_plan(*args) == want, args
    finally:
        hip.set_skinny_waves(None)
    for (M, N, K, cus), (waves, blocks) in seen.items():
        assert waves in hip.SKINNY_WAVES and waves <= K // 128 and blocks == -(-N // 16), (M, N, K, cus, waves, blocks)
        assert (waves, blocks) == seen[(1, N, K, cus)]            # M does not enter
    for K, cus in itertools.product(KS, CUS):    # more columns never get more waves
        ws = [seen[(1, N, K, cus)][0] for N in NS]
        assert ws == sorted(ws, reverse=True), (K, cus, ws)
    for N, cus in itertools.product(NS, CUS):    # a longer K never fewer
        ws = [seen[(1, N, K, cus)][0] for K in KS]
        assert ws == sorted(ws), (N, cus, ws)
    for N, K in itertools.product(NS, KS):       # nor more CUs
        assert seen[(1, N, K, 64)][0] <= seen[(1, N, K, 256)][0], (N, K)
    assert hip.skinny_mx_plan(8, 640, 1792) == (8, 40) and hip.skinny_mx_plan(8, 32768, 640) == (1, 2048)
    for bad in ((0, 64, 128), (17, 64, 128), (8, 64, 96), (8, 20, 128)):
        with pytest.raises(ValueError):
            hip.skinny_mx_plan(*bad)
        assert not hip.skinny_mx_supported(*bad, 128, 128, 4, 64, BF16)
    assert hip.skinny_mx_supported(8, 64, 128, 128, 128, 4, 64, BF16)
    assert not hip.skinny_mx_supported(8, 64, 128, 128, 128, 4, 64, BF16, s_addr=2)


def test_generate_errors_and_host_step(host_devices):
    """A host decode step under the mode equals the step with every eligible weight (2-D, K % 128 == 0, N % 64 == 0:
    all but the head, N = 257) replaced by its dequantised values, and differs from the unquantised step."""
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd.models import TransformerLM, generate
    from learning_jax_sharding_amd.ops import linear as L
    host_devices(1)
    tok = tokens()
    params, put = lm_params(LM, tok)
    ids = put(tok[:, :9].numpy())
    with pytest.raises(ValueError, match="weight_quant must be"):
        generate(TransformerLM(**LM), params, ids, 4, weight_quant="int4")
    with pytest.raises(ValueError, match="draft"):
        generate(TransformerLM(**LM), params, ids, 4, weight_quant="mxfp8", draft=(TransformerLM(**LM), params))
    count = [0]

    def deq(a):
        t = a.to_torch()
        if t.dim() != 2 or t.shape[0] % 128 or t.shape[1] % 64:
            return a
        count[0] += 1
        return put(_mx(t.to(BF16).t().contiguous())[2].t().contiguous().numpy())

    params_hat = ljs.tree_map(deq, params)
    assert count[0] == 7 * LM["layers"], count                # q, k, v, out, gate, up, down
    model = TransformerLM(**LM, dtype=BF16)

    def step(p, mode):       # (the cache rows of every run come from the same unquantised prefill of `params`)
        cache = model.init_cache(4, 32)
        with torch.no_grad():
            _, cache = model.apply({"params": params}, ids, cache=cache, prompt_lens=[5, 9, 7, 6])
            with L.weight_quant(mode):
                return model.apply({"params": p}, put(tok[:, 9:10].numpy()), cache=cache)[0].to_torch().float()

    got, want, plain = step(params, "mxfp8"), step(params_hat, None), step(params, None)
    assert torch.equal(got, want) and not torch.equal(got, plain)
