"""Chunked prefill (``extend="chunk"``, ``generate(prefill_chunk=)``) on host devices."""
import numpy as np
import pytest
import torch

import attn_oracle as AO
from test_decode import GEN_SEED, LM, PLENS, lm_params, tokens

BF16, F32 = torch.bfloat16, torch.float32
SCALE = 0.125


def _inputs(kind, B, H, Hkv, T, cap):
    q, k, v, _ = AO.inputs(kind, B, H, T, cap, SCALE)
    return q, k[:, :, :Hkv].contiguous(), v[:, :, :Hkv].contiguous()


@pytest.mark.parametrize("kind", AO.KINDS)
@pytest.mark.parametrize("H,Hkv", [(4, 4), (6, 2)])
def test_chunk_reference_matches_oracle(kind, H, Hkv):
    from learning_jax_sharding_amd.ops import kernels as K
    B, T, cap, lens = 4, 9, 96, [-3, 0, 40, 90]           # no key for some rows; the last one clamps at cap
    q, k, v = _inputs(kind, B, H, Hkv, T, cap)
    for b, n0 in enumerate(lens):                         # dead rows hold NaN
        k[b, max(n0 + T, 0):] = float("nan")
        v[b, max(n0 + T, 0):] = float("nan")
    lt = torch.tensor(lens, dtype=torch.int32)
    o, lse = K.attn_chunk_reference(q, k, v, lt, SCALE)
    assert o.shape == (B, T, H, 64) and o.dtype == BF16 and lse.shape == (B, H, T) and lse.dtype == F32
    got = K.attn_chunk(q, k, v, lt, SCALE)                # host tensors: the reference, silently
    assert torch.equal(got[0], o) and torch.equal(got[1], lse)
    for b, n0 in enumerate(lens):
        n = max(min(n0 + T, cap), 1)
        qb = q[b:b + 1]
        kb, vb = (torch.nan_to_num(x[b:b + 1, :n].float()).to(BF16).repeat_interleave(H // Hkv, 2) for x in (k, v))
        want_o, want_lse = AO.forward(qb, kb, vb, SCALE, causal=True, q_offset=n0)
        model_o, _ = AO.forward(qb, kb, vb, SCALE, causal=True, q_offset=n0, rounded=True)
        AO.check(f"chunk ref {kind} b{b} o", o[b:b + 1], want_o, model_o)
        AO.check_lse(lse[b:b + 1], want_lse, AO.lse2_f32(qb, kb, SCALE, causal=True, q_offset=n0), name=f"b{b} lse")


@pytest.mark.parametrize("T", [1, 3, 8])
def test_chunk_reference_is_extend_reference_to_one_ulp(T):
    """One masked einsum against ``T`` stacked single-query calls: the same recipe in two summation orders."""
    from learning_jax_sharding_amd.ops import kernels as K
    B, H, Hkv, cap = 3, 8, 2, 48
    q, k, v = _inputs("plain", B, H, Hkv, T, cap)
    lt = torch.tensor([0, 7, cap - 2], dtype=torch.int32)
    (o, lse), (wo, wl) = K.attn_chunk_reference(q, k, v, lt, SCALE), K.attn_extend_reference(q, k, v, lt, SCALE)
    ulp = 2.0 ** -7 * wo.float().abs()                    # one bf16 ulp of the value (8 significand bits)
    assert ((o.float() - wo.float()).abs() <= ulp).all()
    # two f32 sums of at most 48 terms: each within 48 * 2^-24 of l, which log2 turns into log2(e) times that
    assert torch.allclose(lse, wl, rtol=2.0 ** -22, atol=2 * 48 * 2.0 ** -24 * AO.LOG2E)
    # the MX-fp8 form is the bf16 form on the dequantised cache, dead bytes and scales poisoned or not
    kq, ke = K._mx_bytes(k)
    vq, ve = K._mx_bytes(v)
    deq = K.attn_chunk_reference(q, K.mx_cache_dequant(kq, ke), K.mx_cache_dequant(vq, ve), lt, SCALE)
    for b, n0 in enumerate(lt.tolist()):
        for buf, fill in ((kq, 0x7F), (vq, 0xFF), (ke, 0xFF), (ve, 0x00)):
            buf[b, min(n0 + T, cap):] = fill
    for got in (K.attn_chunk_q8_reference(q, kq, vq, ke, ve, lt, SCALE), K.attn_chunk_q8(q, kq, vq, ke, ve, lt, SCALE)):
        assert torch.equal(got[0], deq[0]) and torch.equal(got[1], deq[1])


def test_chunk_reference_of_one_position_is_the_decode_reference():
    """``T = 1``: the chunk references are the decode references with ``extra = 1``, bit for bit and for both cache kinds;
    a sequence without a key (``lens = -1``) and one at capacity included."""
    from learning_jax_sharding_amd.ops import kernels as K
    B, H, Hkv, cap = 4, 8, 2, 48
    q = _inputs("plain", B, H, Hkv, 1, cap)[0]
    kf, vf = (torch.randn(B, cap, Hkv, 64, generator=torch.Generator().manual_seed(s)).to(BF16) for s in (1, 2))
    lt = torch.tensor([-1, 0, 17, cap], dtype=torch.int32)
    got, want = K.attn_chunk_reference(q, kf, vf, lt, SCALE), K.attn_decode_reference(q, kf, vf, lt, SCALE, extra=1)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert (got[0][0] == 0).all() and torch.isinf(got[1][0]).all() and torch.isfinite(got[1][1:]).all()
    cache = (*K._mx_bytes(kf), *K._mx_bytes(vf))
    cache = (cache[0], cache[2], cache[1], cache[3])      # (kc, vc, kcs, vcs)
    got, want = K.attn_chunk_q8_reference(q, *cache, lt, SCALE), K.attn_decode_q8_reference(q, *cache, lt, SCALE, extra=1)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert (got[0][0] == 0).all() and torch.isinf(got[1][0]).all() and torch.isfinite(got[1][1:]).all()


@pytest.mark.parametrize("shape,cus,want", [
    ((1, 1, 8, 8), 256, (64, (1, 8, 1))),           # a lone row
    ((4, 33, 8, 2), 256, (64, (3, 2, 4))),          # 132 rows: 16 blocks of 128 rows would leave CUs idle
    ((64, 33, 8, 2), 256, (128, (2, 2, 64))),       # 256 blocks of 128 rows fill the chip
    ((64, 16, 8, 2), 256, (64, (1, 2, 64))),        # 64 rows fit one 64-row tile however many blocks there are
    ((8, 2048, 8, 8), 256, (128, (16, 8, 8))),
    ((8, 2048, 6, 2), 8, (128, (48, 2, 8))),        # G = 3
])
def test_plan_chunk(shape, cus, want):
    from learning_jax_sharding_amd.ops import hip
    assert hip.plan_chunk(*shape, cus=cus) == want
    with pytest.raises(ValueError):
        hip.plan_chunk(1, 1, 6, 4, cus=cus)


def test_chunked_lm_and_errors(host_devices):
    """65 positions with ``extend="chunk"`` (``extend=True`` raises there), and every new ``ValueError``."""
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd.models import TransformerLM, generate
    from learning_jax_sharding_amd.ops import core
    host_devices(1)
    tok = tokens(B=2, S=70)
    params, put = lm_params(LM, tok)
    model = TransformerLM(**LM, dtype=BF16)
    ids = put(tok[:, :65].numpy())
    cache = model.init_cache(2, 80)
    with pytest.raises(ValueError, match="at most 64"):
        model.apply({"params": params}, ids, cache=cache, extend=True)
    logits, cache = model.apply({"params": params}, ids, cache=cache, extend="chunk")
    assert logits.shape == (2, 65, 257) and torch.isfinite(logits.to_torch().float()).all()
    assert cache.lens.to_torch().tolist() == [65, 65]
    with pytest.raises(ValueError, match="prompt_lens"):
        model.apply({"params": params}, ids, cache=cache, extend="chunk", prompt_lens=[65, 65])
    with pytest.raises(ValueError, match="do not fit"):
        model.apply({"params": params}, put(tok[:, :70].numpy()), cache=model.init_cache(2, 69), extend="chunk")
    layer = cache.layer(0)
    z = lambda T, H: ljs.device_put(np.zeros((2, T, H, 64), dtype=np.float32))   # noqa: E731
    with pytest.raises(ValueError, match="False, True or 'chunk'"):
        core.cached_attention(z(3, 4), z(3, 2), z(3, 2), layer[:2], layer[2], extend="chunks")
    with pytest.raises(ValueError, match="capacity"):
        core.cached_attention(z(81, 4), z(81, 2), z(81, 2), layer[:2], layer[2], extend="chunk")
    gids = put(tok[:, :9].numpy())
    for bad in (0, -4, 2.5):
        with pytest.raises(ValueError, match="prefill_chunk"):
            generate(model, params, gids, 4, prefill_chunk=bad)
    with pytest.raises(ValueError, match="prefill_chunk"):
        generate(model, params, gids, 4, prefill_chunk=4, draft=(model, params))


def test_generate_prefill_chunk_matches_single_prefill(host_devices):
    """Ragged prompts fed in chunks of 4 (each sequence's first token comes from another chunk) in float32, where the
    two prefills differ by summation order only and the reference's top-2 gaps (test_decode.py) decide the tokens."""
    from learning_jax_sharding_amd.models import TransformerLM, generate
    host_devices(1)
    tok = tokens(seed=GEN_SEED)
    params, put = lm_params(LM, tok)
    model = TransformerLM(**LM, dtype=F32)
    ids = put(tok[:, :max(PLENS)].numpy())
    want = generate(model, params, ids, 8, prompt_lens=PLENS)
    for n in (4, 9, 100):
        got, lens = generate(model, params, ids, 8, prompt_lens=PLENS, prefill_chunk=n, return_lens=True)
        assert torch.equal(got, want) and lens.tolist() == [8] * 4, (n, got, want)
