"""Multi-token cached steps (``extend=True``) and greedy speculative decoding on host devices.

* ``attn_extend_reference`` / ``attn_extend_q8_reference`` are the stacked ``attn_decode*_reference`` results, bit for bit,
  and ``kernels.attn_extend*`` run them silently on the host;
* a small ``TransformerLM`` (the decode tests' model): a prefill of ragged prompts followed by ONE ``extend=True`` call
  on ``T`` tokens against the uncached causal forward on the same tokens at the same positions, and against
  ``T`` single steps, by the decode tests' rule with the single steps as the other equally valid evaluation:

      max|C - R| <= 4 max|A - R| + 2^-23 max|R|

  ``R``: the float32 uncached logits, ``A``: the cached single steps, ``C``: the extend call (both in the tested dtype);
* every ``ValueError`` of the new options, before any launch;
* ``generate(draft=...)`` against plain ``generate`` and the uncached argmax loop, with the target as its own draft
  (every round then emits ``k + 1`` tokens) and with a differently seeded draft.
"""
import numpy as np
import pytest
import torch

import test_decode as TD

BF16, F32 = torch.bfloat16, torch.float32
LM, PLENS, SCALE = TD.LM, TD.PLENS, TD.SCALE


# ----------------------------------------------------------------------------- 1. the references
@pytest.mark.parametrize("H,Hkv", [(4, 4), (8, 2), (16, 1)])
def test_extend_references_are_stacked_decode_references(H, Hkv):
    from learning_jax_sharding_amd.ops import kernels as K
    B, T, cap = 4, 5, 48
    gen = torch.Generator().manual_seed(3)
    q = torch.randn(B, T, H, 64, generator=gen).to(BF16)
    kc = torch.randn(B, cap, Hkv, 64, generator=gen).to(BF16)
    vc = torch.randn(B, cap, Hkv, 64, generator=gen).to(BF16)
    lens = torch.tensor([0, 7, cap - T, cap - 1], dtype=torch.int32)          # the last one clamps
    for b, n in enumerate(lens.tolist()):                                      # dead rows hold NaN
        kc[b, n + T:] = float("nan")
        vc[b, n + T:] = float("nan")
    o, lse = K.attn_extend_reference(q, kc, vc, lens, SCALE)
    assert o.shape == (B, T, H, 64) and o.dtype == BF16 and lse.shape == (B, H, T) and lse.dtype == F32
    assert torch.isfinite(o.float()).all()
    for t in range(T):
        wo, wl = K.attn_decode_reference(q[:, t:t + 1], kc, vc, lens, SCALE, extra=t + 1)
        assert torch.equal(o[:, t:t + 1], wo) and torch.equal(lse[..., t:t + 1], wl), t
    got = K.attn_extend(q, kc, vc, lens, SCALE)                                # host tensors: the reference, silently
    assert torch.equal(got[0], o) and torch.equal(got[1], lse)
    # the MX-fp8 form: quantise the live rows, poison the dead bytes and scales with the formats' NaNs
    kq, ke = K._mx_bytes(torch.nan_to_num(kc.float()).to(BF16))
    vq, ve = K._mx_bytes(torch.nan_to_num(vc.float()).to(BF16))
    for b, n in enumerate(lens.tolist()):
        for buf, fill in ((kq, 0x7F), (vq, 0xFF), (ke, 0xFF), (ve, 0xFF)):
            buf[b, n + T:] = fill
    o8, l8 = K.attn_extend_q8_reference(q, kq, vq, ke, ve, lens, SCALE)
    assert o8.shape == (B, T, H, 64) and l8.shape == (B, H, T) and torch.isfinite(o8.float()).all()
    for t in range(T):
        wo, wl = K.attn_decode_q8_reference(q[:, t:t + 1], kq, vq, ke, ve, lens, SCALE, extra=t + 1)
        assert torch.equal(o8[:, t:t + 1], wo) and torch.equal(l8[..., t:t + 1], wl), t
    got = K.attn_extend_q8(q, kq, vq, ke, ve, lens, SCALE)
    assert torch.equal(got[0], o8) and torch.equal(got[1], l8)


def test_lens_add_delta():
    from learning_jax_sharding_amd.ops import kernels as K
    lens = torch.tensor([3, 9, 0], dtype=torch.int32)
    assert K.lens_add_delta(lens, torch.tensor([2, -4, 0], dtype=torch.int32)) is lens
    assert lens.tolist() == [5, 5, 0]
    with pytest.raises(ValueError, match="delta"):
        K.lens_add_delta(lens, torch.tensor([1, 1, 1]))


# ----------------------------------------------------------------------------- 2. the model
def extend_rows(lm, params, tok, plens, T, put, dtype, cache_sharding=None, max_len=None):
    """Cached logits of the real positions: the ragged prefill, then ONE extend call on ``tok[b, plens[b] : plens[b] + T]``."""
    from learning_jax_sharding_amd.models import TransformerLM
    model = TransformerLM(**lm, dtype=dtype)
    B, P = tok.shape[0], max(plens)
    cache = model.init_cache(B, max_len or (P + T), sharding=cache_sharding)
    logits, cache = model.apply({"params": params}, put(tok[:, :P].numpy()), cache=cache, prompt_lens=plens)
    lp = logits.to_torch().double()
    x = torch.stack([tok[b, n:n + T] for b, n in enumerate(plens)])
    lg, cache = model.apply({"params": params}, put(x.numpy()), cache=cache, extend=True)
    assert tuple(lg.shape) == (B, T, lm["vocab_size"])
    assert cache.lens.to_torch().tolist() == [n + T for n in plens]
    lg = lg.to_torch().double()
    return [torch.cat([lp[b, :plens[b]], lg[b]]) for b in range(B)], cache


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("pos", ["rope", "table"])
def test_extend_matches_single_steps_and_uncached_forward(host_devices, pos, dtype):
    host_devices(1)
    T = 6
    lm = dict(LM) if pos == "rope" else dict(LM, rope_theta=None, max_len=32)
    tok = TD.tokens()
    params, put = TD.lm_params(lm, tok)
    R = TD.uncached_logits(lm, params, tok, put, F32)
    steps, _ = TD.teacher_forced(lm, params, tok, PLENS, T, put, dtype=dtype, max_len=32)
    A = torch.zeros_like(R)
    for b, n in enumerate(PLENS):
        A[b, :n + T] = steps[b]
    rows, cache = extend_rows(lm, params, tok, PLENS, T, put, dtype, max_len=32)
    TD.rule_check(f"extend host {pos} {dtype}", rows, R, A, PLENS, T)
    # the prompt's logits are the prefill's own; one position with extend=True is a single step, bit for bit
    for b, n in enumerate(PLENS):
        assert torch.equal(rows[b][:n], steps[b][:n]), b
    rows1, _ = extend_rows(lm, params, tok, PLENS, 1, put, dtype, max_len=32)
    for b, n in enumerate(PLENS):
        assert torch.equal(rows1[b], steps[b][:n + 1]), b
    # a second extend call continues where the first stopped
    from learning_jax_sharding_amd.models import TransformerLM
    model = TransformerLM(**lm, dtype=dtype)
    x = torch.stack([tok[b, n + T:n + T + 2] for b, n in enumerate(PLENS)])
    lg, cache = model.apply({"params": params}, put(x.numpy()), cache=cache, extend=True)
    assert cache.lens.to_torch().tolist() == [n + T + 2 for n in PLENS]
    more, _ = TD.teacher_forced(lm, params, tok, PLENS, T + 2, put, dtype=dtype, max_len=32)
    A2 = torch.zeros_like(R)
    for b, n in enumerate(PLENS):
        A2[b, :n + T + 2] = more[b]
    both = [torch.cat([rows[b], lg.to_torch().double()[b]]) for b in range(len(PLENS))]
    TD.rule_check(f"extend twice host {pos} {dtype}", both, R, A2, PLENS, T + 2)


# ----------------------------------------------------------------------------- 3. errors
def test_extend_errors(host_devices):
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd.models import MultiHeadAttention, TransformerLayer, TransformerLM, generate
    from learning_jax_sharding_amd.ops import core
    host_devices(1)
    tok = TD.tokens(B=2, S=12)
    params, put = TD.lm_params(LM, tok)
    ids = put(tok.numpy())
    model = TransformerLM(**LM)
    cache = model.init_cache(2, 96)
    with pytest.raises(ValueError, match="extend"):
        model.apply({"params": params}, ids, extend=True)
    with pytest.raises(ValueError, match="prompt_lens"):
        model.apply({"params": params}, ids, cache=cache, prompt_lens=[3, 4], extend=True)
    with pytest.raises(ValueError, match="extend.*64"):
        model.apply({"params": params}, put(TD.tokens(B=2, S=65).numpy()), cache=cache, extend=True)
    assert cache.lens.to_torch().tolist() == [0, 0]
    x = ljs.random.normal(ljs.random.PRNGKey(0), (2, 4, 128))
    attn = MultiHeadAttention(128, heads=4, dim_head=64, kv_heads=2, causal=True, rope_theta=10000.0)
    ap = attn.init(ljs.random.PRNGKey(1), x)["params"]
    with pytest.raises(ValueError, match="extend"):
        attn.apply({"params": ap}, x, extend=True)
    layer = TransformerLayer(128, heads=4, dim_head=64, ff_dim=256, causal=True, norm="rms")
    lp = layer.init(ljs.random.PRNGKey(1), x)["params"]
    with pytest.raises(ValueError, match="extend"):
        layer.apply({"params": lp}, x, extend=True)
    q = ljs.random.normal(ljs.random.PRNGKey(2), (2, 65, 4, 64), dtype=BF16)
    kv = ljs.random.normal(ljs.random.PRNGKey(3), (2, 65, 2, 64), dtype=BF16)
    with pytest.raises(ValueError, match="extend"):
        core.cached_attention(q, kv, kv, cache.layer(0)[:2], cache.lens, extend=True)
    with pytest.raises(ValueError, match="one new position"):
        core.cached_attention(q, kv, kv, cache.layer(0)[:2], cache.lens)
    # generate with a draft
    draft = (model, params)
    small = TransformerLM(**dict(LM, vocab_size=256))
    with pytest.raises(ValueError, match="draft"):
        generate(model, params, ids, 4, draft=draft, key=ljs.random.PRNGKey(0))
    with pytest.raises(ValueError, match="draft"):
        generate(model, params, ids, 4, draft=draft, eos_id=3, pad_id=0)
    with pytest.raises(ValueError, match="vocabulary"):
        generate(model, params, ids, 4, draft=(small, params))
    with pytest.raises(ValueError, match="draft_tokens"):
        generate(model, params, ids, 4, draft=draft, draft_tokens=0)
    with pytest.raises(ValueError, match="draft_tokens"):
        generate(model, params, ids, 4, draft=draft, draft_tokens=64)
    generate(model, params, ids, 2, draft=draft, draft_tokens=2, max_len=16)          # 12 + 2 + 2 fits
    with pytest.raises(ValueError, match="max_len"):
        generate(model, params, ids, 3, draft=draft, draft_tokens=2, max_len=16)      # 12 + 3 + 2 does not


# ----------------------------------------------------------------------------- 4. speculative generate
# The precondition is test_decode's, on the reference alone: at TD.GEN_SEED the float32 uncached model's top-2 logit
# gap is at least 1e-3 max|logit| at EVERY emitted position (reference_generate takes the minimum over all of them).
# The decode rule bounds a float32 cached evaluation's distance from that reference by 4 max|A - R| + 2^-23 max|R|, a
# few float32 roundings of max|logit| (the rule's figures printed above: about 1e-6 max|R|), a thousand times
# below that gap, so no argmax can flip, whether a token comes from a single step or from an extend call.
NEW = 9                       # the prefill's token, then rounds of k + 1 = 4: (NEW - 1) % 4 == 0


@pytest.fixture(scope="module")
def spec_reference():
    return {}


def _reference(cache, host_devices):
    if not cache:
        host_devices(1)
        tok = TD.tokens(seed=TD.GEN_SEED)
        params, put = TD.lm_params(LM, tok)
        want, gap = TD.reference_generate(LM, params, tok, PLENS, NEW, put)
        print(f"extend-figures generate reference top-2 gap / max|logit| = {gap:.3e}")
        cache.update(tok=tok, params=params, put=put, want=want, gap=gap)
    return cache


@pytest.mark.parametrize("which", ["self", "other"])
def test_speculative_generate_matches_plain(host_devices, spec_reference, which):
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd.models import TransformerLM, generate
    ref = _reference(spec_reference, host_devices)
    host_devices(1)
    tok, params, put, want = ref["tok"], ref["params"], ref["put"], ref["want"]
    assert ref["gap"] >= 1e-3, ref["gap"]        # the precondition, on the reference alone, every position counted
    model = TransformerLM(**LM, dtype=F32)
    ids = put(tok[:, :max(PLENS)].numpy())
    plain = generate(model, params, ids, NEW, prompt_lens=PLENS)
    assert torch.equal(plain, want)
    k = 3
    if which == "self":
        draft = (model, params)
    else:
        dlm = dict(LM, layers=1)
        draft = (TransformerLM(**dlm, dtype=F32), TransformerLM(**dlm).init(ljs.random.PRNGKey(7), ids)["params"])
    got, lens, mean = generate(model, params, ids, NEW, prompt_lens=PLENS, draft=draft, draft_tokens=k, return_lens=True)
    print(f"extend-figures speculative {which}: mean tokens per round {mean:.3f}")
    assert got.shape == (4, NEW) and got.dtype == torch.int64 and lens.tolist() == [NEW] * 4
    assert torch.equal(got, want), (got, want)
    if which == "self":
        assert mean == k + 1, mean               # every round emitted k + 1 tokens
    else:
        assert 1.0 <= mean <= k + 1, mean
    # lengths that the rounds do not divide, a round per poll, and a single new token
    for new, kk, poll in ((NEW - 2, 3, 1), (NEW, 1, 0), (1, 3, 16)):
        got = generate(model, params, ids, new, prompt_lens=PLENS, draft=draft, draft_tokens=kk, stop_poll=poll)
        assert torch.equal(got, want[:, :new]), (new, kk, poll)


def test_speculative_generate_two_devices(host_devices, spec_reference):
    from learning_jax_sharding_amd.models import TransformerLM, generate
    lm = dict(LM, vocab_size=256)
    tok = TD.tokens(vocab=256, seed=TD.GEN_SEED)
    host_devices(1)
    params1, put1 = TD.lm_params(lm, tok)
    want, gap = TD.reference_generate(lm, params1, tok, PLENS, 6, put1)
    assert gap >= 1e-3, gap
    host_devices(2)
    params, put, cache_sh, Ctx = TD.mesh_setup((2, 1), lm, tok)
    model = TransformerLM(**lm, dtype=F32)
    with Ctx():
        got = generate(model, params, put(tok[:, :max(PLENS)].numpy()), 6, prompt_lens=PLENS, cache_sharding=cache_sh,
                       draft=(model, params), draft_tokens=2)
    assert torch.equal(got, want), (got, want)
