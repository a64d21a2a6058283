"""The MX-fp8 KV cache on host devices: the two torch references that state its semantics, the cache object and
``generate(..., cache_quant="mxfp8")``.

* ``kv_append_q8_reference`` stores ``fp8.quantize_mx_ref`` of ``rope_reference``'s rows (v: of the rows as they are)
  at the right rows, bytes and scale bytes compared as uint8; rows past ``max_len`` are dropped (guard bytes
  and guard scales untouched); the host-base mode with T = 5;
* ``attn_decode_q8_reference`` is ``attn_decode_reference`` on the dequantised cache, bit for bit, whatever the
  dead rows' bytes and scale bytes hold;
* a quantised ``KVCache``: 66 / 128 of the bf16 cache's bytes, the pytree round trip with its scales, the
  errors; ``generate`` on one host device and on two with the batch sharded.
"""
import pytest
import torch

from test_decode import LM, PLENS, lm_params, mesh_setup, tokens

BF16, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
SCALE = 0.125
FILL = 0xFF


def _K():
    from learning_jax_sharding_amd.ops import kernels as K
    return K


def _mx(x):
    """(bytes, scale bytes) of rows ``x[..., 64]`` by ``quantize_mx_ref``, in the stored encoding."""
    from learning_jax_sharding_amd.ops.fp8 import quantize_mx_ref
    q, ex = quantize_mx_ref(x)
    return q.view(U8), (ex + 127).to(U8)


def _inputs(B, T, H, Hkv, seed):
    gen = torch.Generator().manual_seed(seed)
    mk = lambda h: torch.randn(B, T, h, 64, generator=gen).to(BF16)   # noqa: E731
    return mk(H), mk(Hkv), mk(Hkv)


def _filled(B, cap, Hkv, guard=0):
    mk = lambda w: torch.full((B, cap + guard, Hkv, w), FILL, dtype=U8)   # noqa: E731
    return mk(64), mk(64), mk(2), mk(2)


# ----------------------------------------------------------------------------- the references
def test_append_reference_is_rope_then_quantize():
    K = _K()
    B, T, H, Hkv, cap, theta = 4, 3, 4, 2, 16, 10000.0
    q, k, v = _inputs(B, T, H, Hkv, 5)
    k[1, 0, 0] = 0                                     # all-zero blocks: scale byte 0 (exponent -127), bytes 0
    v[1, 0, 1, 32:] = 0
    lens = [0, 7, cap - 2, cap]                        # the last two run past the cache
    big = _filled(B, cap, Hkv, guard=4)
    kc, vc, kcs, vcs = (t[:, :cap] for t in big)
    q_out = K.kv_append_q8(k, v, kc, vc, kcs, vcs, torch.tensor(lens, dtype=torch.int32), q=q, theta=theta)
    for t in big:                                      # guard rows: neither bytes nor scales
        assert (t[:, cap:] == FILL).all()
    for b, n in enumerate(lens):
        written = []
        for t in range(T):
            p = n + t
            if p >= cap:
                assert (q_out[b, t] == 0).all(), (b, t)
                continue
            qr = K.rope_reference(q[b:b + 1, t:t + 1], None, p, theta)[0]
            kr = K.rope_reference(k[b:b + 1, t:t + 1], None, p, theta)[0]
            assert kr.dtype == BF16 and torch.equal(q_out[b, t], qr[0, 0]), (b, t)
            wk, wks = _mx(kr[0, 0])
            wv, wvs = _mx(v[b, t])
            assert torch.equal(kc[b, p], wk) and torch.equal(kcs[b, p], wks), (b, t)
            assert torch.equal(vc[b, p], wv) and torch.equal(vcs[b, p], wvs), (b, t)
            written.append(p)
        rest = torch.ones(cap, dtype=torch.bool)
        rest[written] = False
        for t in (kc, vc, kcs, vcs):
            assert (t[b][rest] == FILL).all(), b
    assert (kcs[1, 7, 0] == 0).all() and (kc[1, 7, 0] & 0x7F == 0).all() and (kcs[1, 7, 1] != 0).all()   # (rope gives -0)
    assert vcs[1, 7, 1, 1] == 0 and (vc[1, 7, 1, 32:] == 0).all() and vcs[1, 7, 1, 0] != 0


def test_append_reference_host_base_mode():
    """No lens: T = 5 rows to rows 0..4, k as it is or rotated at positions 0..4."""
    K = _K()
    B, T, Hkv, cap, theta = 2, 5, 2, 8, 10000.0
    _, k, v = _inputs(B, T, 4, Hkv, 6)
    for th in (None, theta):
        kc, vc, kcs, vcs = _filled(B, cap, Hkv)
        assert K.kv_append_q8(k, v, kc, vc, kcs, vcs, None, theta=th) is None
        kr = k if th is None else K.rope_reference(k, None, 0, th)[0]
        wk, wks = _mx(kr)
        wv, wvs = _mx(v)
        assert torch.equal(kc[:, :T], wk) and torch.equal(kcs[:, :T], wks)
        assert torch.equal(vc[:, :T], wv) and torch.equal(vcs[:, :T], wvs)
        for t in (kc, vc, kcs, vcs):
            assert (t[:, T:] == FILL).all()


@pytest.mark.parametrize("H,Hkv", [(8, 8), (8, 2), (32, 1)])
def test_attention_reference_is_the_bf16_reference_on_the_dequantised_cache(H, Hkv):
    from learning_jax_sharding_amd.ops.fp8 import dequantize_mx_ref
    K = _K()
    B, cap, lens = 4, 96, [0, 1, 40, 95]
    gen = torch.Generator().manual_seed(7)
    q = torch.randn(B, 1, H, 64, generator=gen).to(BF16)
    kc, kcs = _mx(torch.randn(B, cap, Hkv, 64, generator=gen).to(BF16))
    vc, vcs = _mx(torch.randn(B, cap, Hkv, 64, generator=gen).to(BF16) * 3.0)
    lt = torch.tensor(lens, dtype=torch.int32)
    deq = lambda c, s: dequantize_mx_ref(c.view(torch.float8_e4m3fn), s.int() - 127)   # noqa: E731
    kd, vd = deq(kc, kcs), deq(vc, vcs)
    assert torch.equal(kd.to(BF16).float(), kd) and torch.equal(vd.to(BF16).float(), vd)     # exact in bf16
    for extra in (1, 0):
        want = K.attn_decode_reference(q, kd.to(BF16), vd.to(BF16), lt, SCALE, extra)
        got = K.attn_decode_q8(q, kc, vc, kcs, vcs, lt, SCALE, extra)
        assert got[0].dtype == BF16 and got[0].shape == (B, 1, H, 64) and got[1].shape == (B, H, 1)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), extra
    assert (got[0][0] == 0).all() and torch.isposinf(got[1][0]).all()            # extra = 0, lens = 0: no key
    # dead rows: the e4m3 NaNs and the e8m0 NaN / zero have no influence
    base = K.attn_decode_q8_reference(q, kc, vc, kcs, vcs, lt, SCALE, 1)
    for byte, sbyte in ((0x7F, 0xFF), (0xFF, 0x00)):
        kp, vp, ksp, vsp = kc.clone(), vc.clone(), kcs.clone(), vcs.clone()
        for b, n in enumerate(lens):
            kp[b, n + 1:] = byte
            vp[b, n + 1:] = byte
            ksp[b, n + 1:] = sbyte
            vsp[b, n + 1:] = sbyte
        got = K.attn_decode_q8_reference(q, kp, vp, ksp, vsp, lt, SCALE, 1)
        assert torch.isfinite(got[0].float()).all()
        assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1]), (byte, sbyte)


# ----------------------------------------------------------------------------- the cache object
def test_quantised_cache_object(host_devices):
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd.models import KVCache, TransformerLM
    host_devices(1)
    model = TransformerLM(**LM)
    plain = model.init_cache(3, 16)
    assert plain.k_scale == [] and plain.v_scale == [] and plain.quant is None and len(plain.layer(0)) == 3
    cache = model.init_cache(3, 16, quant="mxfp8")
    assert cache.quant == "mxfp8" and len(cache) == 2 and cache.max_len == 16 and cache.batch == 3
    assert cache.k[0].shape == (3, 16, 2, 64) and cache.k[0].dtype == U8 and cache.v[1].dtype == U8
    assert cache.k_scale[0].shape == (3, 16, 2, 2) and cache.v_scale[1].dtype == U8
    assert cache.nbytes * 128 == plain.nbytes * 66                                 # 64 + 2 bytes against 128
    k, v, lens, ks, vs = cache.layer(1)
    assert k is cache.k[1] and v is cache.v[1] and lens is cache.lens and ks is cache.k_scale[1] and vs is cache.v_scale[1]
    leaves, td = ljs.tree_flatten(cache)
    assert len(leaves) == 4 * 2 + 1 and all(isinstance(l, ljs.ShardedArray) for l in leaves)
    back = ljs.tree_unflatten(td, leaves)
    assert isinstance(back, KVCache) and back.lens is cache.lens and back.k[1] is cache.k[1]
    assert back.k_scale[0] is cache.k_scale[0] and back.v_scale[1] is cache.v_scale[1] and back.quant == "mxfp8"
    assert len(ljs.tree_flatten(plain)[0]) == 2 * 2 + 1                            # unquantised: as ever
    with pytest.raises(ValueError, match="quant"):
        model.init_cache(3, 16, quant="int4")
    with pytest.raises(ValueError, match="quant"):
        KVCache.zeros(2, 3, 16, 2, 64, quant="fp8")
    with pytest.raises(ValueError, match="dim_head % 32"):
        KVCache.zeros(2, 3, 16, 2, 48, quant="mxfp8")


# ----------------------------------------------------------------------------- generate
def _manual_generate(model, params, tok, plens, new, put, quant):
    """Prefill + greedy decode steps through ``model.apply`` with a cache: what ``generate`` is built from."""
    B = tok.shape[0]
    cache = model.init_cache(B, max(plens) + new, quant=quant)
    with torch.no_grad():
        logits, cache = model.apply({"params": params}, put(tok[:, :max(plens)].numpy()), cache=cache, prompt_lens=plens)
        lg = logits.to_torch()
        cur = torch.stack([lg[b, plens[b] - 1].float().argmax() for b in range(B)])[:, None]
        out = [cur]
        for _ in range(new - 1):
            logits, cache = model.apply({"params": params}, put(cur.numpy()), cache=cache)
            cur = logits.to_torch()[:, -1].float().argmax(-1, keepdim=True)
            out.append(cur)
    return torch.cat(out, dim=1).long(), cache


def test_generate_with_a_quantised_cache(host_devices):
    from learning_jax_sharding_amd.models import TransformerLM, generate
    host_devices(1)
    tok = tokens()
    params, put = lm_params(LM, tok)
    model = TransformerLM(**LM)
    ids = put(tok[:, :max(PLENS)].numpy())
    got = generate(model, params, ids, 6, prompt_lens=PLENS, cache_quant="mxfp8")
    assert got.shape == (4, 6) and got.dtype == torch.int64
    want, cache = _manual_generate(model, params, tok, PLENS, 6, put, "mxfp8")
    assert torch.equal(got, want), (got, want)
    assert cache.lens.to_torch().tolist() == [n + 5 for n in PLENS]
    # the rows of the prompt and of the decode steps hold bytes and scales; the rest is untouched
    k0, s0 = cache.k[0].to_torch(), cache.k_scale[0].to_torch()
    for b, n in enumerate(PLENS):
        assert (s0[b, :n + 5] != 0).all() and k0[b, :n + 5].any()
    assert (s0[0, max(PLENS) + 5:] == 0).all()
    # the prefill attends to unquantised keys: the first token is the unquantised run's
    plain = generate(model, params, ids, 6, prompt_lens=PLENS)
    assert torch.equal(got[:, 0], plain[:, 0])
    with pytest.raises(ValueError, match="cache_quant"):
        generate(model, params, ids, 6, prompt_lens=PLENS, cache_quant="int4")


def test_two_devices_batch_sharded_give_one_devices_tokens(host_devices):
    from learning_jax_sharding_amd.models import TransformerLM, generate
    lm = dict(LM, vocab_size=256, dtype=F32)        # f32: a row's logits do not depend on the rows batched with it
    tok = tokens(vocab=256)
    host_devices(1)
    params1, put1 = lm_params(lm, tok)
    ids1 = put1(tok[:, :max(PLENS)].numpy())
    want = generate(TransformerLM(**lm), params1, ids1, 6, prompt_lens=PLENS, cache_quant="mxfp8")
    host_devices(2)
    params, put, cache_sh, Ctx = mesh_setup((2, 1), lm, tok)
    with Ctx():
        model = TransformerLM(**lm)
        cache = model.init_cache(4, 16, sharding=cache_sh, quant="mxfp8")
        assert tuple(cache.k_scale[0].tile.tile_shape) == (2, 1, 1, 1) and len(cache.k_scale[0].local) == 2
        got = generate(model, params, put(tok[:, :max(PLENS)].numpy()), 6, prompt_lens=PLENS, cache_sharding=cache_sh,
                       cache_quant="mxfp8")
    assert torch.equal(got, want), (got, want)
