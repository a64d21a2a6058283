"""Grouped-query attention (k / v with ``kv_heads < heads``; query head h reads key/value head
h // G, G = heads // kv_heads) on host devices: the torch formulations of ops/kernels.py against the
float64 oracle of tests/attn_oracle.py on ``repeat_interleave``d K / V, the ``kv_heads`` field of
the models, sharding, context parallelism and the flops helpers.

The bound on an f32 result is the one of ``attn_oracle.check_lse`` and tests/test_norm_gpu.py:

    |got - want| <= 4 E_ref + 2^-23 max|want|

with ``want`` the float64 oracle and ``E_ref`` the largest error against it of the *expanded-MHA* f32
reference: the present multi-head code run on K / V expanded to one head per query head."""
import numpy as np
import pytest
import torch

import attn_oracle as AO

F32, F64 = torch.float32, torch.float64
SCALE = 0.25


def _check(name, got, want, ref):
    """The module docstring's bound; prints the figures first."""
    got, want, ref = (t.detach().to(F64) for t in (got, want, ref))
    assert got.shape == want.shape == ref.shape, (name, got.shape, want.shape, ref.shape)
    e_ref = (ref - want).abs().max().item()
    err = (got - want).abs().max().item()
    allowed = 4.0 * e_ref + 2.0 ** -23 * want.abs().max().item()
    print(f"gqa-figures {name} max_err={err:.3e} E_ref={e_ref:.3e} allowed={allowed:.3e}")
    assert torch.isfinite(got).all(), name
    assert err <= allowed, (name, err, e_ref, allowed)


def _group_sum64(t, G):
    """[B, S, H, D] per-query-head gradients -> [B, S, H / G, D], summed in f64."""
    B, S, H, D = t.shape
    return t.to(F64).reshape(B, S, H // G, G, D).sum(3)


def _inputs(H, Hkv, B=2, Sq=24, Sk=40, D=16, seed=0):
    gen = torch.Generator().manual_seed(100 * H + 10 * Hkv + seed)
    q = torch.randn(B, Sq, H, D, generator=gen)
    k = torch.randn(B, Sk, Hkv, D, generator=gen)
    v = torch.randn(B, Sk, Hkv, D, generator=gen)
    do = torch.randn(B, Sq, H, D, generator=gen)
    return q, k, v, do


HEADS = [(4, 2), (6, 2), (4, 1), (4, 4)]
# (causal, q_offset): Sq = 24 queries against Sk = 40 keys, the causal case with the queries as the
# last 24 positions
MASKS = [(False, 0), (True, 16)]


# ----------------------------------------------------------------------------- 1. host reference
@pytest.mark.parametrize("causal,q_offset", MASKS, ids=["full", "causal"])
@pytest.mark.parametrize("H,Hkv", HEADS)
def test_reference_matches_oracle(H, Hkv, causal, q_offset):
    from learning_jax_sharding_amd.ops import kernels as K
    G = H // Hkv
    q, k, v, do = _inputs(H, Hkv)
    kx, vx = k.repeat_interleave(G, 2), v.repeat_interleave(G, 2)
    # forward: the same bits as the present code on expanded K / V
    got = K.attention_reference(q, k, v, SCALE, causal, q_offset)
    assert torch.equal(got, K.attention_reference(q, kx, vx, SCALE, causal, q_offset))
    # oracle: float64 on the expanded K / V, dk / dv summed over each group
    o64, lse64 = AO.forward(q, kx, vx, SCALE, causal, q_offset)
    dq64, dkx64, dvx64 = AO.backward(q, kx, vx, o64, lse64, do, SCALE, causal, q_offset)
    want = (dq64, _group_sum64(dkx64, G), _group_sum64(dvx64, G))
    _check("o", got, o64, K.attention_reference(q, kx, vx, SCALE, causal, q_offset))

    def grads(kk, vv, expand):
        ls = [t.clone().requires_grad_(True) for t in (q, kk, vv)]
        ke, ve = (ls[1].repeat_interleave(G, 2), ls[2].repeat_interleave(G, 2)) if expand else (ls[1], ls[2])
        out = K.attention_reference(ls[0], ke, ve, SCALE, causal, q_offset)
        return torch.autograd.grad(out, ls, do)

    ref = grads(k, v, True)     # expanded MHA, autograd's sum over the group
    got = grads(k, v, False)
    for name, g, w, r in zip(("dq", "dk", "dv"), got, want, ref):
        assert g.shape == w.shape and g.dtype == F32
        _check(name, g, w, r)


@pytest.mark.parametrize("causal,q_offset", MASKS, ids=["full", "causal"])
@pytest.mark.parametrize("H,Hkv", HEADS)
def test_host_blocks_match_oracle(H, Hkv, causal, q_offset):
    """attention_fwd_lse and attention_bwd_block (the ring's block functions) with Hkv < H."""
    from learning_jax_sharding_amd.ops import kernels as K
    G = H // Hkv
    q, k, v, do = _inputs(H, Hkv, seed=1)
    kx, vx = k.repeat_interleave(G, 2), v.repeat_interleave(G, 2)
    o64, lse64 = AO.forward(q, kx, vx, SCALE, causal, q_offset)
    o, lse = K.attention_fwd_lse(q, k, v, SCALE, causal, q_offset)
    ox, lsex = K.attention_fwd_lse(q, kx, vx, SCALE, causal, q_offset)
    assert torch.equal(o, ox) and torch.equal(lse, lsex) and lse.shape == (q.shape[0], H, q.shape[1])
    _check("block o", o, o64, ox)
    # two key blocks merged equal the expanded merge
    st, stx = [None, None], [None, None]
    for (a, b), last in (((0, 24), False), ((24, 40), True)):
        m = K.attention_fwd_merge(q, k[:, a:b], v[:, a:b], SCALE, causal, q_offset - a, st, last)
        mx = K.attention_fwd_merge(q, kx[:, a:b], vx[:, a:b], SCALE, causal, q_offset - a, stx, last)
    assert torch.equal(m, mx) and torch.equal(st[1], stx[1])
    _check("merged o", m, o64, mx)
    # the backward block, given the oracle's output and lse
    dq64, dkx64, dvx64 = AO.backward(q, kx, vx, o64, lse64, do, SCALE, causal, q_offset)
    want = (dq64, _group_sum64(dkx64, G), _group_sum64(dvx64, G))
    o32, lse32 = o64.to(F32), lse64.to(F32)
    rq, rk, rv = K.attention_bwd_block(q, kx, vx, o32, do, lse32, SCALE, causal, q_offset)
    ref = (rq, _group_sum64(rk, G), _group_sum64(rv, G))
    got = K.attention_bwd_block(q, k, v, o32, do, lse32, SCALE, causal, q_offset)
    for name, g, w, r in zip(("block dq", "block dk", "block dv"), got, want, ref):
        assert g.dtype == F32
        _check(name, g, w, r)


def test_reference_rejects_bad_head_counts():
    from learning_jax_sharding_amd.ops import kernels as K
    q, k, v, _ = _inputs(4, 2)
    with pytest.raises(ValueError, match="2 heads and v has 1"):
        K.attention_reference(q, k, v[:, :, :1], SCALE)
    q6 = torch.randn(2, 24, 6, 16)
    k4 = torch.randn(2, 40, 4, 16)
    with pytest.raises(ValueError, match="6 query heads"):
        K.attention_reference(q6, k4, k4, SCALE)
    with pytest.raises(ValueError, match="6 query heads"):
        K.attention_bwd_block(q6, k4, k4, q6, q6, torch.zeros(2, 6, 24), SCALE)


# ----------------------------------------------------------------------------- 2. the module
def _module(kv_heads, impl="fused", heads=8, dim_head=64, **kw):
    from learning_jax_sharding_amd.models import MultiHeadAttention
    return MultiHeadAttention(64, heads=heads, dim_head=dim_head, dtype=F32, impl=impl, kv_heads=kv_heads, **kw)


def _init(model, shape=(2, 12, 64)):
    import learning_jax_sharding_amd as ljs
    x = ljs.random.normal(ljs.random.PRNGKey(0), shape)
    return x, model.init(ljs.random.PRNGKey(1), x)["params"]


def _shapes(params):
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd import nn
    flat = {}

    def walk(t, path=()):
        if isinstance(t, dict):
            for k in sorted(t):
                walk(t[k], path + (k,))
        else:
            flat["/".join(path)] = tuple(t.shape)
    walk(ljs.tree_map(lambda a: a.to_torch(), nn.unbox(params)))
    return flat


def test_module_fields(host_devices):
    host_devices(1)
    x, p_none = _init(_module(None))
    _, p_same = _init(_module(8))
    assert _shapes(p_none) == _shapes(p_same)
    assert _shapes(p_none)["to_k/kernel"] == (64, 512)
    out_none = _module(None).apply({"params": p_none}, x).to_torch()
    out_same = _module(8).apply({"params": p_same}, x).to_torch()
    assert torch.equal(out_none, out_same)
    sh = _shapes(_init(_module(2))[1])
    assert sh["to_k/kernel"] == (64, 128) and sh["to_v/kernel"] == (64, 128)
    assert sh["to_q/kernel"] == (64, 512) and sh["to_out_0/kernel"] == (512, 64)
    assert set(sh) == set(_shapes(p_none))
    for bad in (3, 0, -1, 16):
        with pytest.raises(ValueError, match="kv_heads"):
            _init(_module(bad))


def _module_oracle(p, x, cot, H, D, causal, theta):
    """The block in float64 from the parameters ``p`` (K / V kernels of H heads): output and the
    gradients of sum(out * cot) by parameter."""
    from learning_jax_sharding_amd.ops import kernels as K
    p = {n: {m: t.to(F64).clone().requires_grad_(True) for m, t in d.items()} for n, d in p.items()}
    B, S, _ = x.shape
    x = x.to(F64)
    q, k, v = ((x @ p[n]["kernel"]).view(B, S, H, D) for n in ("to_q", "to_k", "to_v"))
    cos, sin = K.rope_table_host(S, D, theta, dtype=F64)
    cos, sin = cos.view(1, S, 1, D // 2), sin.view(1, S, 1, D // 2)

    def rot(t):
        a, b = t[..., :D // 2], t[..., D // 2:]
        return torch.cat([a * cos - b * sin, b * cos + a * sin], -1)

    o, _ = AO.forward(rot(q), rot(k), v, D ** -0.5, causal)
    out = o.reshape(B, S, H * D) @ p["to_out_0"]["kernel"] + p["to_out_0"]["bias"]
    leaves = [(n, m) for n in sorted(p) for m in sorted(p[n])]
    gs = torch.autograd.grad(out, [p[n][m] for n, m in leaves], cot.to(F64))
    return out.detach(), {f"{n}/{m}": g for (n, m), g in zip(leaves, gs)}


@pytest.mark.parametrize("impl", ["fused", "einsum"])
def test_module_equals_repeated_kv_weights(host_devices, impl):
    """A causal + RoPE GQA block in f32 against the float64 oracle of the MHA block whose K / V kernels
    repeat each key/value head's 64 columns G times; E_ref is the f32 MHA module on those kernels.
    The GQA kernel gradient is the sum of the repeats' gradients."""
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd import nn
    host_devices(1)
    H, Hkv, D, theta = 8, 2, 64, 1e4
    G = H // Hkv
    kw = dict(causal=True, rope_theta=theta)
    gqa, mha = _module(Hkv, impl, **kw), _module(None, impl, **kw)
    x, params = _init(gqa)
    params = nn.unbox(params)
    pt = ljs.tree_map(lambda a: a.to_torch(), params)

    def repeat(w):   # [M, Hkv * D] -> [M, H * D], head j's columns G times
        return w.view(-1, Hkv, 1, D).expand(-1, Hkv, G, D).reshape(-1, H * D).contiguous()

    def fold(g):     # the gradient of the repeated kernel -> of the GQA kernel (f64)
        return g.to(F64).view(-1, Hkv, G, D).sum(2).reshape(-1, Hkv * D)

    pt_rep = {n: dict(d) for n, d in pt.items()}
    for n in ("to_k", "to_v"):
        pt_rep[n]["kernel"] = repeat(pt[n]["kernel"])
    p_rep = {n: {m: ljs.device_put(t) for m, t in d.items()} for n, d in pt_rep.items()}
    cot = torch.randn(tuple(x.shape), generator=torch.Generator().manual_seed(5))
    cot_a = ljs.device_put(cot)

    def run(model, p):
        val, g = ljs.value_and_grad(lambda q: (model.apply({"params": q}, x) * cot_a).sum())(p)
        out = model.apply({"params": p}, x).to_torch()
        g = ljs.tree_map(lambda a: a.to_torch(), nn.unbox(g))
        return out, {f"{n}/{m}": g[n][m] for n in g for m in g[n]}

    want_out, want_g = _module_oracle(pt_rep, x.to_torch(), cot, H, D, True, theta)
    ref_out, ref_g = run(mha, p_rep)
    got_out, got_g = run(gqa, params)
    assert got_out.dtype == F32
    _check(f"{impl} out", got_out, want_out, ref_out)
    assert set(got_g) == set(want_g)
    for name in sorted(got_g):
        w, r = want_g[name], ref_g[name]
        if name in ("to_k/kernel", "to_v/kernel"):
            w, r = fold(w), fold(r)
        assert got_g[name].shape == w.shape, name
        _check(f"{impl} d {name}", got_g[name], w, r)


def test_attention_next_hint_not_given(host_devices, monkeypatch):
    """The fused projection + forward kernel is multi-head only: no hint with kv_heads < heads, and
    the projections are one dense for Q and one two-kernel dense for K | V."""
    import contextlib
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd.ops import linear as L
    from learning_jax_sharding_amd.spmd import plan as _plan
    host_devices(1)
    entered = []

    @contextlib.contextmanager
    def recording(heads, dim_head, scale):
        entered.append((heads, dim_head))
        yield

    monkeypatch.setattr(L, "attention_next", recording)
    x = ljs.random.normal(ljs.random.PRNGKey(0), (2, 256, 128))
    seen = {}
    for name, kv in (("mha", None), ("same", 2), ("gqa", 1)):
        from learning_jax_sharding_amd.models import MultiHeadAttention
        model = MultiHeadAttention(128, heads=2, dim_head=64, kv_heads=kv)
        params = model.init(ljs.random.PRNGKey(1), x)["params"]
        del entered[:]
        with _plan.record_plan() as rec:
            model.apply({"params": params}, x)
        seen[name] = (len(entered), [s.info["n_kernels"] for s in rec.steps if s.kind == "dense"],
                      [s.info.get("kv_heads") for s in rec.steps if s.kind == "attention"])
    assert seen["mha"] == (1, [3, 1], [2]) and seen["same"] == seen["mha"], seen
    assert seen["gqa"] == (0, [1, 2, 1], [1]), seen


# ----------------------------------------------------------------------------- 3. sharding
_LM = dict(vocab_size=256, dim=64, layers=1, heads=4, dim_head=16, ff_dim=128, max_len=16)


def _lm_run(host_devices, mesh_shape, kv_heads):
    from test_embed import lm_step
    from learning_jax_sharding_amd.spmd import plan as _plan
    host_devices(int(np.prod(mesh_shape)))
    with _plan.record_plan() as rec:
        logits, val, grads, _, spec = lm_step(mesh_shape, dict(_LM, kv_heads=kv_heads))
    return val, grads, spec, rec


def test_lm_step_on_meshes(host_devices):
    """heads=4, kv_heads=2 through tests/test_embed.py's lm_step on 1 x 1 and 2 x 2 host meshes: the
    loss agreement of test_transformer_lm_step (1e-5 max(1, |loss|)), K / V kernels of 32 columns
    split over model, and no collective that the kv_heads=4 run lacks."""
    one, g1, spec1, _ = _lm_run(host_devices, (1, 1), 2)
    val, g4, spec4, rec = _lm_run(host_devices, (2, 2), 2)
    print(f"gqa-lm loss 1-device={one:.8g} 2x2={val:.8g} diff={abs(one - val):.3g}")
    assert np.isfinite(val) and 3.0 < val < 9.0, val
    assert abs(val - one) <= 1e-5 * max(1.0, abs(one)), (val, one)
    assert set(g1) == set(g4)
    for name, g in g4.items():
        assert np.isfinite(g).all(), name
    assert g4["layer_0/attn/to_k/kernel"].shape == (64, 32) and g4["layer_0/attn/to_v/kernel"].shape == (64, 32)
    assert g4["layer_0/attn/to_q/kernel"].shape == (64, 64)
    assert spec4["layer_0/attn/to_k/kernel"] == (1, 2)
    # (the init, the forward and the forward inside value_and_grad)
    assert [s.info["kv_heads"] for s in rec.steps if s.kind == "attention"] == [2, 2, 2]
    _, _, _, rec_mha = _lm_run(host_devices, (2, 2), 4)
    from collections import Counter
    have, base = Counter(rec.collective_kinds()), Counter(rec_mha.collective_kinds())
    print(f"gqa-lm collectives gqa={dict(have)} mha={dict(base)}")
    assert set(have) <= set(base), (have, base)


def test_kv_heads_below_the_shard_count_raises(host_devices):
    """kv_heads=1 with the heads over a 2-way model axis: a ValueError naming kv_heads and the shard
    count, from the model and from dot_product_attention on head-sharded arrays."""
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd.mesh import Mesh, create_device_mesh
    from learning_jax_sharding_amd.ops import core
    from learning_jax_sharding_amd.sharding import NamedSharding, PartitionSpec as P
    with pytest.raises(ValueError, match=r"kv_heads=1 .*2 ways"):
        _lm_run(host_devices, (2, 2), 1)
    host_devices(4)
    mesh = Mesh(create_device_mesh((2, 2)), ("data", "model"))
    sh = NamedSharding(mesh, P("data", None, "model"))
    q = ljs.device_put(torch.randn(2, 8, 4, 16).bfloat16(), sh)
    kv1 = ljs.device_put(torch.randn(2, 8, 1, 16).bfloat16(), NamedSharding(mesh, P("data")))
    with pytest.raises(ValueError, match=r"kv_heads=1 .*2 ways"):
        core.dot_product_attention(q, kv1, kv1)
    # two key/value heads over the two shards: each device's query heads read its own key/value head
    from learning_jax_sharding_amd.ops import kernels as K
    kt, vt = torch.randn(2, 8, 2, 16).bfloat16(), torch.randn(2, 8, 2, 16).bfloat16()
    k2, v2 = ljs.device_put(kt, sh), ljs.device_put(vt, sh)
    got = core.dot_product_attention(q, k2, v2, causal=True).to_torch()
    want = K.attention_reference(q.to_torch(), kt, vt, 16 ** -0.5, True)
    assert torch.equal(got, want)


# ----------------------------------------------------------------------------- 4. context parallelism
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("mesh_shape", [(1, 4), (2, 2)])
def test_context_parallel_modes_agree(host_devices, causal, mesh_shape):
    """tests/test_numeric.py::test_ring_attention_matches_allgather with K / V of 2 heads against q's
    4: ring, Ulysses and all-gather agree in values and gradients (the same tolerances).  Ulysses
    needs kv_heads % group == 0: with 4 sequence shards it runs the all-gather plan."""
    import learning_jax_sharding_amd as ljs
    import learning_jax_sharding_amd.numpy as jnp
    from learning_jax_sharding_amd.array import ShardedArray
    from learning_jax_sharding_amd.mesh import Mesh, create_device_mesh
    from learning_jax_sharding_amd.parallel import sequence as SQ
    from learning_jax_sharding_amd.sharding import NamedSharding, PartitionSpec as P
    from learning_jax_sharding_amd.spmd import plan as _plan
    host_devices(4)
    mesh = Mesh(create_device_mesh(mesh_shape), ("data", "model"))
    g = torch.Generator().manual_seed(0)
    B, S, H, Hkv, D = 2, 32, 4, 2, 16
    arrs = [torch.randn(B, S, h, D, generator=g).bfloat16() for h in (H, Hkv, Hkv)]
    cot = torch.randn(B, S, H, D, generator=g)
    sh = NamedSharding(mesh, P("data", "model"))
    res = {}
    for mode in ("allgather", "ring", "ulysses"):
        q, k, v = (ljs.device_put(a, sh) for a in arrs)
        leaves = [ljs.spmd.api._fresh_leaf(a) for a in (q, k, v)]
        with _plan.record_plan() as rec:
            out = SQ.context_parallel_attention(*leaves, causal=causal, mode=mode)
        kinds = [st.kind for st in rec.steps]
        if mode == "ulysses":
            if mesh_shape == (2, 2):
                assert "ulysses_attention" in kinds and kinds.count("all_to_all") == 4, kinds
            else:
                assert "ulysses_attention" not in kinds and "all_to_all" not in kinds, kinds
        if mode == "ring":
            assert "ring_attention" in kinds, kinds
        loss = (out.astype(jnp.float32) * ljs.device_put(cot, sh)).sum()
        ins = [t for l in leaves for t in l.local.values()]
        outs = [t for t in loss.local.values()]
        gs = torch.autograd.grad(outs, ins, [torch.full_like(t, 1.0 / len(outs)) for t in outs])
        n_loc = len(leaves[0].local)
        glob = []
        for ai, leaf in enumerate(leaves):
            loc = {d: gs[ai * n_loc + i] for i, d in enumerate(leaf.local)}
            assert all(tuple(t.shape) == tuple(leaf.local[d].shape) for d, t in loc.items())
            ga = ShardedArray(leaf.shape, torch.float32, leaf.sharding, {d: t.float() for d, t in loc.items()})
            glob.append(np.asarray(ga))
        assert glob[1].shape == (B, S, Hkv, D) and glob[2].shape == (B, S, Hkv, D)
        res[mode] = (np.asarray(out.astype(jnp.float32)), glob)
    for mode in ("ring", "ulysses"):
        np.testing.assert_allclose(res[mode][0], res["allgather"][0], rtol=2e-2, atol=2e-2)
        for a, b in zip(res[mode][1], res["allgather"][1]):
            np.testing.assert_allclose(a, b, rtol=3e-2, atol=3e-2 * max(1.0, np.abs(b).max()))


# ----------------------------------------------------------------------------- 5. flops
def test_flops_helpers():
    from learning_jax_sharding_amd.models.attention import attention_block_flops
    from learning_jax_sharding_amd.models.transformer import transformer_layer_flops
    B, S, M, H, D, F = 8, 256, 640, 8, 64, 2560
    t, inner = B * S, H * D
    qk = 2 * B * H * S * S * D
    out = 2 * t * inner * M
    for train in (False, True):
        # kv_heads=None: the present values, written out
        qkv = 3 * 2 * t * M * inner
        fwd = qkv + 2 * qk + out
        want = fwd + (2 * out + 4 * qk + qkv if train else 0)
        assert attention_block_flops(B, S, M, H, D, train) == float(want)
        assert attention_block_flops(B, S, M, H, D, train, kv_heads=None) == float(want)
        assert attention_block_flops(B, S, M, H, D, train, kv_heads=8) == float(want)
        ff = 2 * 2 * t * M * F
        assert transformer_layer_flops(B, S, M, H, D, F, train) == want + (3 * ff if train else ff)
        # kv_heads=2 of 8: Q of 512 columns, K and V of 128 each; scores and P.V unchanged
        qkv2 = 2 * t * M * 512 + 2 * (2 * t * M * 128)
        fwd2 = qkv2 + 2 * qk + out
        want2 = fwd2 + (2 * out + 4 * qk + qkv2 if train else 0)
        assert attention_block_flops(B, S, M, H, D, train, kv_heads=2) == float(want2)
        assert want2 < want
        ffg = 3 * 2 * t * M * F
        assert transformer_layer_flops(B, S, M, H, D, F, train, gated=True, kv_heads=2) == \
            want2 + (3 * ffg if train else ffg)
    assert attention_block_flops(8, 256, 640, 8, 64, False) == pytest.approx(6.442e9, rel=1e-3)
