"""The KV cache, the decode references and greedy generation on host devices.

* ``plan_decode`` (the pure plan of csrc/kernels/decode.hip) over a grid of arguments;
* ``attn_decode_reference`` against the float64 oracle of tests/attn_oracle.py, per sequence
  ``forward(q, k[:n_b], v[:n_b], causal=False)``, held by ``AO.check`` / ``AO.check_lse``;
  ``kv_append_reference`` against ``rope_reference`` + copy, bit for bit;
* a small ``TransformerLM`` teacher-forced through prefill + 8 decode steps against its uncached causal
  forward on the same tokens at the same positions.  The rule: with ``R`` the logits of the same model
  in float32, uncached, ``A`` the bf16 uncached logits and ``C`` the bf16 cached ones,

      max|C - R| <= 4 max|A - R| + 2^-23 max|R|

  (the project's factor for another equally valid evaluation order); both sides are printed;
* ``generate`` with a float32 model against a Python loop of uncached forwards with ``argmax``;
* two host devices (a batch-sharded and a head-sharded mesh) against one; the errors.
"""
import itertools

import numpy as np
import pytest
import torch

import attn_oracle as AO

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
SCALE = 0.125
LM = dict(vocab_size=257, dim=128, layers=2, heads=4, kv_heads=2, dim_head=64, norm="rms", ff="swiglu",
          rope_theta=10000.0, causal=True)
PLENS = [5, 9, 7, 6]
STEPS = 8


# ----------------------------------------------------------------------------- 1. the plan
def test_plan_decode_properties():
    from learning_jax_sharding_amd.ops import hip
    tile = hip.decode_key_tile()
    assert tile == 32
    grid = itertools.product([1, 2, 8, 64, 300], [1, 2, 8], [1, 31, 32, 33, 100, 512, 4096, 32768, 100000],
                             [1, 64, 256, 304])
    seen = {}
    for B, Hkv, cap, cus in grid:
        splits, keys = hip.plan_decode(B, Hkv, cap, cus)
        assert splits >= 1 and keys >= tile and keys % tile == 0, (B, Hkv, cap, cus, splits, keys)
        assert splits * keys >= cap, (B, Hkv, cap, cus, splits, keys)
        assert (splits - 1) * keys < cap, (B, Hkv, cap, cus, splits, keys)      # no split starts past the cache
        if cap <= tile:
            assert splits == 1, (B, Hkv, cap, cus, splits)
        seen[(B, Hkv, cap, cus)] = (splits, keys)
    # pure: a forced launch plan, other calls in between and a second pass change nothing
    hip.set_decode_splits(4, 128)
    try:
        for args, want in seen.items():
            assert hip.plan_decode(*args) == want, args
    finally:
        hip.set_decode_splits(None)
    # a long cache on few sequences is split to fill the chip; many sequences need no split
    assert hip.plan_decode(1, 1, 32768, 256)[0] >= 256
    assert hip.plan_decode(512, 8, 512, 256)[0] == 1
    with pytest.raises(ValueError):
        hip.plan_decode(0, 1, 512, 256)


# ----------------------------------------------------------------------------- 2. the references
def _oracle_check(name, o, lse, q, k, v, ns):
    G = q.shape[2] // k.shape[2]
    for b, n in enumerate(ns):
        if n == 0:
            assert torch.equal(o[b], torch.zeros_like(o[b])) and torch.isposinf(lse[b]).all(), name
            continue
        qb = q[b:b + 1]
        kb, vb = (t[b:b + 1, :n].repeat_interleave(G, 2) for t in (k, v))
        want_o, want_lse = AO.forward(qb, kb, vb, SCALE)
        model_o, _ = AO.forward(qb, kb, vb, SCALE, rounded=True)
        AO.check(f"{name} b{b} o", o[b:b + 1], want_o, model_o)
        AO.check_lse(lse[b:b + 1], want_lse, AO.lse2_f32(qb, kb, SCALE), name=f"{name} b{b} lse")


@pytest.mark.parametrize("kind", AO.KINDS)
@pytest.mark.parametrize("H,Hkv", [(8, 8), (8, 2), (32, 1)])
def test_attn_decode_reference_matches_oracle(kind, H, Hkv):
    from learning_jax_sharding_amd.ops import kernels as K
    cap, lens = 96, [0, 1, 40, 95]
    q, k, v, _ = AO.inputs(kind, 4, H, 1, cap, SCALE)
    k, v = k[:, :, :Hkv].contiguous(), v[:, :, :Hkv].contiguous()
    o, lse = K.attn_decode(q, k, v, torch.tensor(lens, dtype=torch.int32), SCALE, 1)
    assert o.shape == (4, 1, H, 64) and o.dtype == BF16 and lse.shape == (4, H, 1) and lse.dtype == F32
    _oracle_check(f"ref {kind} H{H}/{Hkv}", o, lse, q, k, v, [n + 1 for n in lens])
    # extra = 0: no key at all, and the whole cache
    o, lse = K.attn_decode_reference(q[:2], k[:2], v[:2], torch.tensor([0, cap], dtype=torch.int32), SCALE, 0)
    _oracle_check(f"ref extra0 {kind}", o, lse, q[:2], k[:2], v[:2], [0, cap])
    # rows at and beyond n_b have no influence, whatever they hold
    lt = torch.tensor(lens, dtype=torch.int32)
    base = K.attn_decode_reference(q, k, v, lt, SCALE, 1)
    for fill in (float("nan"), float("inf"), 3e38):
        kp, vp = k.clone(), v.clone()
        for b, n in enumerate(lens):
            kp[b, n + 1:] = fill
            vp[b, n + 1:] = fill
        got = K.attn_decode_reference(q, kp, vp, lt, SCALE, 1)
        assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1]), fill


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_kv_append_reference_is_rope_plus_copy(dtype):
    from learning_jax_sharding_amd.ops import kernels as K
    B, T, H, Hkv, D, cap, theta = 4, 3, 4, 2, 64, 16, 10000.0
    gen = torch.Generator().manual_seed(5)
    q = torch.randn(B, T, H, D, generator=gen).to(dtype)
    k = torch.randn(B, T, Hkv, D, generator=gen).to(dtype)
    v = torch.randn(B, T, Hkv, D, generator=gen).to(dtype)
    lens = [0, 7, cap - 2, cap]                      # the last two run past the cache
    kc = torch.full((B, cap, Hkv, D), 7.0, dtype=dtype)
    vc = torch.full((B, cap, Hkv, D), 7.0, dtype=dtype)
    q_out = K.kv_append(k, v, kc, vc, torch.tensor(lens, dtype=torch.int32), q=q, theta=theta)
    for b, n in enumerate(lens):
        written = []
        for t in range(T):
            p = n + t
            if p >= cap:
                assert (q_out[b, t] == 0).all(), (b, t)
                continue
            qr, kr = K.rope_reference(q[b:b + 1, t:t + 1], None, p, theta)[0], \
                K.rope_reference(k[b:b + 1, t:t + 1], None, p, theta)[0]
            assert torch.equal(q_out[b, t], qr[0, 0]) and torch.equal(kc[b, p], kr[0, 0]), (b, t)
            assert torch.equal(vc[b, p], v[b, t]), (b, t)
            written.append(p)
        rest = torch.ones(cap, dtype=torch.bool)
        rest[written] = False
        assert (kc[b][rest] == 7.0).all() and (vc[b][rest] == 7.0).all(), b
    # host-base mode: rows 0 .. T-1, k as it is
    kc.fill_(7.0)
    vc.fill_(7.0)
    assert K.kv_append(k, v, kc, vc) is None
    assert torch.equal(kc[:, :T], k) and torch.equal(vc[:, :T], v) and (kc[:, T:] == 7.0).all()


# ----------------------------------------------------------------------------- 3. the model
def tokens(B=4, S=24, vocab=257, seed=0):
    return torch.randint(0, vocab, (B, S), generator=torch.Generator().manual_seed(seed))


def lm_params(lm, tok, put=None):
    """(f32 parameters, put) of ``TransformerLM(**lm)``; ``put``: host ids -> array (default: unplaced)."""
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd.models import TransformerLM
    put = put or (lambda a: ljs.device_put(np.asarray(a)))
    return TransformerLM(**lm).init(ljs.random.PRNGKey(1), put(tok.numpy()))["params"], put


def uncached_logits(lm, params, tok, put, dtype):
    from learning_jax_sharding_amd.models import TransformerLM
    with torch.no_grad():
        return TransformerLM(**lm, dtype=dtype).apply({"params": params}, put(tok.numpy())).to_torch().double()


def teacher_forced(lm, params, tok, plens, steps, put, dtype=BF16, cache_sharding=None, max_len=None, step_fn=None):
    """Cached logits of the real positions: prefill of the right-padded prompts ``tok[:, :max(plens)]`` then
    ``steps`` decode steps fed ``tok[b, plens[b] + s]``.  Returns (rows, cache): rows[b] is ``[plens[b] + steps,
    vocab]`` float64, to be compared with the uncached forward's ``[b, :plens[b] + steps]``."""
    from learning_jax_sharding_amd.models import TransformerLM
    model = TransformerLM(**lm, dtype=dtype)
    B, P = tok.shape[0], max(plens)
    cache = model.init_cache(B, max_len or (P + steps), sharding=cache_sharding)
    logits, cache = model.apply({"params": params}, put(tok[:, :P].numpy()), cache=cache, prompt_lens=plens)
    lp = logits.to_torch().double()
    rows = [[lp[b, :plens[b]]] for b in range(B)]
    assert cache.lens.to_torch().tolist() == list(plens)
    step_fn = step_fn or (lambda p, x, c: model.apply({"params": p}, x, cache=c))
    for s in range(steps):
        t = torch.stack([tok[b, plens[b] + s] for b in range(B)])[:, None]
        lg, cache = step_fn(params, put(t.numpy()), cache)
        lg = lg.to_torch().double()
        assert lg.shape[1] == 1
        for b in range(B):
            rows[b].append(lg[b])
    assert cache.lens.to_torch().tolist() == [n + steps for n in plens]
    return [torch.cat(r) for r in rows], cache


def rule_check(name, rows, R, A, plens, steps):
    """max|C - R| <= 4 max|A - R| + 2^-23 max|R| over the real positions; prints both sides."""
    real = [slice(0, n + steps) for n in plens]
    err_c = max((rows[b] - R[b, real[b]]).abs().max().item() for b in range(len(plens)))
    err_a = max((A[b, real[b]] - R[b, real[b]]).abs().max().item() for b in range(len(plens)))
    rmax = max(R[b, real[b]].abs().max().item() for b in range(len(plens)))
    allowed = 4.0 * err_a + 2.0 ** -23 * rmax
    print(f"decode-figures {name} max|C-R|={err_c:.4e} max|A-R|={err_a:.4e} allowed={allowed:.4e} max|R|={rmax:.3f}")
    assert all(torch.isfinite(r).all() for r in rows), name
    assert err_c <= allowed, (name, err_c, err_a, allowed)


@pytest.mark.parametrize("pos", ["rope", "table"])
def test_cached_decode_matches_uncached_forward(host_devices, pos):
    host_devices(1)
    lm = dict(LM) if pos == "rope" else dict(LM, rope_theta=None, max_len=32)
    tok = tokens()
    params, put = lm_params(lm, tok)
    R = uncached_logits(lm, params, tok, put, F32)
    A = uncached_logits(lm, params, tok, put, BF16)
    rows, cache = teacher_forced(lm, params, tok, PLENS, STEPS, put, max_len=32)
    assert cache.k[0].shape == (4, 32, 2, 64) and cache.k[0].dtype == BF16 and cache.lens.dtype == torch.int32
    rule_check(f"host {pos}", rows, R, A, PLENS, STEPS)
    # a prefill restarts the cache: the same prompt again gives the same logits and lengths
    from learning_jax_sharding_amd.models import TransformerLM
    model = TransformerLM(**lm)
    again, cache = model.apply({"params": params}, put(tok[:, :9].numpy()), cache=cache, prompt_lens=PLENS)
    assert cache.lens.to_torch().tolist() == PLENS
    for b, n in enumerate(PLENS):
        assert torch.equal(again.to_torch().double()[b, :n], rows[b][:n])


def test_cache_is_a_pytree(host_devices):
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd.models import KVCache, TransformerLM
    host_devices(1)
    cache = TransformerLM(**LM).init_cache(3, 16)
    leaves, td = ljs.tree_flatten(cache)
    assert len(leaves) == 2 * 2 + 1 and all(isinstance(l, ljs.ShardedArray) for l in leaves)
    back = ljs.tree_unflatten(td, leaves)
    assert isinstance(back, KVCache) and back.lens is cache.lens and back.k[1] is cache.k[1]
    assert all(float(l.to_torch().float().abs().sum()) == 0.0 for l in leaves)


# ----------------------------------------------------------------------------- 4. generate
def reference_generate(lm, params, tok, plens, new, put, dtype=F32):
    """A Python loop of uncached forwards with argmax: (tokens [B, new], the smallest top-2 logit gap
    over the steps divided by the largest |logit|)."""
    from learning_jax_sharding_amd.models import TransformerLM
    model = TransformerLM(**lm, dtype=dtype)
    B = tok.shape[0]
    seqs = [tok[b, :plens[b]].tolist() for b in range(B)]
    out, gap = [], float("inf")
    with torch.no_grad():
        for _ in range(new):
            L = max(len(s) for s in seqs)
            batch = torch.tensor([s + [0] * (L - len(s)) for s in seqs])
            logits = model.apply({"params": params}, put(batch.numpy())).to_torch().double()
            step = []
            for b, s in enumerate(seqs):
                row = logits[b, len(s) - 1]
                top = row.topk(2).values
                gap = min(gap, ((top[0] - top[1]) / row.abs().max()).item())
                step.append(int(row.argmax()))
                s.append(step[-1])
            out.append(step)
    return torch.tensor(out).T.contiguous(), gap


GEN_SEED = 8     # chosen for the reference's own top-2 gaps, at vocab 257 and 256 (asserted below)


def test_generate_matches_uncached_loop(host_devices):
    from learning_jax_sharding_amd.models import TransformerLM, generate
    host_devices(1)
    tok = tokens(seed=GEN_SEED)
    params, put = lm_params(LM, tok)
    want, gap = reference_generate(LM, params, tok, PLENS, 8, put)
    print(f"decode-figures generate reference top-2 gap / max|logit| = {gap:.3e}")
    assert gap >= 1e-3, gap          # the precondition, on the reference alone
    model = TransformerLM(**LM, dtype=F32)
    got = generate(model, params, put(tok[:, :max(PLENS)].numpy()), 8, prompt_lens=PLENS)
    assert got.shape == (4, 8) and got.dtype == torch.int64
    assert torch.equal(got, want), (got, want)
    one = generate(model, params, put(tok[:, :max(PLENS)].numpy()), 1, prompt_lens=PLENS)
    assert torch.equal(one, want[:, :1])


# ----------------------------------------------------------------------------- 5. two devices
def mesh_setup(mesh_shape, lm, tok, host_params=None):
    """(params placed by the vocab-parallel rules, put, cache sharding, context manager factory);
    ``host_params``: the values (host arrays by path) instead of a fresh init's."""
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd import nn
    from learning_jax_sharding_amd.mesh import Mesh, create_device_mesh
    from learning_jax_sharding_amd.models import TransformerLM
    from learning_jax_sharding_amd.parallel.tensor import VOCAB_PARALLEL_RULES as rules
    from learning_jax_sharding_amd.sharding import NamedSharding, PartitionSpec as P
    mesh = Mesh(create_device_mesh(mesh_shape), ("data", "model"))
    put = lambda a: ljs.device_put(np.asarray(a), NamedSharding(mesh, P("data")))   # noqa: E731
    with mesh, nn.axis_rules(rules):
        params = TransformerLM(**lm).init(ljs.random.PRNGKey(1), put(tok.numpy()))["params"]
    shardings = nn.logical_to_mesh_sharding(nn.get_partition_spec(params), mesh, rules)
    params = ljs.device_put(params if host_params is None else host_params, shardings)

    class Ctx:
        def __enter__(self):
            self.a, self.b = mesh, nn.axis_rules(rules)
            self.a.__enter__()
            self.b.__enter__()

        def __exit__(self, *e):
            self.b.__exit__(*e)
            self.a.__exit__(*e)

    return params, put, NamedSharding(mesh, P("data", None, "model", None)), Ctx


@pytest.mark.parametrize("mesh_shape", [(2, 1), (1, 2)], ids=["batch", "heads"])
def test_two_devices_match_one(host_devices, mesh_shape):
    from learning_jax_sharding_amd import nn
    from learning_jax_sharding_amd.models import TransformerLM, generate
    from learning_jax_sharding_amd.spmd import plan as _plan
    lm = dict(LM, vocab_size=256)
    tok = tokens(vocab=256, seed=GEN_SEED)
    host_devices(1)
    params1, put1 = lm_params(lm, tok)
    R = uncached_logits(lm, params1, tok, put1, F32)
    A = uncached_logits(lm, params1, tok, put1, BF16)
    want, gap = reference_generate(lm, params1, tok, PLENS, 6, put1)
    assert gap >= 1e-3, gap
    host_devices(2)
    params, put, cache_sh, Ctx = mesh_setup(mesh_shape, lm, tok)
    flat1 = {k: v for k, v in _flat(nn.unbox(params1))}
    for k, v in _flat(nn.unbox(params)):          # the same parameters on both
        assert torch.equal(v.to_torch(), flat1[k].to_torch()), k
    with Ctx(), _plan.record_plan() as rec:
        rows, cache = teacher_forced(lm, params, tok, PLENS, STEPS, put, cache_sharding=cache_sh)
    assert tuple(cache.k[0].tile.tile_shape) == (mesh_shape[0], 1, mesh_shape[1], 1)
    assert [s.info["tiles"] for s in rec.steps if s.kind == "cached_attention"] == \
        [(mesh_shape[0], 1, mesh_shape[1], 1)] * (2 * STEPS)
    rule_check(f"2 devices {mesh_shape}", rows, R, A, PLENS, STEPS)
    with Ctx():
        got = generate(TransformerLM(**lm, dtype=F32), params, put(tok[:, :max(PLENS)].numpy()), 6,
                       prompt_lens=PLENS, cache_sharding=cache_sh)
    assert torch.equal(got, want), (got, want)


def _flat(tree, path=()):
    if isinstance(tree, dict):
        for k in sorted(tree):
            yield from _flat(tree[k], path + (k,))
    else:
        yield "/".join(path), tree


# ----------------------------------------------------------------------------- 6. errors
def test_errors(host_devices):
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd.mesh import Mesh, create_device_mesh
    from learning_jax_sharding_amd.models import MultiHeadAttention, TransformerLM, generate
    from learning_jax_sharding_amd.sharding import NamedSharding, PartitionSpec as P
    host_devices(2)
    tok = tokens(B=2, S=12)
    params, put = lm_params(LM, tok)
    ids = put(tok.numpy())
    model = TransformerLM(**LM)
    cache = model.init_cache(2, 16)
    with pytest.raises(ValueError, match="max_len"):
        generate(model, params, ids, 5, max_len=16)                     # 12 + 5 > 16
    with pytest.raises(ValueError, match="max_len"):
        generate(TransformerLM(**dict(LM, rope_theta=None, max_len=16)), params, ids, 5)
    with pytest.raises(ValueError, match="prompt_lens"):
        generate(model, params, ids, 2, prompt_lens=[3, 13])
    with pytest.raises(ValueError, match="causal"):
        TransformerLM(**dict(LM, causal=False)).apply({"params": params}, ids, cache=cache)
    relu = dict(LM, ff="relu", fp8=True)
    with pytest.raises(ValueError, match="fp8"):
        TransformerLM(**relu).apply({"params": params}, ids, cache=cache)
    with pytest.raises(ValueError, match="max_len"):
        model.apply({"params": params}, put(tokens(B=2, S=17).numpy()), cache=cache)
    # the attention block: a context and the einsum formulation
    attn = MultiHeadAttention(128, heads=4, dim_head=64, kv_heads=2, causal=True, rope_theta=10000.0)
    x = ljs.random.normal(ljs.random.PRNGKey(0), (2, 4, 128))
    ap = attn.init(ljs.random.PRNGKey(1), x)["params"]
    layer = cache.layer(0)
    out, back = attn.apply({"params": ap}, x, cache=layer)
    assert out.shape == (2, 4, 128) and back[0] is layer[0]
    with pytest.raises(ValueError, match="context"):
        attn.apply({"params": ap}, x, context=x, cache=layer)
    ein = MultiHeadAttention(128, heads=4, dim_head=64, kv_heads=2, causal=True, impl="einsum")
    with pytest.raises(ValueError, match="einsum"):
        ein.apply({"params": ap}, x, cache=layer)
    # a length-sharded cache
    mesh = Mesh(create_device_mesh((1, 2)), ("data", "model"))
    with pytest.raises(NotImplementedError, match="length-sharded"):
        model.init_cache(2, 16, sharding=NamedSharding(mesh, P(None, "model")))
    # kv_heads that the head shards do not divide: the existing ValueError
    mqa = TransformerLM(**dict(LM, kv_heads=1))
    with pytest.raises(ValueError):
        mqa.init_cache(2, 16, sharding=NamedSharding(mesh, P(None, None, "model")))
