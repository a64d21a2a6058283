"""Rotary position embedding on host devices: the torch formulation (ops/kernels.py rope_reference,
the semantics the HIP kernel shares) against the float64 oracle of tests/rope_oracle.py, the sharded
``core.rope``, the table cache, and the ``causal`` / ``rope_theta`` fields of the model classes."""
import numpy as np
import pytest
import torch

import rope_oracle as O

F32, BF16 = torch.float32, torch.bfloat16
THETA = 10000.0
SHAPE = (2, 37, 3)
COMBOS = [(D, off) for D in (16, 64, 256) for off in (0, 1000, 100000)]


def _qk(D, dtype, seed=0, shape=SHAPE):
    gen = torch.Generator().manual_seed(seed + D)
    q = torch.randn(*shape, D, generator=gen).to(dtype)
    k = torch.randn(*shape, D, generator=gen).to(dtype)
    return q, k


# ------------------------------------------------------------------------------------ reference
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("D,off", COMBOS, ids=[f"D{D}-off{off}" for D, off in COMBOS])
def test_reference_matches_float64_oracle(D, off, dtype):
    """Forward and (through autograd) backward of the torch formulation, q and k, under the f32 /
    bf16 bounds of rope_oracle; an f32 output from bf16 inputs as well."""
    from learning_jax_sharding_amd.ops import kernels as K
    q, k = _qk(D, dtype)
    gq, gk = _qk(D, dtype, seed=100)
    qs, ks = q.clone().requires_grad_(True), k.clone().requires_grad_(True)
    qo, ko = K.rope_reference(qs, ks, off, THETA)
    assert qo.dtype == dtype and ko.dtype == dtype
    dq, dk = torch.autograd.grad([qo, ko], [qs, ks], [gq, gk])
    tag = f"ref D={D} off={off}"
    O.check(f"{tag} q'", qo, *O.rotate64(q, off, THETA))
    O.check(f"{tag} k'", ko, *O.rotate64(k, off, THETA))
    O.check(f"{tag} dq", dq, *O.rotate64(gq, off, THETA, inverse=True))
    O.check(f"{tag} dk", dk, *O.rotate64(gk, off, THETA, inverse=True))
    if dtype == BF16:
        q32, none = K.rope_reference(q, None, off, THETA, out_dtype=F32)
        assert none is None and q32.dtype == F32
        O.check(f"{tag} q' bf16->f32", q32, *O.rotate64(q, off, THETA))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_position_zero_is_the_identity(dtype):
    from learning_jax_sharding_amd.ops import kernels as K
    q, k = _qk(64, dtype)
    qo, ko = K.rope_reference(q, k, 0, THETA)
    assert torch.equal(qo[:, 0], q[:, 0]) and torch.equal(ko[:, 0], k[:, 0])
    assert not torch.equal(qo[:, 1], q[:, 1])


def test_scores_depend_on_relative_position_only():
    """q'.k'^T is unchanged when every position moves by 17.  Each rotated element is within EPS m of
    the exact rotation (the f32 bound), and exact rotations give equal scores, so two runs differ by
    at most the sum over both of EPS (m_q.|k'| + |q'|.m_k), with 1 % for the second-order terms; the
    dot products themselves are taken in float64."""
    from learning_jax_sharding_amd.ops import kernels as K
    q, k = _qk(64, F32)
    runs = []
    for off in (0, 17):
        qo, ko = K.rope_reference(q, k, off, THETA)
        mq, mk = O.rotate64(q, off, THETA)[1], O.rotate64(k, off, THETA)[1]
        s = torch.einsum("bqhd,bkhd->bhqk", qo.double(), ko.double())
        bound = O.EPS_F32 * (torch.einsum("bqhd,bkhd->bhqk", mq, ko.double().abs())
                             + torch.einsum("bqhd,bkhd->bhqk", qo.double().abs(), mk))
        runs.append((s, bound))
    diff = (runs[0][0] - runs[1][0]).abs()
    allowed = 1.01 * (runs[0][1] + runs[1][1])
    print(f"rope-figures relative max|diff|={diff.max():.3e} worst_fraction_of_bound={(diff / allowed).max():.3f}")
    assert (diff <= allowed).all()
    # and the scores do depend on the relative position: rotating k alone by 17 more moves them
    k17 = K.rope_reference(k, None, 17, THETA)[0]
    s17 = torch.einsum("bqhd,bkhd->bhqk", K.rope_reference(q, None, 0, THETA)[0].double(), k17.double())
    assert ((s17 - runs[0][0]).abs() > allowed).any()


# ------------------------------------------------------------------------------------ core.rope
def _put(x, mesh_shape, spec):
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd.mesh import Mesh, create_device_mesh
    from learning_jax_sharding_amd.sharding import NamedSharding, PartitionSpec as P
    mesh = Mesh(create_device_mesh(mesh_shape), ("data", "model"))
    return ljs.device_put(x.numpy(), NamedSharding(mesh, P(*spec)))


LAYOUTS = [((1, 2), (None, "model")), ((1, 4), (None, "model")), ((2, 2), ("data", "model")),
           ((2, 2), (None, "model", None, "data"))]


@pytest.mark.parametrize("mesh_shape,spec", LAYOUTS, ids=["len2", "len4", "batch2xlen2", "len2xdim2"])
def test_sharded_rope_equals_one_device(host_devices, mesh_shape, spec):
    """core.rope over length, over batch x length and with head_dim sharded (resharded whole first):
    bit for bit the one-device result, each shard rotated from the start of its length region, one
    ``rope`` plan step, no collective for a whole head_dim."""
    from learning_jax_sharding_amd.ops import core
    from learning_jax_sharding_amd.ops import kernels as K
    from learning_jax_sharding_amd.spmd import plan as _plan
    q, k = _qk(32, F32, shape=(4, 24, 2))
    host_devices(1)
    q1, k1 = core.rope(_put(q, (1, 1), ()), _put(k, (1, 1), ()), theta=THETA)
    one_q, one_k = q1.to_torch(), k1.to_torch()
    assert torch.equal(one_q, K.rope_reference(q, None, 0, THETA)[0])
    host_devices(int(np.prod(mesh_shape)))
    seen = []
    real = K.rope
    qs, ks = _put(q, mesh_shape, spec), _put(k, mesh_shape, spec)
    K.rope = lambda a, b=None, pos_offset=0, *r, **kw: (seen.append(pos_offset), real(a, b, pos_offset, *r, **kw))[1]
    try:
        with _plan.record_plan() as rec:
            qn, kn = core.rope(qs, ks, theta=THETA)
            only_q = core.rope(qs, theta=THETA)
    finally:
        K.rope = real
    steps = [s for s in rec.steps if s.kind == "rope"]
    assert len(steps) == 2 and steps[0].info["tensors"] == 2 and steps[0].info["joint"]
    assert steps[1].info["tensors"] == 1
    assert steps[0].info["tiles"][3] == 1
    sharded_dim = len(spec) == 4
    assert [s.kind for s in rec.steps if s.kind != "rope"] == [] or sharded_dim
    assert qn.tile.tile_shape[:3] == qs.tile.tile_shape[:3] and qn.tile.tile_shape[3] == 1
    nlen = qs.tile.tile_shape[1]
    assert sorted(set(seen)) == [i * (24 // nlen) for i in range(nlen)], seen
    for d in qn.local:
        assert seen.count(qn.tile.region(d, qn.shape)[1][0]) >= 2
    assert torch.equal(qn.to_torch(), one_q) and torch.equal(kn.to_torch(), one_k)
    assert torch.equal(only_q.to_torch(), one_q)


def test_rope_argument_errors(host_devices):
    from learning_jax_sharding_amd.ops import core
    host_devices(1)
    with pytest.raises(ValueError):
        core.rope(_put(torch.zeros(2, 3, 4), (1, 1), ()))
    with pytest.raises(ValueError):
        core.rope(_put(torch.zeros(2, 3, 4, 5), (1, 1), ()))


# ------------------------------------------------------------------------------------ table cache
def test_table_cache_grows_by_doubling_and_keeps_old_tables():
    from learning_jax_sharding_amd.ops import kernels as K
    cache, cpu = K.RopeTableCache(), torch.device("cpu")
    c0, s0 = cache.get(cpu, 64, THETA, 10)
    assert c0.dtype == F32 and tuple(c0.shape) == tuple(s0.shape) == (1024, 32)
    assert cache.get(cpu, 64, THETA, 1024)[0] is c0 and not cache.superseded
    c1, s1 = cache.get(cpu, 64, THETA, 1025)
    assert tuple(c1.shape) == (2048, 32)
    assert torch.equal(c1[:1024], c0) and torch.equal(s1[:1024], s0)
    assert len(cache.superseded) == 1 and cache.superseded[0][0] is c0 and cache.superseded[0][1] is s0
    c2, _ = cache.get(cpu, 64, THETA, 9000)
    assert tuple(c2.shape) == (16384, 32) and len(cache.superseded) == 2
    assert cache.get(cpu, 64, THETA, 3)[0] is c2
    # another head_dim or theta is another table
    assert tuple(cache.get(cpu, 16, THETA, 1)[0].shape) == (1024, 8)
    assert not torch.equal(cache.get(cpu, 64, 500.0, 1)[0], c2[:1024])
    # the float64 formula, rounded once
    p = np.arange(16384, dtype=np.float64)[:, None]
    ang = p * np.power(np.float64(THETA), -2.0 * np.arange(32, dtype=np.float64) / 64)[None, :]
    assert np.array_equal(c2.numpy(), np.cos(ang).astype(np.float32))
    assert np.array_equal(cache.get(cpu, 64, THETA, 3)[1].numpy(), np.sin(ang).astype(np.float32))
    assert np.array_equal(K.rope_table_host(5, 64, THETA, start=7)[0].numpy(), np.cos(ang[7:12]).astype(np.float32))


def test_table_is_not_created_during_a_graph_capture(monkeypatch):
    """Under a capture a table that is long enough is handed out, a missing or too short one raises
    (the capture would record the upload and hold an address nothing keeps alive on purpose)."""
    from learning_jax_sharding_amd.ops import kernels as K
    cache, gpu = K.RopeTableCache(), torch.device("cuda", 0)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="graph capture"):
        cache.get(gpu, 64, THETA, 10)
    have = K.rope_table_host(1024, 64, THETA)          # stands in for a table made by a warm-up call
    cache.live[K.RopeTableCache._key(gpu, 64, THETA)] = have
    assert cache.get(gpu, 64, THETA, 1024)[0] is have[0]
    with pytest.raises(RuntimeError, match="1024 rows and 1025 are needed"):
        cache.get(gpu, 64, THETA, 1025)
    assert not cache.superseded


def test_rope_dispatch_on_host_tensors(monkeypatch):
    """Host tensors take the torch formulation whatever LJS_FUSED_ROPE says, with no warning."""
    import warnings
    from learning_jax_sharding_amd.ops import kernels as K
    q, k = _qk(24, F32)
    for v in ("0", "1"):
        monkeypatch.setenv("LJS_FUSED_ROPE", v)
        assert K.fused_rope_enabled() == (v == "1")
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            qo, ko = K.rope(q, k, 3, THETA)
        assert torch.equal(qo, K.rope_reference(q, None, 3, THETA)[0])
        assert K.rope(q, None, 3, THETA)[1] is None


def test_rope_instances_use_no_scratch():
    """Every instance of the rope kernel is in the gfx950 code object (f32 / bf16 in x f32 / bf16 out x
    forward / inverse = 8), uses no scratch and no LDS, spills nothing, and stays within 64 VGPRs (8
    waves per SIMD)."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "learning_jax_sharding_amd", "_lib", "libljs_kernels.so")
    if not os.path.exists(lib):
        from learning_jax_sharding_amd.csrc import build
        build.build_all()
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(root, "scripts",
                                                                                   "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    res = {n: k for n, k in kr.resources(lib).items() if "rope_kernel" in n}
    assert len(res) == 8, sorted(res)
    for n, k in res.items():
        assert k.get("scratch", 0) == 0 and k.get("vgpr_spill", 0) == 0 and k.get("sgpr_spill", 0) == 0, (n, k)
        assert k.get("lds", 0) == 0 and k["vgpr"] <= 64, (n, k)


# ------------------------------------------------------------------------------------ models
LM = dict(vocab_size=64, dim=32, layers=2, heads=2, dim_head=16)


def _logits(lm, tok):
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd.models import TransformerLM
    model = TransformerLM(**lm)
    ids = ljs.device_put(tok.numpy())
    params = model.init(ljs.random.PRNGKey(1), ids)["params"]
    return model.apply({"params": params}, ids).to_torch().float()


def test_causal_lm_does_not_see_the_future(host_devices):
    """Changing the token at position 7 leaves the causal + RoPE model's logits at positions < 7 where
    they were (1e-6 max|logits|; bit-equal is expected and printed) and moves a logit at a position
    >= 7 by more than 1e-3 max|logits|.  Control: without ``causal`` the same change moves a logit at a
    position < 7, so the test can fail."""
    host_devices(1)
    tok = torch.randint(0, 64, (2, 12), generator=torch.Generator().manual_seed(5))
    tok2 = tok.clone()
    tok2[:, 7] = (tok[:, 7] + 13) % 64
    for causal in (True, False):
        lm = dict(LM, causal=causal, rope_theta=1e4)
        a, b = _logits(lm, tok), _logits(lm, tok2)
        scale = a.abs().max().item()
        before, after = (a[:, :7] - b[:, :7]).abs().max().item(), (a[:, 7:] - b[:, 7:]).abs().max().item()
        print(f"rope-figures causal={causal} max|logits|={scale:.4g} moved before 7: {before:.3g} (bit-equal: "
              f"{torch.equal(a[:, :7], b[:, :7])}), from 7 on: {after:.3g}")
        assert after > 1e-3 * scale
        if causal:
            assert before <= 1e-6 * scale
        else:
            assert before > 1e-3 * scale


def test_default_fields_change_nothing(host_devices):
    host_devices(1)
    tok = torch.randint(0, 64, (2, 12), generator=torch.Generator().manual_seed(5))
    base = _logits(dict(LM, max_len=12), tok)
    assert torch.equal(base, _logits(dict(LM, max_len=12, causal=False, rope_theta=None), tok))
    # and each field does something
    assert not torch.equal(_logits(LM, tok), _logits(dict(LM, rope_theta=1e4), tok))
    assert not torch.equal(_logits(LM, tok), _logits(dict(LM, causal=True), tok))


@pytest.mark.parametrize("impl", ["fused", "einsum"])
def test_attention_formulations_agree(host_devices, impl):
    """A causal + RoPE MultiHeadAttention in f32: ``impl='einsum'`` (mask before its softmax) and
    ``impl='fused'`` give the same block output, and it equals a direct evaluation from the parameters."""
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd import nn
    from learning_jax_sharding_amd.models import MultiHeadAttention
    from learning_jax_sharding_amd.ops import kernels as K
    host_devices(1)
    model = MultiHeadAttention(32, heads=2, dim_head=16, dtype=F32, impl=impl, causal=True, rope_theta=1e4)
    x = ljs.random.normal(ljs.random.PRNGKey(0), (2, 10, 32))
    params = model.init(ljs.random.PRNGKey(1), x)["params"]
    got = model.apply({"params": params}, x).to_torch()
    p = ljs.tree_map(lambda a: a.to_torch(), nn.unbox(params))
    xt = x.to_torch()
    q, k, v = ((xt @ p[n]["kernel"]).view(2, 10, 2, 16) for n in ("to_q", "to_k", "to_v"))
    q, k = K.rope_reference(q, k, 0, 1e4)
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) * 16 ** -0.5
    s = s.masked_fill(torch.arange(10)[None, :] > torch.arange(10)[:, None], float("-inf"))
    o = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, -1), v).reshape(2, 10, 32)
    want = o @ p["to_out_0"]["kernel"] + p["to_out_0"]["bias"]
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-5, atol=1e-5 * want.abs().max().item())


def test_causal_rope_lm_on_a_mesh_matches_one_device(host_devices):
    """The causal + RoPE LM step on a (2, 2) host mesh under VOCAB_PARALLEL_RULES against (1, 1): the
    bound tests/test_embed.py test_transformer_lm_step puts on the existing model, 1e-5 max(1, |loss|)."""
    from test_embed import lm_step
    lm = dict(LM, causal=True, rope_theta=1e4)
    host_devices(1)
    logits1, one, g1, *_ = lm_step((1, 1), lm)
    host_devices(4)
    logits4, val, g4, *_ = lm_step((2, 2), lm)
    print(f"rope-lm loss 1-device={one:.8g} 2x2={val:.8g} diff={abs(one - val):.3g}")
    assert tuple(logits4.shape) == (4, 16, 64) and np.isfinite(val)
    assert abs(val - one) <= 1e-5 * max(1.0, abs(one)), (val, one)
    assert set(g1) == set(g4) and "pos_embed/embedding" not in g4
    for name, g in g4.items():
        assert np.isfinite(g).all(), name


def test_model_errors(host_devices):
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd.models import MultiHeadAttention, TransformerLM
    host_devices(1)
    ids = ljs.device_put(np.zeros((2, 8), dtype=np.int64))
    with pytest.raises(ValueError, match="max_len"):
        TransformerLM(**LM, rope_theta=1e4, max_len=8).init(ljs.random.PRNGKey(1), ids)
    x = ljs.random.normal(ljs.random.PRNGKey(0), (2, 8, 32))
    attn = MultiHeadAttention(32, heads=2, dim_head=16, rope_theta=1e4)
    params = attn.init(ljs.random.PRNGKey(1), x)["params"]
    with pytest.raises(ValueError, match="context"):
        attn.apply({"params": params}, x, x)


def test_attention_next_hint_only_for_the_plain_module(host_devices, monkeypatch):
    """The fused projection + forward kernel is non-causal and takes un-rotated q / k: the hint that
    lets the QKV dense run it is given for the default module and never with ``causal`` or ``rope_theta``."""
    import contextlib
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd.models import MultiHeadAttention
    from learning_jax_sharding_amd.ops import linear as L
    host_devices(1)
    entered = []

    @contextlib.contextmanager
    def recording(heads, dim_head, scale):
        entered.append((heads, dim_head))
        yield

    monkeypatch.setattr(L, "attention_next", recording)
    x = ljs.random.normal(ljs.random.PRNGKey(0), (2, 256, 128))
    counts = {}
    for name, kw in (("plain", {}), ("causal", dict(causal=True)), ("rope", dict(rope_theta=1e4)),
                     ("both", dict(causal=True, rope_theta=1e4))):
        model = MultiHeadAttention(128, heads=2, dim_head=64, **kw)
        params = model.init(ljs.random.PRNGKey(1), x)["params"]
        del entered[:]
        model.apply({"params": params}, x)
        counts[name] = len(entered)
    assert counts == {"plain": 1, "causal": 0, "rope": 0, "both": 0}, counts
