"""decode.hip at head dim 128 on a real MI355X: ``attn_decode`` against the float64 oracle of tests/attn_oracle.py
(per sequence, held by ``AO.check`` / ``AO.check_lse``) under forced plans with lengths on the 16-key tile edges;
poisoned tails and determinism; ``attn_extend`` against stacked ``attn_decode`` calls, ``kv_append`` against
``hip.rope`` (and ``quantize_mx_ref`` of it) and the MX-fp8 attention against the bf16 one on the dequantised cache,
all bit for bit; what the descriptor refuses."""
import pytest
import torch

import attn_oracle as AO

pytestmark = pytest.mark.gpu

D, SCALE, CAP, THETA = 128, 128 ** -0.5, 256, 10000.0
BF16, U8 = torch.bfloat16, torch.uint8
PLANS = [(1, 256), (4, 64), (8, 32)]
HEADS = [(8, 8), (8, 2), (8, 1), (16, 1)]
LENS = [[0, 1, 15, 16], [17, 31, 32, 33], [63, 64, 65, 255]]      # extra = 1: n_b = lens + 1
INVALID = 1      # hipErrorInvalidValue


def _hip():
    from learning_jax_sharding_amd.ops import hip
    return hip


@pytest.fixture(autouse=True)
def _default_plan():
    yield
    _hip().set_decode_splits(None)


_CASES = {}


def _case(kind, B, H, Hkv, ns):
    """Inputs (bf16, CPU) and the per-sequence oracle / model / f32 reference for key counts ``ns``, computed once."""
    key = (kind, B, H, Hkv, tuple(ns))
    if key not in _CASES:
        q, k, v, _ = AO.inputs(kind, B, H, 1, CAP, SCALE, D=D)
        k, v = k[:, :, :Hkv].contiguous(), v[:, :, :Hkv].contiguous()
        per = []
        for b, n in enumerate(ns):
            if n == 0:
                per.append(None)
                continue
            qb = q[b:b + 1]
            kb, vb = (t[b:b + 1, :n].repeat_interleave(H // Hkv, 2) for t in (k, v))
            o, lse = AO.forward(qb, kb, vb, SCALE)
            per.append((o, lse, AO.forward(qb, kb, vb, SCALE, rounded=True)[0], AO.lse2_f32(qb, kb, SCALE)))
        _CASES[key] = (q, k, v, per)
    return _CASES[key]


def _check(name, o, lse, per):
    o, lse = o.cpu(), lse.cpu()
    for b, ref in enumerate(per):
        if ref is None:      # no key: o = 0, lse2 = +inf
            assert torch.equal(o[b], torch.zeros_like(o[b])) and torch.isposinf(lse[b]).all(), name
            continue
        AO.check(f"{name} b{b} o", o[b:b + 1], ref[0], ref[2])
        AO.check_lse(lse[b:b + 1], ref[1], ref[3], name=f"{name} b{b} lse")


def _run(q, k, v, lens, extra=1):
    o, lse = _hip().attn_decode(q.cuda(), k.cuda(), v.cuda(), torch.tensor(lens, dtype=torch.int32).cuda(), SCALE, extra)
    torch.cuda.synchronize()
    assert o.shape == (q.shape[0], 1, q.shape[2], D) and lse.shape == (q.shape[0], q.shape[2], 1)
    return o, lse


@pytest.mark.parametrize("H,Hkv", HEADS, ids=[f"h{h}kv{k}" for h, k in HEADS])
@pytest.mark.parametrize("plan", PLANS, ids=[f"{n}x{k}" for n, k in PLANS])
def test_decode_matches_oracle(plan, H, Hkv):
    hip = _hip()
    hip.set_decode_splits(*plan)
    for lens in LENS:
        for kind in AO.KINDS:
            q, k, v, per = _case(kind, 4, H, Hkv, [n + 1 for n in lens])
            with hip.launch_log() as log:
                o, lse = _run(q, k, v, lens)
            want = [f"attn_decode128<G{H // Hkv}>"] + (["decode_merge128"] if plan[0] > 1 else [])
            assert [r["name"] for r in log] == want and log[0]["grid"] == (plan[0], Hkv, 4), log
            _check(f"decode128 {plan} H{H}/{Hkv} {kind} lens{lens}", o, lse, per)


@pytest.mark.parametrize("plan", PLANS, ids=[f"{n}x{k}" for n, k in PLANS])
def test_extra_zero_empty_and_full(plan):
    _hip().set_decode_splits(*plan)
    q, k, v, per = _case("plain", 2, 8, 2, [0, CAP])
    _check(f"extra0 {plan}", *_run(q, k, v, [0, CAP], extra=0), per)


@pytest.mark.parametrize("plan", PLANS, ids=[f"{n}x{k}" for n, k in PLANS])
def test_poisoned_tail_and_determinism(plan):
    """Rows at and beyond n_b filled with NaN, +Inf and 3e38 give the bits of a zero tail; a second run gives equal bits."""
    _hip().set_decode_splits(*plan)
    lens = [0, 15, 16, 130]
    q, k, v, _ = _case("plain", 4, 8, 2, [1, 16, 17, 131])

    def tail(fill):
        kk, vv = k.clone(), v.clone()
        for b, n in enumerate(lens):
            kk[b, n + 1:] = fill
            vv[b, n + 1:] = fill
        return kk, vv

    base, again = _run(q, *tail(0.0), lens), _run(q, *tail(0.0), lens)
    assert torch.equal(base[0], again[0]) and torch.equal(base[1], again[1])
    for fill in (float("nan"), float("inf"), 3e38):
        got = _run(q, *tail(fill), lens)
        assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1]), fill


def _rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(BF16).cuda()


@pytest.mark.parametrize("G", [1, 2, 4, 8, 16])
@pytest.mark.parametrize("T", [2, 5, 16])
def test_extend_equals_stacked_decode(T, G):
    """Row (b, t, h) has the bits of ``attn_decode`` with ``extra = t + 1`` under the same plan; the last sequence's
    limits clamp at the capacity."""
    hip = _hip()
    hip.set_decode_splits(4, 64)
    B, Hkv = 3, (1 if G == 16 else 2)
    q, kc, vc = _rand((B, T, G * Hkv, D), 1), _rand((B, CAP, Hkv, D), 2), _rand((B, CAP, Hkv, D), 3)
    lt = torch.tensor([0, 47, CAP - 1], dtype=torch.int32).cuda()
    with hip.launch_log() as log:
        o, lse = hip.attn_extend(q, kc, vc, lt, SCALE)
    assert [r["name"].split("<")[0] for r in log] == ["attn_extend128", "decode_merge128"], log
    for t in range(T):
        ot, lt_ = hip.attn_decode(q[:, t:t + 1], kc, vc, lt, SCALE, t + 1)
        assert torch.equal(o[:, t:t + 1], ot) and torch.equal(lse[:, :, t:t + 1], lt_), t


def _fresh(kind, B, cap, Hkv, guard=0):
    """A cache of sentinels, ``guard`` rows allocated behind it: the views and the whole buffers."""
    shapes = [(D, BF16, 7.0)] * 2 if kind == "bf16" else [(D, U8, 0xAB)] * 2 + [(D // 32, U8, 0xAB)] * 2
    big = [torch.full((B, cap + guard, Hkv, n), fill, dtype=dt).cuda() for n, dt, fill in shapes]
    return [t[:, :cap] for t in big], big


@pytest.mark.parametrize("mode", ["lens", "host-base"])
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("kind", ["bf16", "mx8"])
def test_append_matches_rope(kind, T, mode):
    """k, v, q as column blocks of one fused buffer; rows at ``p = cap - 1`` (written) and ``p >= cap`` (not)."""
    from learning_jax_sharding_amd.ops import kernels as K
    hip = _hip()
    B, H, Hkv, cap = 4, 4, 2, 32
    lens = [0, 17, cap - 1, cap] if mode == "lens" else [0] * B
    fused = _rand((B, T, (H + 2 * Hkv) * D), 10 + T)
    q, k, v = (fused[..., a * D:b * D].view(B, T, -1, D) for a, b in ((0, H), (H, H + Hkv), (H + Hkv, H + 2 * Hkv)))
    cache, big = _fresh(kind, B, cap, Hkv, guard=4)
    lt = torch.tensor(lens, dtype=torch.int32).cuda() if mode == "lens" else None
    with hip.launch_log() as log:
        q_out = (hip.kv_append if kind == "bf16" else hip.kv_append_q8)(k, v, *cache, lt, q=q, theta=THETA)
    torch.cuda.synchronize()
    assert [r["name"] for r in log] == ["kv_append128<rot,q>" if kind == "bf16" else "kv_append128<rot,q,mx8>"], log
    want, _ = _fresh(kind, B, cap, Hkv)
    for b, n in enumerate(lens):
        for t in range(T):
            p = n + t
            if p >= cap:
                assert (q_out[b, t] == 0).all(), (b, t)
                continue
            kr, _ = hip.rope(k[b:b + 1, t:t + 1].contiguous(), None, pos_offset=p, theta=THETA)
            qr, _ = hip.rope(q[b:b + 1, t:t + 1].contiguous(), None, pos_offset=p, theta=THETA)
            assert torch.equal(q_out[b, t], qr[0, 0]), (b, t)
            rows = (kr[0, 0], v[b, t])
            if kind == "mx8":
                kq, vq = K._mx_bytes(rows[0][None]), K._mx_bytes(rows[1][None])
                rows = (kq[0][0], vq[0][0], kq[1][0], vq[1][0])
            for w, r in zip(want, rows):
                w[b, p] = r
    for name, got, w, whole in zip(("kc", "vc", "kcs", "vcs"), cache, want, big):
        assert torch.equal(got, w), name                        # appended rows, and sentinels everywhere else
        assert (whole[:, cap:] == whole[0, cap, 0, 0]).all(), name    # nothing behind the cache


@pytest.mark.parametrize("plan", [(1, 256), (4, 64)], ids=["1x256", "4x64"])
def test_q8_attention_is_bf16_attention_on_the_dequantised_cache(plan):
    from learning_jax_sharding_amd.ops import kernels as K
    hip = _hip()
    hip.set_decode_splits(*plan)
    B, H, Hkv, T = 3, 8, 2, 3
    cache, _ = _fresh("mx8", B, CAP, Hkv)
    hip.kv_append_q8(_rand((B, CAP, Hkv, D), 4), _rand((B, CAP, Hkv, D), 5), *cache, None, theta=THETA)
    kd, vd = K.mx_cache_dequant(cache[0], cache[2]), K.mx_cache_dequant(cache[1], cache[3])
    q = _rand((B, T, H, D), 6)
    lt = torch.tensor([0, 100, CAP - 2], dtype=torch.int32).cuda()
    with hip.launch_log() as log:
        got = hip.attn_decode_q8(q[:, :1], *cache, lt, SCALE, 1) + hip.attn_extend_q8(q, *cache, lt, SCALE)
    names = [r["name"] for r in log if not r["name"].startswith("decode_merge128")]
    assert names == ["attn_decode128<G4,mx8>", "attn_extend128<G4,P2,mx8>"], log
    want = hip.attn_decode(q[:, :1], kd, vd, lt, SCALE, 1) + hip.attn_extend(q, kd, vd, lt, SCALE)
    for g, w in zip(got, want):
        assert torch.equal(g, w)


def test_descriptor_refusals():
    """A head dim that is neither 64 nor 128 is refused by every entry, a 128 descriptor by ``ljs_attn_chunk`` and a scale
    buffer off the 4-byte rule by the MX-fp8 entries, all with nothing launched."""
    hip = _hip()
    cap = 16
    z = lambda *s, dt=BF16: torch.zeros(*s, dtype=dt).cuda()   # noqa: E731
    q, o, lse, lens = z(1, 1, 1, D), z(1, 1, 1, D), z(1, 1, 1, dt=torch.float32), z(1, dt=torch.int32)
    kc, k8, ks = z(1, cap, 1, D), z(1, cap, 1, D, dt=U8), z(1, cap, 1, 4, dt=U8)
    off = z(cap * 4 + 4, dt=U8)[2:2 + cap * 4].view(1, cap, 1, 4)       # a 2-byte aligned base
    entries = {"kv_append": lambda d: hip._kv_append_desc(d, q, q, lens),
               "attn_decode": lambda d: hip._attn_decode_desc(d, q, o, lse, None, lens, SCALE, 1),
               "attn_chunk": lambda d: hip._attn_chunk_desc(d, q, o, lse, lens, SCALE)}
    good = {"bf16": lambda: hip._cache_desc(hip.CACHE_BF16, kc, kc), "mx8": lambda: hip._cache_desc(hip.CACHE_MX8, k8, k8, ks, ks)}
    assert good["bf16"]().dim == D
    bad = [(e, d) for e in entries for d in ("bf16-96", "mx8-96")] + [("attn_chunk", "bf16"), ("attn_chunk", "mx8")] \
        + [("kv_append", "mx8-off"), ("attn_decode", "mx8-off")]
    for entry, which in bad:
        desc = good[which.split("-")[0]]() if which != "mx8-off" else hip._cache_desc(hip.CACHE_MX8, k8, k8, off, ks)
        if which.endswith("96"):
            desc.dim = 96
        with hip.launch_log() as log:
            assert entries[entry](desc) == INVALID, (entry, which)
        assert log.total == 0, (entry, which, log)
    with hip.launch_log() as log:                                   # the good descriptors launch
        assert [entries[e](good[k]()) for e in ("kv_append", "attn_decode") for k in good] == [0] * 4
    assert [r["name"] for r in log] == ["kv_append128<copy>", "kv_append128<copy,mx8>", "attn_decode128<G1>",
                                        "attn_decode128<G1,mx8>"], log
    torch.cuda.synchronize()
