"""The decode kernels of csrc/kernels/decode.hip on a real MI355X: ``attn_decode`` against the float64
oracle of tests/attn_oracle.py (per sequence, ``forward(q, k[:n_b], v[:n_b], causal=False)``, held by
``AO.check`` / ``AO.check_lse``), under forced split plans and the default plan; poisoned cache tails,
determinism and strided operands bit for bit; ``kv_append`` against ``hip.rope`` bit for bit, its bounds
and its host-base mode; the launch log; the G > 16 fallback."""
import warnings

import pytest
import torch

import attn_oracle as AO

pytestmark = pytest.mark.gpu

SCALE = 0.125
CAP = 512
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
PLANS = [(1, 512), (4, 128), (8, 64)]
HEADS = [(8, 8), (8, 2), (8, 1), (16, 1)]
LENS = [[0, 1, 15, 16], [17, 63, 64, 65], [127, 128, 129, 511]]      # extra = 1: n_b = lens + 1
INVALID = 1      # hipErrorInvalidValue


def _hip():
    from learning_jax_sharding_amd.ops import hip
    return hip


@pytest.fixture(autouse=True)
def _default_plan():
    yield
    _hip().set_decode_splits(None)


_CASES = {}


def _case(kind, B, H, Hkv, cap, ns):
    """Inputs (bf16, CPU) and the per-sequence oracle / model / f32 reference for key counts ``ns``,
    computed once and left unchanged."""
    key = (kind, B, H, Hkv, cap, tuple(ns))
    if key not in _CASES:
        q, k, v, _ = AO.inputs(kind, B, H, 1, cap, SCALE)
        k, v = k[:, :, :Hkv].contiguous(), v[:, :, :Hkv].contiguous()
        G = H // Hkv
        per = []
        for b, n in enumerate(ns):
            if n == 0:
                per.append(None)
                continue
            qb = q[b:b + 1]
            kb = k[b:b + 1, :n].repeat_interleave(G, 2)
            vb = v[b:b + 1, :n].repeat_interleave(G, 2)
            o, lse = AO.forward(qb, kb, vb, SCALE)
            mo, _ = AO.forward(qb, kb, vb, SCALE, rounded=True)
            per.append((o, lse, mo, AO.lse2_f32(qb, kb, SCALE)))
        _CASES[key] = (q, k, v, per)
    return _CASES[key]


def _check(name, o, lse, per):
    o, lse = o.cpu(), lse.cpu()
    for b, ref in enumerate(per):
        if ref is None:      # no key: o = 0, lse2 = +inf
            assert torch.equal(o[b], torch.zeros_like(o[b])), name
            assert torch.isposinf(lse[b]).all(), name
            continue
        want_o, want_lse, model_o, ref32 = ref
        AO.check(f"{name} b{b} o", o[b:b + 1], want_o, model_o)
        AO.check_lse(lse[b:b + 1], want_lse, ref32, name=f"{name} b{b} lse")


def _run(q, k, v, lens, extra=1):
    hip = _hip()
    lt = torch.tensor(lens, dtype=torch.int32).cuda()
    o, lse = hip.attn_decode(q.cuda(), k.cuda(), v.cuda(), lt, SCALE, extra)
    torch.cuda.synchronize()
    assert o.shape == (q.shape[0], 1, q.shape[2], 64) and o.dtype == BF16
    assert lse.shape == (q.shape[0], q.shape[2], 1) and lse.dtype == F32
    return o, lse


# ----------------------------------------------------------------------------- attn_decode vs the oracle
@pytest.mark.parametrize("H,Hkv", HEADS, ids=[f"h{h}kv{k}" for h, k in HEADS])
@pytest.mark.parametrize("plan", PLANS, ids=[f"{n}x{k}" for n, k in PLANS])
def test_decode_matches_oracle(plan, H, Hkv):
    hip = _hip()
    hip.set_decode_splits(*plan)
    for lens in LENS:
        for kind in AO.KINDS:
            q, k, v, per = _case(kind, 4, H, Hkv, CAP, [n + 1 for n in lens])
            with hip.launch_log() as log:
                o, lse = _run(q, k, v, lens)
            dec = [r for r in log if r["name"].startswith("attn_decode<")]
            assert len(dec) == 1 and dec[0]["grid"] == (plan[0], Hkv, 4) and dec[0]["block"] == 256, log
            assert dec[0]["name"] == f"attn_decode<G{H // Hkv}>", dec
            assert [r["name"] for r in log if r is not dec[0]] == (["decode_merge"] if plan[0] > 1 else []), log
            _check(f"decode {plan} H{H}/{Hkv} {kind} lens{lens}", o, lse, per)


def test_extra_zero_empty_and_full():
    """``extra = 0``: a sequence without any key (o = 0, lse2 = +inf) next to a full cache."""
    hip = _hip()
    q, k, v, per = _case("plain", 2, 8, 2, CAP, [0, CAP])
    for plan in PLANS:
        hip.set_decode_splits(*plan)
        o, lse = _run(q, k, v, [0, CAP], extra=0)
        _check(f"extra0 {plan}", o, lse, per)


def test_default_plan_long_cache():
    """The plan function's own plan at cap = 4096 with lengths up to 4095."""
    hip = _hip()
    cap, lens = 4096, [4095, 2000]
    q, k, v, per = _case("plain", 2, 8, 2, cap, [n + 1 for n in lens])
    splits, keys = hip.plan_decode(2, 2, cap)
    assert splits > 1 and splits * keys >= cap and keys % hip.decode_key_tile() == 0
    with hip.launch_log() as log:
        o, lse = _run(q, k, v, lens)
    assert [r["name"] for r in log] == ["attn_decode<G4>", "decode_merge"] and log[0]["grid"] == (splits, 2, 2), log
    _check("default plan cap4096", o, lse, per)


# ----------------------------------------------------------------------------- bits
@pytest.mark.parametrize("plan", PLANS, ids=[f"{n}x{k}" for n, k in PLANS])
def test_poisoned_tail_and_determinism(plan):
    """Rows at and beyond n_b filled with NaN, +Inf and 3e38 give the bits of a zero tail; two runs of
    the same call give equal bits."""
    hip = _hip()
    hip.set_decode_splits(*plan)
    lens = [0, 17, 129, 300]
    q, k, v, _ = _case("plain", 4, 8, 2, CAP, [1, 18, 130, 301])

    def tail(fill):
        kk, vv = k.clone(), v.clone()
        for b, n in enumerate(lens):
            kk[b, n + 1:] = fill
            vv[b, n + 1:] = fill
        return kk, vv

    base = _run(q, *tail(0.0), lens)
    again = _run(q, *tail(0.0), lens)
    assert torch.equal(base[0], again[0]) and torch.equal(base[1], again[1])
    for fill in (float("nan"), float("inf"), 3e38):
        got = _run(q, *tail(fill), lens)
        assert torch.isfinite(got[0]).all(), fill
        assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1]), fill


def test_strided_operands():
    """kc / vc as the two column blocks of one buffer and q a view of a wider buffer: the contiguous
    run's bits."""
    hip = _hip()
    hip.set_decode_splits(4, 128)
    B, H, Hkv = 4, 8, 2
    lens = [3, 64, 200, 511]
    q, k, v, _ = _case("plain", B, H, Hkv, CAP, [4, 65, 201, 512])
    base = _run(q, k, v, lens)
    kv = torch.empty(B, CAP, 2 * Hkv * 64, dtype=BF16).cuda()
    kv[..., :Hkv * 64] = k.cuda().view(B, CAP, Hkv * 64)
    kv[..., Hkv * 64:] = v.cuda().view(B, CAP, Hkv * 64)
    kc = kv[..., :Hkv * 64].view(B, CAP, Hkv, 64)
    vc = kv[..., Hkv * 64:].view(B, CAP, Hkv, 64)
    wide = torch.zeros(B, 1, H * 64 + 64, dtype=BF16).cuda()
    wide[..., :H * 64] = q.cuda().view(B, 1, H * 64)
    qv = wide[..., :H * 64].view(B, 1, H, 64)
    assert not kc.is_contiguous() and not qv.is_contiguous() and kc.stride(1) == 2 * Hkv * 64
    got = hip.attn_decode(qv, kc, vc, torch.tensor(lens, dtype=torch.int32).cuda(), SCALE, 1)
    torch.cuda.synchronize()
    assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1])


def test_bad_arguments_launch_nothing():
    hip = _hip()
    q = torch.zeros(2, 1, 8, 64, dtype=BF16).cuda()
    kc = torch.zeros(2, 64, 2, 64, dtype=BF16).cuda()
    o, lse = torch.empty_like(q), torch.empty(2, 8, 1).cuda()
    lens = torch.zeros(2, dtype=torch.int32).cuda()
    ws = torch.empty(1 << 16).cuda()
    n0 = hip.lib().ljs_launch_count()
    assert hip.attn_decode_raw(q, kc, kc, o, lse, ws, lens, -1.0) == INVALID              # scale <= 0
    assert hip.attn_decode_raw(q[:, :, :7], kc, kc, o, lse, ws, lens, SCALE) == INVALID    # 7 % 2 != 0
    mis = torch.zeros(2 * 64 * 2 * 64 + 8, dtype=BF16).cuda()[4:4 + 2 * 64 * 2 * 64].view(2, 64, 2, 64)
    assert hip.attn_decode_raw(q, mis, kc, o, lse, ws, lens, SCALE) == INVALID             # 8-byte aligned base
    hip.set_decode_splits(2, 48)                                                           # not a tile multiple
    assert hip.attn_decode_raw(q, kc, kc, o, lse, ws, lens, SCALE) == INVALID
    hip.set_decode_splits(None)
    assert hip.kv_append_raw(kc[:, :1], kc[:, :1], mis, kc, lens) == INVALID
    assert hip.lib().ljs_launch_count() == n0


# ----------------------------------------------------------------------------- kv_append
def _append_inputs(B, T, H, Hkv, seed=0):
    gen = torch.Generator().manual_seed(11 + seed)
    mk = lambda h: torch.randn(B, T, h, 64, generator=gen).to(BF16).cuda()   # noqa: E731
    return mk(H), mk(Hkv), mk(Hkv)


SENT = 7.0


def test_append_rotates_like_rope():
    """Rotated k and q_out equal ``hip.rope`` at ``pos_offset = lens[b]`` bit for bit, per sequence; v is
    copied exactly; every other row keeps its sentinel; exactly one launch."""
    hip = _hip()
    B, H, Hkv, cap, theta = 4, 8, 2, 64, 10000.0
    lens = [0, 5, 62, 63]
    q, k, v = _append_inputs(B, 1, H, Hkv)
    kc = torch.full((B, cap, Hkv, 64), SENT, dtype=BF16).cuda()
    vc = torch.full((B, cap, Hkv, 64), SENT, dtype=BF16).cuda()
    lt = torch.tensor(lens, dtype=torch.int32).cuda()
    with hip.launch_log() as log:
        q_out = hip.kv_append(k, v, kc, vc, lt, q=q, theta=theta)
    torch.cuda.synchronize()
    assert [r["name"] for r in log] == ["kv_append<rot,q>"], log
    assert torch.equal(lt.cpu(), torch.tensor(lens, dtype=torch.int32))
    for b, n in enumerate(lens):
        qr, _ = hip.rope(q[b:b + 1], None, pos_offset=n, theta=theta)
        kr, _ = hip.rope(k[b:b + 1], None, pos_offset=n, theta=theta)
        assert torch.equal(q_out[b:b + 1], qr), b
        assert torch.equal(kc[b, n], kr[0, 0]), b
        assert torch.equal(vc[b, n], v[b, 0]), b
        rest = torch.ones(cap, dtype=torch.bool)
        rest[n] = False
        assert (kc[b][rest.cuda()] == SENT).all() and (vc[b][rest.cuda()] == SENT).all(), b


def test_append_drops_rows_past_the_cache():
    """``lens[b] + T > cap``: guard rows allocated behind the cache keep their sentinel and the rows in
    range are still written."""
    hip = _hip()
    B, H, Hkv, cap, T, theta = 4, 8, 2, 32, 3, 10000.0
    lens = [cap - 1, cap - 2, 10, cap]
    q, k, v = _append_inputs(B, T, H, Hkv, seed=1)
    big_k = torch.full((B, cap + 8, Hkv, 64), SENT, dtype=BF16).cuda()
    big_v = torch.full((B, cap + 8, Hkv, 64), SENT, dtype=BF16).cuda()
    kc, vc = big_k[:, :cap], big_v[:, :cap]
    lt = torch.tensor(lens, dtype=torch.int32).cuda()
    q_out = hip.kv_append(k, v, kc, vc, lt, q=q, theta=theta)
    torch.cuda.synchronize()
    assert (big_k[:, cap:] == SENT).all() and (big_v[:, cap:] == SENT).all()
    for b, n in enumerate(lens):
        for t in range(T):
            p = n + t
            if p < cap:
                kr, _ = hip.rope(k[b:b + 1, t:t + 1], None, pos_offset=p, theta=theta)
                qr, _ = hip.rope(q[b:b + 1, t:t + 1], None, pos_offset=p, theta=theta)
                assert torch.equal(kc[b, p], kr[0, 0]) and torch.equal(vc[b, p], v[b, t]), (b, t)
                assert torch.equal(q_out[b, t], qr[0, 0]), (b, t)
            else:
                assert (q_out[b, t] == 0).all(), (b, t)
        written = [n + t for t in range(T) if n + t < cap]
        rest = torch.ones(cap, dtype=torch.bool)
        rest[written] = False
        assert (kc[b][rest.cuda()] == SENT).all(), b


@pytest.mark.parametrize("rot", [False, True], ids=["copy", "rot"])
def test_append_host_base_mode(rot):
    """Prefill: no lens, T = 9 rows to rows 0..8, as they are or rotated at positions 0..8."""
    hip = _hip()
    B, Hkv, cap, T, theta = 2, 2, 32, 9, 10000.0
    _, k, v = _append_inputs(B, T, 8, Hkv, seed=2)
    kc = torch.full((B, cap, Hkv, 64), SENT, dtype=BF16).cuda()
    vc = torch.full((B, cap, Hkv, 64), SENT, dtype=BF16).cuda()
    with hip.launch_log() as log:
        assert hip.kv_append(k, v, kc, vc, None, theta=theta if rot else None) is None
    torch.cuda.synchronize()
    assert [r["name"] for r in log] == ["kv_append<rot>" if rot else "kv_append<copy>"], log
    want_k = hip.rope(k, None, pos_offset=0, theta=theta)[0] if rot else k
    assert torch.equal(kc[:, :T], want_k) and torch.equal(vc[:, :T], v)
    assert (kc[:, T:] == SENT).all() and (vc[:, T:] == SENT).all()


def test_lens_add():
    hip = _hip()
    lt = torch.tensor([0, 7, 511], dtype=torch.int32).cuda()
    with hip.launch_log() as log:
        hip.lens_add(lt, 1)
    assert [r["name"] for r in log] == ["lens_add"] and lt.tolist() == [1, 8, 512]


# ----------------------------------------------------------------------------- fallback
def test_group_of_32_takes_the_fallback():
    """heads / kv_heads = 32 is beyond the kernel: the torch formulation on the GPU, with its warning."""
    from learning_jax_sharding_amd.ops import kernels as K
    hip = _hip()
    K._WARNED_DECODE.clear()
    q, k, v, per = _case("plain", 1, 32, 1, 64, [40])
    lt = torch.tensor([39], dtype=torch.int32).cuda()
    with hip.launch_log() as log, pytest.warns(UserWarning, match="attn_decode"):
        o, lse = K.attn_decode(q.cuda(), k.cuda(), v.cuda(), lt, SCALE, 1)
    torch.cuda.synchronize()
    assert not [r for r in log if r["name"].startswith("attn_decode")], log
    _check("fallback G32", o, lse, per)
    with warnings.catch_warnings():
        warnings.simplefilter("error")       # one-time
        K.attn_decode(q.cuda(), k.cuda(), v.cuda(), lt, SCALE, 1)
