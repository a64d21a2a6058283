"""The MX-fp8 cache kernels of csrc/kernels/decode.hip on a real MI355X.

``kv_append<..,mx8>``: the stored bytes and scale bytes equal ``fp8.quantize_mx_ref(hip.rope(...))`` (v: of the rows as
they are), compared as uint8, for the ``rot,q``, ``rot`` and ``copy`` instances, on strided operands (column blocks of
one fused buffer), into caches pre-filled with 0xFF with guard rows behind them; ``q_out`` is ``hip.rope``'s bits.

``attn_decode<..,mx8>``: ``AO.check`` / ``AO.check_lse`` against the float64 oracle of tests/attn_oracle.py on the
dequantised K / V (``dequantize_mx_ref`` of the cache's own bytes: exact), with the bounds tests/test_decode_gpu.py
uses for bf16 caches -- past the dequantisation the arithmetic is the same; forced plans and the default plan;
poisoned tails, determinism and strided views bit for bit; the refusals."""
import pytest
import torch

import attn_oracle as AO

pytestmark = pytest.mark.gpu

SCALE = 0.125
CAP = 512
BF16, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
PLANS = [(1, 512), (4, 128), (8, 64)]
HEADS = [(8, 8), (8, 2), (8, 1), (16, 1)]
LENS = [[0, 1, 15, 16], [17, 63, 64, 65], [127, 128, 129, 511]]      # extra = 1: n_b = lens + 1
INVALID = 1      # hipErrorInvalidValue
FILL = 0xFF


def _hip():
    from learning_jax_sharding_amd.ops import hip
    return hip


@pytest.fixture(autouse=True)
def _default_plan():
    yield
    _hip().set_decode_splits(None)


def _mx(x):
    """(e4m3 bytes, e8m0 bytes) of rows ``x[..., 64]`` by ``quantize_mx_ref``, as the cache stores them (CPU)."""
    from learning_jax_sharding_amd.ops.fp8 import quantize_mx_ref
    q, ex = quantize_mx_ref(x.cpu())
    return q.view(U8), (ex + 127).to(U8)


def _deq(c, s):
    from learning_jax_sharding_amd.ops.fp8 import dequantize_mx_ref
    d = dequantize_mx_ref(c.view(torch.float8_e4m3fn), s.int() - 127)
    assert torch.equal(d.to(BF16).float(), d)          # exact in bf16, so the oracle sees the cache's own values
    return d.to(BF16)


_CASES = {}


def _case(kind, B, H, Hkv, cap, ns):
    """q (bf16), the quantised cache (bytes and scales, CPU) of tests/test_decode_gpu.py's inputs, and the
    per-sequence oracle / model / f32 reference on the dequantised K / V, computed once and left unchanged."""
    key = (kind, B, H, Hkv, cap, tuple(ns))
    if key not in _CASES:
        q, k, v, _ = AO.inputs(kind, B, H, 1, cap, SCALE)
        kc, kcs = _mx(k[:, :, :Hkv].contiguous())
        vc, vcs = _mx(v[:, :, :Hkv].contiguous())
        k, v = _deq(kc, kcs), _deq(vc, vcs)
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
        _CASES[key] = (q, (kc, vc, kcs, vcs), per)
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


def _run(q, cache, lens, extra=1):
    hip = _hip()
    lt = torch.tensor(lens, dtype=torch.int32).cuda()
    o, lse = hip.attn_decode_q8(q.cuda(), *[t.cuda() for t in cache], lt, SCALE, extra)
    torch.cuda.synchronize()
    assert o.shape == (q.shape[0], 1, q.shape[2], 64) and o.dtype == BF16
    assert lse.shape == (q.shape[0], q.shape[2], 1) and lse.dtype == F32
    return o, lse


# ----------------------------------------------------------------------------- attn_decode<..,mx8> vs the oracle
@pytest.mark.parametrize("H,Hkv", HEADS, ids=[f"h{h}kv{k}" for h, k in HEADS])
@pytest.mark.parametrize("plan", PLANS, ids=[f"{n}x{k}" for n, k in PLANS])
def test_decode_q8_matches_oracle(plan, H, Hkv):
    hip = _hip()
    hip.set_decode_splits(*plan)
    for lens in LENS:
        for kind in AO.KINDS:
            q, cache, per = _case(kind, 4, H, Hkv, CAP, [n + 1 for n in lens])
            with hip.launch_log() as log:
                o, lse = _run(q, cache, lens)
            dec = [r for r in log if r["name"].startswith("attn_decode<")]
            assert len(dec) == 1 and dec[0]["grid"] == (plan[0], Hkv, 4) and dec[0]["block"] == 256, log
            assert dec[0]["name"] == f"attn_decode<G{H // Hkv},mx8>", dec
            assert [r["name"] for r in log if r is not dec[0]] == (["decode_merge"] if plan[0] > 1 else []), log
            _check(f"decode q8 {plan} H{H}/{Hkv} {kind} lens{lens}", o, lse, per)


def test_extra_zero_empty_and_full():
    """``extra = 0``: a sequence without any key (o = 0, lse2 = +inf) next to a full cache."""
    hip = _hip()
    q, cache, per = _case("plain", 2, 8, 2, CAP, [0, CAP])
    for plan in PLANS:
        hip.set_decode_splits(*plan)
        o, lse = _run(q, cache, [0, CAP], extra=0)
        _check(f"q8 extra0 {plan}", o, lse, per)


def test_default_plan():
    """The plan function's own plan at cap = 1024: more than one split."""
    hip = _hip()
    cap, lens = 1024, [1023, 600]
    q, cache, per = _case("plain", 2, 8, 2, cap, [n + 1 for n in lens])
    splits, keys = hip.plan_decode(2, 2, cap)
    assert splits > 1 and splits * keys >= cap and keys % hip.decode_key_tile() == 0
    with hip.launch_log() as log:
        o, lse = _run(q, cache, lens)
    assert [r["name"] for r in log] == ["attn_decode<G4,mx8>", "decode_merge"] and log[0]["grid"] == (splits, 2, 2), log
    _check("q8 default plan cap1024", o, lse, per)


# ----------------------------------------------------------------------------- bits
@pytest.mark.parametrize("plan", PLANS, ids=[f"{n}x{k}" for n, k in PLANS])
def test_poisoned_tail_and_determinism(plan):
    """Dead rows' bytes set to 0x7F / 0xFF (the e4m3 NaNs) and their scale bytes to 0xFF / 0x00 (the e8m0 NaN, the
    smallest scale) give the bits of the clean run; two runs of the same call give equal bits."""
    hip = _hip()
    hip.set_decode_splits(*plan)
    lens = [0, 17, 129, 300]
    q, cache, _ = _case("plain", 4, 8, 2, CAP, [1, 18, 130, 301])

    def tail(byte, sbyte):
        out = [t.clone() for t in cache]
        for b, n in enumerate(lens):
            out[0][b, n + 1:] = byte
            out[1][b, n + 1:] = byte
            out[2][b, n + 1:] = sbyte
            out[3][b, n + 1:] = sbyte
        return out

    base = _run(q, cache, lens)
    again = _run(q, cache, lens)
    assert torch.equal(base[0], again[0]) and torch.equal(base[1], again[1])
    for byte, sbyte in ((0x7F, 0xFF), (0xFF, 0x00), (0x7F, 0x00), (0x00, 0xFF)):
        got = _run(q, tail(byte, sbyte), lens)
        assert torch.isfinite(got[0]).all(), (byte, sbyte)
        assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1]), (byte, sbyte)


def test_strided_cache_views():
    """kc / vc as the two column blocks of one byte buffer, the scales as column blocks of another, q a view of a
    wider buffer: the contiguous run's bits."""
    hip = _hip()
    hip.set_decode_splits(4, 128)
    B, H, Hkv = 4, 8, 2
    lens = [3, 64, 200, 511]
    q, cache, _ = _case("plain", B, H, Hkv, CAP, [4, 65, 201, 512])
    base = _run(q, cache, lens)
    kc, vc, kcs, vcs = (t.cuda() for t in cache)
    kv = torch.empty(B, CAP, 2 * Hkv * 64, dtype=U8).cuda()
    kv[..., :Hkv * 64] = kc.view(B, CAP, Hkv * 64)
    kv[..., Hkv * 64:] = vc.view(B, CAP, Hkv * 64)
    sc = torch.empty(B, CAP, 2 * Hkv * 2, dtype=U8).cuda()
    sc[..., :Hkv * 2] = kcs.view(B, CAP, Hkv * 2)
    sc[..., Hkv * 2:] = vcs.view(B, CAP, Hkv * 2)
    kcv, vcv = kv[..., :Hkv * 64].view(B, CAP, Hkv, 64), kv[..., Hkv * 64:].view(B, CAP, Hkv, 64)
    ksv, vsv = sc[..., :Hkv * 2].view(B, CAP, Hkv, 2), sc[..., Hkv * 2:].view(B, CAP, Hkv, 2)
    wide = torch.zeros(B, 1, H * 64 + 64, dtype=BF16).cuda()
    wide[..., :H * 64] = q.cuda().view(B, 1, H * 64)
    qv = wide[..., :H * 64].view(B, 1, H, 64)
    assert not kcv.is_contiguous() and not ksv.is_contiguous() and not qv.is_contiguous()
    got = hip.attn_decode_q8(qv, kcv, vcv, ksv, vsv, torch.tensor(lens, dtype=torch.int32).cuda(), SCALE, 1)
    torch.cuda.synchronize()
    assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1])


def test_bad_arguments_launch_nothing():
    hip = _hip()
    q = torch.zeros(2, 1, 8, 64, dtype=BF16).cuda()
    kc = torch.zeros(2, 64, 2, 64, dtype=U8).cuda()
    ks = torch.zeros(2, 64, 2, 2, dtype=U8).cuda()
    o, lse = torch.empty_like(q), torch.empty(2, 8, 1).cuda()
    lens = torch.zeros(2, dtype=torch.int32).cuda()
    ws = torch.empty(1 << 16).cuda()
    k1 = torch.zeros(2, 1, 2, 64, dtype=BF16).cuda()
    n0 = hip.lib().ljs_launch_count()
    assert hip.attn_decode_q8_raw(q, kc, kc, ks, ks, o, lse, ws, lens, SCALE) == 0                 # (the good call)
    n1 = hip.lib().ljs_launch_count()
    assert n1 == n0 + 1
    assert hip.attn_decode_q8_raw(q, kc, kc, None, ks, o, lse, ws, lens, SCALE) == INVALID         # null scale
    assert hip.attn_decode_q8_raw(q, kc, kc, ks, None, o, lse, ws, lens, SCALE) == INVALID
    odd = torch.zeros(2, 64, 2 * 3, dtype=U8).cuda().view(2, 64, 2, 3)[..., :2]                    # head stride 3
    assert odd.stride(2) == 3
    assert hip.attn_decode_q8_raw(q, kc, kc, odd, ks, o, lse, ws, lens, SCALE) == INVALID          # odd scale stride
    q32 = torch.zeros(2, 1, 64, 64, dtype=BF16).cuda()
    o32, lse32 = torch.empty_like(q32), torch.empty(2, 64, 1).cuda()
    assert hip.attn_decode_q8_raw(q32, kc, kc, ks, ks, o32, lse32, ws, lens, SCALE) == INVALID     # G = 32
    assert hip.attn_decode_q8_raw(q, kc, kc, ks, ks, o, lse, ws, lens, 0.0) == INVALID             # scale <= 0
    assert hip.attn_decode_q8_raw(q, kc, kc, ks, ks, o, lse, ws, lens, -1.0) == INVALID
    mis = torch.zeros(2 * 64 * 2 * 64 + 16, dtype=U8).cuda()[8:8 + 2 * 64 * 2 * 64].view(2, 64, 2, 64)
    assert hip.attn_decode_q8_raw(q, mis, kc, ks, ks, o, lse, ws, lens, SCALE) == INVALID          # 8-byte aligned base
    hip.set_decode_splits(2, 48)                                                                   # not a tile multiple
    assert hip.attn_decode_q8_raw(q, kc, kc, ks, ks, o, lse, ws, lens, SCALE) == INVALID
    hip.set_decode_splits(None)
    assert hip.kv_append_q8_raw(k1, k1, kc, kc, None, ks, lens) == INVALID                         # null scale
    assert hip.kv_append_q8_raw(k1, k1, kc, kc, odd, ks, lens) == INVALID                          # odd scale stride
    assert hip.kv_append_q8_raw(k1, k1, mis, kc, ks, ks, lens) == INVALID
    assert hip.lib().ljs_launch_count() == n1
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- kv_append<..,mx8>
APP_CAP = 40
THETA = 10000.0


def _append_setup(B, T, H, Hkv, seed):
    """q / k / v as column blocks of one fused bf16 buffer (strided), with all-zero blocks in v; caches and scales
    pre-filled with 0xFF, with guard rows behind them."""
    gen = torch.Generator().manual_seed(23 + seed)
    fused = torch.randn(B, T, (H + 2 * Hkv) * 64, generator=gen).to(BF16).cuda()
    q = fused[..., :H * 64].view(B, T, H, 64)
    k = fused[..., H * 64:(H + Hkv) * 64].view(B, T, Hkv, 64)
    v = fused[..., (H + Hkv) * 64:].view(B, T, Hkv, 64)
    v[0, 0, 0, :32] = 0
    v[B - 1, T - 1, Hkv - 1, 32:] = 0
    assert not k.is_contiguous() and not v.is_contiguous()
    mk = lambda w: torch.full((B, APP_CAP + 8, Hkv, w), FILL, dtype=U8).cuda()   # noqa: E731
    big = (mk(64), mk(64), mk(2), mk(2))
    return q, k, v, big, tuple(t[:, :APP_CAP] for t in big)


def _check_append(name, k_rows, v, views, big, rows):
    """``rows``: {(b, t): p} of the rows written; ``k_rows(b, t, p)``: the bf16 row the bf16 cache would hold."""
    kc, vc, kcs, vcs = (t.cpu() for t in views)
    for t in big:
        assert (t[:, APP_CAP:] == FILL).all(), name              # guard rows: neither bytes nor scales
    untouched = torch.ones(kc.shape[:2], dtype=torch.bool)
    for (b, t), p in rows.items():
        wk, wks = _mx(k_rows(b, t, p))
        wv, wvs = _mx(v[b, t])
        assert torch.equal(kc[b, p], wk) and torch.equal(kcs[b, p], wks), (name, b, t)
        assert torch.equal(vc[b, p], wv) and torch.equal(vcs[b, p], wvs), (name, b, t)
        untouched[b, p] = False
    for t in (kc, vc, kcs, vcs):
        assert (t[untouched] == FILL).all(), name


def _zero_block_scale_byte():
    """What ``ljs_quant_mx_rows`` writes for an all-zero block."""
    from learning_jax_sharding_amd.ops import fp8
    qz, sz = fp8.quant_rows(torch.zeros(1, 64, dtype=BF16).cuda())
    torch.cuda.synchronize()
    assert (qz == 0).all() and sz[0, 0] == sz[0, 1]
    return int(sz[0, 0])


@pytest.mark.parametrize("lens", [[0, 17, APP_CAP - 1], [APP_CAP, APP_CAP + 5, 3]], ids=["inside", "beyond"])
@pytest.mark.parametrize("Hkv", [1, 2])
@pytest.mark.parametrize("inst", ["rot,q", "rot", "copy"])
def test_append_q8_device_lens(inst, Hkv, lens):
    """T = 1 at rows read on the device: 0, a middle row, cap - 1, cap and beyond."""
    hip = _hip()
    B, H = 3, 8
    q, k, v, big, views = _append_setup(B, 1, H, Hkv, seed=Hkv)
    lt = torch.tensor(lens, dtype=torch.int32).cuda()
    theta = None if inst == "copy" else THETA
    with hip.launch_log() as log:
        q_out = hip.kv_append_q8(k, v, *views, lt, q=q if inst == "rot,q" else None, theta=theta)
    torch.cuda.synchronize()
    assert [r["name"] for r in log] == [f"kv_append<{inst},mx8>"], log
    assert torch.equal(lt.cpu(), torch.tensor(lens, dtype=torch.int32))
    rot = lambda x, p: hip.rope(x.contiguous(), None, pos_offset=p, theta=THETA)[0]   # noqa: E731
    k_rows = (lambda b, t, p: k[b, t]) if theta is None else (lambda b, t, p: rot(k[b:b + 1, t:t + 1], p)[0, 0])
    rows = {(b, 0): n for b, n in enumerate(lens) if n < APP_CAP}
    _check_append(f"{inst} Hkv{Hkv} lens{lens}", k_rows, v, views, big, rows)
    if inst == "rot,q":
        assert q_out.dtype == BF16 and q_out.shape == q.shape
        for b, n in enumerate(lens):
            want = rot(q[b:b + 1], n) if n < APP_CAP else torch.zeros_like(q_out[b:b + 1])
            assert torch.equal(q_out[b:b + 1], want), b
    else:
        assert q_out is None
    if lens[0] == 0:                                             # the all-zero block of v[0, 0, 0]
        vc, vcs = views[1].cpu(), views[3].cpu()
        assert (vc[0, 0, 0, :32] == 0).all() and int(vcs[0, 0, 0, 0]) == _zero_block_scale_byte()
        assert vcs[0, 0, 0, 1] != vcs[0, 0, 0, 0]


@pytest.mark.parametrize("Hkv", [1, 2])
@pytest.mark.parametrize("inst", ["rot", "copy"])
def test_append_q8_host_base_mode(inst, Hkv):
    """Prefill: no lens, T = 5 rows to rows 0..4, as they are or rotated at positions 0..4."""
    hip = _hip()
    B, T = 3, 5
    _, k, v, big, views = _append_setup(B, T, 8, Hkv, seed=10 + Hkv)
    theta = None if inst == "copy" else THETA
    with hip.launch_log() as log:
        assert hip.kv_append_q8(k, v, *views, None, theta=theta) is None
    torch.cuda.synchronize()
    assert [r["name"] for r in log] == [f"kv_append<{inst},mx8>"], log
    kr = k if theta is None else hip.rope(k.contiguous(), None, pos_offset=0, theta=THETA)[0]
    rows = {(b, t): t for b in range(B) for t in range(T)}
    _check_append(f"host base {inst} Hkv{Hkv}", lambda b, t, p: kr[b, t], v, views, big, rows)
    vc, vcs = views[1].cpu(), views[3].cpu()
    assert (vc[0, 0, 0, :32] == 0).all() and int(vcs[0, 0, 0, 0]) == _zero_block_scale_byte()
    assert (vc[B - 1, T - 1, Hkv - 1, 32:] == 0).all() and int(vcs[B - 1, T - 1, Hkv - 1, 1]) == _zero_block_scale_byte()


def test_append_q8_rows_past_the_cache_with_T3():
    """``lens[b] + T > cap``: the rows in range are written, the others nowhere; q_out gets zeros there."""
    hip = _hip()
    B, H, Hkv, T = 3, 8, 2, 3
    lens = [APP_CAP - 1, APP_CAP - 2, 10]
    q, k, v, big, views = _append_setup(B, T, H, Hkv, seed=5)
    q_out = hip.kv_append_q8(k, v, *views, torch.tensor(lens, dtype=torch.int32).cuda(), q=q, theta=THETA)
    torch.cuda.synchronize()
    rot = lambda x, p: hip.rope(x.contiguous(), None, pos_offset=p, theta=THETA)[0]   # noqa: E731
    rows = {(b, t): n + t for b, n in enumerate(lens) for t in range(T) if n + t < APP_CAP}
    _check_append("past the cache", lambda b, t, p: rot(k[b:b + 1, t:t + 1], p)[0, 0], v, views, big, rows)
    for b, n in enumerate(lens):
        for t in range(T):
            want = rot(q[b:b + 1, t:t + 1], n + t)[0, 0] if n + t < APP_CAP else torch.zeros_like(q_out[b, t])
            assert torch.equal(q_out[b, t], want), (b, t)


# ----------------------------------------------------------------------------- the dispatcher
def test_dispatcher_takes_the_kernels_and_falls_back_with_a_warning():
    """``ops.kernels``' q8 entry points run the mx8 instances on supported shards; a group of 32 runs the torch
    reference on the GPU with a one-time warning."""
    from learning_jax_sharding_amd.ops import kernels as K
    hip = _hip()
    q, cache, per = _case("plain", 2, 8, 2, CAP, [0, CAP])
    lt = torch.tensor([0, CAP], dtype=torch.int32).cuda()
    dev = [t.cuda() for t in cache]
    with hip.launch_log() as log:
        o, lse = K.attn_decode_q8(q.cuda(), *dev, lt, SCALE, 0)
    assert log[0]["name"] == "attn_decode<G4,mx8>", log
    ro, rl = K.attn_decode_q8_reference(q.cuda(), *dev, lt, SCALE, 0)
    _check("dispatcher kernel", o, lse, per)
    _check("dispatcher reference on the GPU", ro, rl, per)
    K._WARNED_DECODE.clear()
    q32 = torch.randn(2, 1, 64, 64, generator=torch.Generator().manual_seed(3)).to(BF16).cuda()
    with hip.launch_log() as log, pytest.warns(UserWarning, match="attn_decode_q8"):
        o32, _ = K.attn_decode_q8(q32, *dev, lt, SCALE, 0)
    torch.cuda.synchronize()
    assert not [r for r in log if r["name"].startswith("attn_decode")], log
    assert o32.shape == (2, 1, 64, 64) and (o32[0] == 0).all()
