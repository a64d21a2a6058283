"""prefill.hip on a real MI355X: ``hip.attn_chunk`` against tests/attn_oracle.py per sequence (``AO.forward(q[b], kc[b, :n],
vc[b, :n], SCALE, causal=True, q_offset=lens[b])``, ``n = min(lens[b] + T, cap)``) under both row tiles, and its bits."""
import pytest
import torch

import attn_oracle as AO

pytestmark = pytest.mark.gpu

SCALE, CAP, B = 0.125, 512, 4
BF16, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
HEADS = [(8, 8), (8, 2), (6, 2), (16, 1)]                 # G = 1, 4, 3, 16
TS = [1, 33, 129]       # a lone row; 132 rows at G = 4 crossing a 128-row tile; two tiles at G = 1
LENS = [[0, 1, 63, 64], [65, 127, 128, 300], [383, 400, 480, 511]]     # tile edges; empty; the last set runs past cap
ALL_KINDS = (8, 2, 33)
INVALID = 1             # hipErrorInvalidValue


def _hip():
    from learning_jax_sharding_amd.ops import hip
    return hip


@pytest.fixture(autouse=True)
def _default_rows():
    yield
    _hip().set_chunk_rows(None)


_CASES = {}


def _case(kind, H, Hkv, T, lens):
    """Inputs (bf16, CPU) and the per-sequence oracle / model / f32 reference, computed once and left unchanged."""
    key = (kind, H, Hkv, T, tuple(lens))
    if key not in _CASES:
        q, k, v, _ = AO.inputs(kind, B, H, T, CAP, SCALE)
        k, v = k[:, :, :Hkv].contiguous(), v[:, :, :Hkv].contiguous()
        per = []
        for b, n0 in enumerate(lens):
            n = min(n0 + T, CAP)
            qb = q[b:b + 1]
            kb, vb = (x[b:b + 1, :n].repeat_interleave(H // Hkv, 2) for x in (k, v))
            o, lse = AO.forward(qb, kb, vb, SCALE, causal=True, q_offset=n0)
            mo, _ = AO.forward(qb, kb, vb, SCALE, causal=True, q_offset=n0, rounded=True)
            per.append((o, lse, mo, AO.lse2_f32(qb, kb, SCALE, causal=True, q_offset=n0)))
        _CASES[key] = (q, k, v, per)
    return _CASES[key]


def _data(H, Hkv, T, lens, seed=5):
    """Random q and caches on the GPU whose rows at and beyond each sequence's largest limit hold NaN, and the same
    caches as MX-fp8 buffers with the formats' NaN bytes (0x7F / 0xFF) and 0xFF / 0x00 scales there."""
    from learning_jax_sharding_amd.ops import kernels as K
    gen = torch.Generator().manual_seed(seed)
    q = torch.randn(B, T, H, 64, generator=gen).to(BF16)
    k = torch.randn(B, CAP, Hkv, 64, generator=gen).to(BF16)
    v = torch.randn(B, CAP, Hkv, 64, generator=gen).to(BF16)
    (kq, ke), (vq, ve) = K._mx_bytes(k), K._mx_bytes(v)
    kz, vz = k.clone(), v.clone()
    for b, n0 in enumerate(lens):
        n = max(min(n0 + T, CAP), 0)
        k[b, n:], v[b, n:], kz[b, n:], vz[b, n:] = float("nan"), float("nan"), 0, 0
        kq[b, n:], vq[b, n:], ke[b, n:], ve[b, n:] = 0x7F, 0xFF, 0xFF, 0x00
    lt = torch.tensor(lens, dtype=torch.int32).cuda()
    return q.cuda(), (k.cuda(), v.cuda()), (kz.cuda(), vz.cuda()), tuple(x.cuda() for x in (kq, vq, ke, ve)), lt


def _same(a, b):
    return torch.equal(a[0].view(torch.int16), b[0].view(torch.int16)) and torch.equal(a[1].view(torch.int32),
                                                                                      b[1].view(torch.int32))


# ----------------------------------------------------------------------------- attn_chunk vs the oracle
@pytest.mark.parametrize("rows", [64, 128])
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("H,Hkv", HEADS, ids=[f"h{h}kv{k}" for h, k in HEADS])
def test_chunk_matches_oracle(H, Hkv, T, rows):
    hip = _hip()
    hip.set_chunk_rows(rows)
    G = H // Hkv
    for lens in LENS:
        for kind in (AO.KINDS if (H, Hkv, T) == ALL_KINDS else ("plain",)):
            q, k, v, per = _case(kind, H, Hkv, T, lens)
            lt = torch.tensor(lens, dtype=torch.int32).cuda()
            with hip.launch_log() as log:
                o, lse = hip.attn_chunk(q.cuda(), k.cuda(), v.cuda(), lt, SCALE)
            torch.cuda.synchronize()
            assert [(r["name"], tuple(r["grid"]), r["block"]) for r in log] == \
                [(f"attn_chunk<R{rows}>", (-(-T * G // rows), Hkv, B), 256)], log
            assert o.shape == (B, T, H, 64) and o.dtype == BF16 and lse.shape == (B, H, T) and lse.dtype == F32
            o, lse = o.cpu(), lse.cpu()
            for b, (want_o, want_lse, model_o, ref32) in enumerate(per):
                name = f"chunk R{rows} H{H}/{Hkv} T{T} {kind} lens{lens} b{b}"
                AO.check(f"{name} o", o[b:b + 1], want_o, model_o)
                AO.check_lse(lse[b:b + 1], want_lse, ref32, name=f"{name} lse")


# ----------------------------------------------------------------------------- bits
@pytest.mark.parametrize("rows", [64, 128])
@pytest.mark.parametrize("H,Hkv,T", [(8, 2, 33), (6, 2, 129), (16, 1, 5)])
def test_poisoned_tails_reruns_and_mx8_bits(H, Hkv, T, rows):
    """NaN rows (bf16) and NaN bytes / scales (MX-fp8) beyond the limits give the bits of a zero tail; a second run gives
    equal bits; the mx8 instance on a cache gives the bits of the bf16 instance on its dequantised copy."""
    from learning_jax_sharding_amd.ops import kernels as K
    hip = _hip()
    hip.set_chunk_rows(rows)
    for lens in LENS:
        q, poisoned, zeroed, q8, lt = _data(H, Hkv, T, lens)
        first = hip.attn_chunk(q, *poisoned, lt, SCALE)
        assert torch.isfinite(first[0].float()).all() and torch.isfinite(first[1]).all()
        assert _same(first, hip.attn_chunk(q, *zeroed, lt, SCALE)), lens
        assert _same(first, hip.attn_chunk(q, *poisoned, lt, SCALE)), lens
        with hip.launch_log() as log:
            got8 = hip.attn_chunk_q8(q, *q8, lt, SCALE)
        assert [r["name"] for r in log] == [f"attn_chunk<R{rows},mx8>"], log
        live = torch.arange(CAP)[None, :] < (torch.tensor(lens) + T).clamp(0, CAP)[:, None]
        z = lambda t: torch.where(live[:, :, None, None].cuda(), t, torch.zeros_like(t))   # noqa: E731
        deq = (K.mx_cache_dequant(z(q8[0]), z(q8[2])), K.mx_cache_dequant(z(q8[1]), z(q8[3])))
        assert _same(got8, hip.attn_chunk(q, *deq, lt, SCALE)), lens
        assert _same(got8, hip.attn_chunk_q8(q, *q8, lt, SCALE)), lens


def test_strided_operands():
    """q as a column block of a fused projection buffer and the caches as views of wider buffers: the bits of the
    contiguous call."""
    hip = _hip()
    H, Hkv, T = 8, 2, 70
    q, _, (k, v), _, lt = _data(H, Hkv, T, LENS[1])
    fused = torch.randn(B, T, (H + 2 * Hkv) * 64, device="cuda").to(BF16)
    fused[..., :H * 64] = q.reshape(B, T, H * 64)
    qs = fused[..., :H * 64].view(B, T, H, 64)
    wide = torch.randn(2, B, CAP + 8, Hkv + 1, 64, device="cuda").to(BF16)
    wide[0, :, 8:, 1:], wide[1, :, 8:, 1:] = k, v
    ks, vs = wide[0, :, 8:, 1:], wide[1, :, 8:, 1:]
    assert not qs.is_contiguous() and not ks.is_contiguous()
    for rows in (64, 128):
        hip.set_chunk_rows(rows)
        assert _same(hip.attn_chunk(qs, ks, vs, lt, SCALE), hip.attn_chunk(q, k, v, lt, SCALE)), rows


def test_negative_length_gives_zeros():
    hip = _hip()
    H, Hkv, T = 8, 2, 3
    q, (k, v), _, q8, _ = _data(H, Hkv, T, [5, 5, 5, 5])
    lt = torch.tensor([-7, -2, 5, -3], dtype=torch.int32).cuda()      # limits: 0 0 0 | 0 0 1 | 6 7 8 | 0 0 0
    for o, lse in (hip.attn_chunk(q, k, v, lt, SCALE), hip.attn_chunk_q8(q, *q8, lt, SCALE)):
        assert not o[0].any() and not o[3].any() and not o[1, :2].any()
        assert torch.isposinf(lse[0]).all() and torch.isposinf(lse[3]).all() and torch.isposinf(lse[1, :, :2]).all()
        assert torch.isfinite(lse[2]).all() and torch.isfinite(lse[1, :, 2]).all() and o[2].any() and o[1, 2].any()


def test_bad_arguments_launch_nothing():
    hip = _hip()
    kc = torch.zeros(2, 64, 2, 64, dtype=BF16).cuda()
    k8 = torch.zeros(2, 64, 2, 64, dtype=U8).cuda()
    ks = torch.zeros(2, 64, 2, 2, dtype=U8).cuda()
    lens = torch.zeros(2, dtype=torch.int32).cuda()

    def ops(T, H=8):
        q = torch.zeros(2, T, H, 64, dtype=BF16).cuda()
        return q, torch.empty_like(q), torch.empty(2, T, H).cuda()

    n0 = hip.lib().ljs_launch_count()
    q, o, lse = ops(100)
    assert hip.attn_chunk_raw(q, kc, kc, o, lse, lens, SCALE) == 0                           # (the good calls: T > cap too)
    assert hip.attn_chunk_q8_raw(q, k8, k8, ks, ks, o, lse, lens, SCALE) == 0
    n1 = hip.lib().ljs_launch_count()
    assert n1 == n0 + 2
    q32, o32, lse32 = ops(4, 64)
    assert hip.attn_chunk_raw(q32, kc, kc, o32, lse32, lens, SCALE) == INVALID               # G = 32
    q7, o7, lse7 = ops(4, 7)
    assert hip.attn_chunk_raw(q7, kc, kc, o7, lse7, lens, SCALE) == INVALID                  # H % Hkv != 0
    assert hip.attn_chunk_raw(q, kc, kc, o, lse, lens, 0.0) == INVALID                       # scale <= 0
    assert hip.attn_chunk_raw(q, kc, kc, o, lse, None, SCALE) == INVALID                     # no lens
    assert hip.attn_chunk_raw(q, kc[..., 4:], kc, o, lse, lens, SCALE) == INVALID            # a misaligned cache base
    assert hip.attn_chunk_q8_raw(q, k8, k8, ks[..., 1:], ks, o, lse, lens, SCALE) == INVALID  # an odd scale base
    assert hip.lib().ljs_launch_count() == n1
    with pytest.raises(NotImplementedError, match="attn_chunk"):
        hip.attn_chunk(q.float(), kc, kc, lens, SCALE)
    torch.cuda.synchronize()


def test_captured_launch_follows_lens():
    """No kernel argument depends on ``lens``: a graph captured at one set of lengths, replayed after they moved, gives the
    eager result at the new lengths (several replays)."""
    hip = _hip()
    H, Hkv, T = 8, 2, 40
    q, _, (k, v), q8, lt = _data(H, Hkv, T, [400] * B)
    lt.copy_(torch.tensor([0, 1, 63, 64], dtype=torch.int32))
    hip.attn_chunk(q, k, v, lt, SCALE), hip.attn_chunk_q8(q, *q8, lt, SCALE)       # warm up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = hip.attn_chunk(q, k, v, lt, SCALE)
        out8 = hip.attn_chunk_q8(q, *q8, lt, SCALE)
    for lens in ([65, 127, 128, 300], [383, 400, 3, 0], [0, 1, 63, 64]):
        lt.copy_(torch.tensor(lens, dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        assert _same(out, hip.attn_chunk(q, k, v, lt, SCALE)), lens
        assert _same(out8, hip.attn_chunk_q8(q, *q8, lt, SCALE)), lens
