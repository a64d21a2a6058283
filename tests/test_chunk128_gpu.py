"""prefill128.hip on a real MI355X under ``LJS_ATTN_D128=1``, held as tests/test_chunk_gpu.py holds the 64 kernel; the switch."""
import functools

import pytest
import torch

import attn_oracle as AO
from learning_jax_sharding_amd.ops import hip, kernels as K
from test_chunk_gpu import INVALID, _same

pytestmark = pytest.mark.gpu

D, SCALE, CAP, B = 128, 128 ** -0.5, 320, 4            # five 64-key tiles
BF16, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
# a lone row; 132 rows at G = 4 crossing a 128-row tile (every kind); two tiles at G = 1; G = 3; G = 16 with dead waves at 128 rows
SHAPES = [(2, 2, 1), (8, 2, 33), (8, 8, 129), (6, 2, 129), (16, 1, 5)]
LENS = [(0, 1, 63, 64), (65, 127, 128, 200), (255, 256, 300, 319)]     # tile edges; empty; the last set runs past cap
_i32 = lambda x: torch.tensor(x, dtype=torch.int32).cuda()   # noqa: E731
_view = lambda t: torch.zeros(B, CAP + 8, t.shape[2] + 1, t.shape[3], dtype=t.dtype, device="cuda")[:, 8:, 1:].copy_(t)   # noqa: E731


@pytest.fixture(autouse=True)
def _switch_on(monkeypatch):
    monkeypatch.setenv("LJS_ATTN_D128", "1")
    yield
    hip.set_chunk_rows(None)


@functools.lru_cache(maxsize=None)
def _case(kind, H, Hkv, T, lens):
    """Inputs (bf16, CPU) and per sequence (oracle o, oracle lse2, model o, f32 lse2): computed once and left unchanged."""
    q, k, v, _ = AO.inputs(kind, B, H, T, CAP, SCALE, D=D)
    k, v, per = k[:, :, :Hkv].contiguous(), v[:, :, :Hkv].contiguous(), []
    for b, n0 in enumerate(lens):
        qkv = [q[b:b + 1]] + [x[b:b + 1, :min(n0 + T, CAP)].repeat_interleave(H // Hkv, 2) for x in (k, v)]
        kw = dict(causal=True, q_offset=n0)
        per.append(AO.forward(*qkv, SCALE, **kw) + (AO.forward(*qkv, SCALE, rounded=True, **kw)[0], AO.lse2_f32(*qkv[:2], SCALE, **kw)))
    return q, k, v, per


def _data(H, Hkv, T, lens):
    """On the GPU: q; caches with NaN rows at and beyond each sequence's largest limit; with zeros there; as MX-fp8 buffers (kc,
    vc, kcs, vcs) with 0x7F / 0xFF bytes and 0xFF / 0x00 scales there; the dequantised live rows; lens."""
    gen = torch.Generator().manual_seed(5)
    q, k, v = (torch.randn(B, n, h, D, generator=gen).to(BF16) for n, h in ((T, H), (CAP, Hkv), (CAP, Hkv)))
    dead = (torch.arange(CAP)[None, :] >= (torch.tensor(lens) + T).clamp(0, CAP)[:, None])[:, :, None, None]
    f = lambda t, x: t.masked_fill(dead, x).cuda()   # noqa: E731
    (kq, ke), (vq, ve) = K._mx_bytes(k), K._mx_bytes(v)
    deq = (K.mx_cache_dequant(f(kq, 0), f(ke, 0)), K.mx_cache_dequant(f(vq, 0), f(ve, 0)))
    return q.cuda(), (f(k, float("nan")), f(v, float("nan"))), (f(k, 0), f(v, 0)), (f(kq, 0x7F), f(vq, 0xFF), f(ke, 0xFF), f(ve, 0)), deq, _i32(lens)


@pytest.mark.parametrize("rows", [64, 128])
@pytest.mark.parametrize("H,Hkv,T", SHAPES)
def test_chunk128_matches_oracle(H, Hkv, T, rows):
    hip.set_chunk_rows(rows)
    G, worst = H // Hkv, [0.0, 0.0]
    for lens in LENS:
        for kind in (AO.KINDS if (H, Hkv, T) == SHAPES[1] else ("plain",)):
            q, k, v, per = _case(kind, H, Hkv, T, lens)
            with hip.launch_log() as log:
                o, lse = (t.cpu() for t in hip.attn_chunk(q.cuda(), k.cuda(), v.cuda(), _i32(lens), SCALE))
            assert [(r["name"], tuple(r["grid"]), r["block"]) for r in log] == [(f"attn_chunk128<R{rows}>", (-(-T * G // rows), Hkv, B), 256)], log
            for b, (want_o, want_lse, model_o, ref32) in enumerate(per):
                name = f"chunk128 R{rows} H{H}/{Hkv} T{T} {kind} lens{lens} b{b}"
                worst[0] = max(worst[0], AO.check(f"{name} o", o[b:b + 1], want_o, model_o))
                worst[1] = max(worst[1], AO.check_lse(lse[b:b + 1], want_lse, ref32, name=f"{name} lse"))
    print(f"chunk128-figures R{rows} H{H}/{Hkv} T{T} worst fraction of the bound: o {worst[0]:.3f} lse2 {worst[1]:.3f}")


@pytest.mark.parametrize("rows", [64, 128])
@pytest.mark.parametrize("H,Hkv,T", [(8, 2, 33), (6, 2, 129)])
def test_bits(H, Hkv, T, rows):
    """Poisoned tails, a second run, mx8 against bf16 on the dequantised live rows and strided views: equal bits; negative lengths."""
    hip.set_chunk_rows(rows)
    for lens in LENS:
        q, poisoned, zeroed, q8, deq, lt = _data(H, Hkv, T, lens)
        first = hip.attn_chunk(q, *poisoned, lt, SCALE)
        assert _same(first, hip.attn_chunk(q, *zeroed, lt, SCALE)) and _same(first, hip.attn_chunk(q, *poisoned, lt, SCALE)), lens
        with hip.launch_log() as log:
            got8 = hip.attn_chunk_q8(q, *q8, lt, SCALE)
        assert [r["name"] for r in log] == [f"attn_chunk128<R{rows},mx8>"], log
        assert _same(got8, hip.attn_chunk(q, *deq, lt, SCALE)) and _same(got8, hip.attn_chunk_q8(q, *q8, lt, SCALE)), lens
    # q as a column block of a fused QKV buffer; the caches, both kinds and the scales too, as views of wider buffers (_view: 8
    # rows and one head in front)
    fused = torch.cat([q.reshape(B, T, H * D), torch.randn(B, T, 2 * Hkv * D, device="cuda").to(BF16)], -1)
    qs, views, views8 = fused[..., :H * D].view(B, T, H, D), [_view(t) for t in zeroed], [_view(t) for t in q8]
    assert _same(hip.attn_chunk(qs, *views, lt, SCALE), first) and _same(hip.attn_chunk_q8(qs, *views8, lt, SCALE), got8)
    neg = _i32([-T - 7, -2, 5, -T])                                         # b = 1: only the rows t < 2 see nothing
    for o, lse in (hip.attn_chunk(q, *zeroed, neg, SCALE), hip.attn_chunk_q8(q, *q8, neg, SCALE)):
        assert not o[0].any() and not o[3].any() and not o[1, :2].any() and o[2].any()
        assert torch.equal(torch.isposinf(lse), (neg[:, None] + torch.arange(1, T + 1).cuda() <= 0)[:, None, :].expand_as(lse))


def test_captured_launch_follows_lens():
    q, _, (k, v), q8, _, lt = _data(8, 2, 40, [250] * B)           # (one graph holds the bf16 and the mx8 instance)
    both = lambda: (hip.attn_chunk(q, k, v, lt, SCALE), hip.attn_chunk_q8(q, *q8, lt, SCALE))   # noqa: E731
    both()                                                                          # warm up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = both()
    for lens in (LENS[0], (65, 127, 128, 200), (250, 240, 3, 0)):
        lt.copy_(_i32(lens))
        graph.replay(), graph.replay()
        torch.cuda.synchronize()
        assert all(_same(a, b) for a, b in zip(out, both())), lens


def test_switch_and_refusals(monkeypatch):
    z = lambda *s, dt=BF16: torch.zeros(*s, dtype=dt).cuda()   # noqa: E731
    kc, k8, ks, lens = z(2, 64, 2, D), z(2, 64, 2, D, dt=U8), z(2, 64, 2, 4, dt=U8), z(2, dt=torch.int32)
    shifted = lambda t, n: z(t.numel() + 2 * n, dt=t.dtype)[n:n + t.numel()].view(t.shape)   # noqa: E731  (the base n elements on)

    def raw(H=8, T=4, c=(kc, kc), lens=lens):
        return (hip.attn_chunk_q8_raw if len(c) == 4 else hip.attn_chunk_raw)(z(2, T, H, D), *c, z(2, T, H, D), z(2, T, H, dt=F32), lens, SCALE)

    count, off = hip.lib().ljs_launch_count, shifted(kc, 4)
    n0 = count()
    assert raw(T=100) == 0 and raw(T=100, c=(k8, k8, ks, ks)) == 0 and count() == n0 + 2        # (the good calls: T > cap too)
    # a 64 descriptor; G = 32; H % Hkv != 0; a null lens; a 128-wide cache base 8 bytes off the grid; a scale base off the 4-byte rule
    bad = [raw(c=(z(2, 64, 2, 64),) * 2), raw(H=64), raw(H=7), raw(lens=None), raw(c=(off, kc)), raw(c=(k8, k8, shifted(ks, 2), ks))]
    assert off.shape[-1] == D and off.data_ptr() % 16 == 8 and bad == [INVALID] * 6 and count() == n0 + 2
    # the switch unset: hip refuses and launches nothing; kernels warns once, and both calls return the reference's values
    monkeypatch.delenv("LJS_ATTN_D128")
    monkeypatch.setattr(K, "_WARNED_DECODE", set())
    q = z(2, 4, 8, D)
    with pytest.raises(NotImplementedError, match="attn_chunk"):
        hip.attn_chunk(q, kc, kc, lens, SCALE)
    with pytest.warns(UserWarning, match="attn_chunk") as rec:
        got = [K.attn_chunk(q, kc, kc, lens, SCALE) for _ in range(2)]
    assert len([w for w in rec if "attn_chunk" in str(w.message)]) == 1 and count() == n0 + 2
    assert all(torch.equal(a, b) for g in got for a, b in zip(g, K.attn_chunk_reference(q, kc, kc, lens, SCALE)))
