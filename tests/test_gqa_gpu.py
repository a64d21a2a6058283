"""Grouped-query attention on a real MI355X: the kernels' K/V head lookup (``ljs_attn_*_gqa``) and
``gqa_reduce`` against the expanded-MHA baseline -- the same entry points on K / V expanded to one
head per query head with ``repeat_interleave`` -- bit for bit, and against the float64 oracle of
tests/attn_oracle.py."""
import ctypes

import pytest
import torch

import attn_oracle as AO

pytestmark = pytest.mark.gpu

SCALE = 0.125
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64


def _hip():
    from learning_jax_sharding_amd.ops import hip
    return hip


def _inputs(B, H, Hkv, Sq, Sk, seed=0):
    """q, do of H heads and k, v of Hkv heads, bf16 on the GPU."""
    gen = torch.Generator().manual_seed(7 * Sq + 3 * Sk + 131 * B + 17 * H + Hkv + 1000 * seed)
    q = torch.randn(B, Sq, H, 64, generator=gen)
    k = torch.randn(B, Sk, Hkv, 64, generator=gen)
    v = torch.randn(B, Sk, Hkv, 64, generator=gen)
    do = torch.randn(B, Sq, H, 64, generator=gen)
    return tuple(t.to(BF16).cuda() for t in (q, k, v, do))


def _expand(t, G):
    return t.repeat_interleave(G, 2).contiguous()


def _fold(x, Hkv):
    """The reference of gqa_reduce: bf16 [B, S, H, 64] -> [B, S, Hkv, 64], an explicit ascending-g loop
    of f32 adds on the host and one rounding to bf16."""
    B, S, H, D = x.shape
    G = H // Hkv
    xf = x.detach().cpu().to(F32).view(B, S, Hkv, G, D)
    acc = xf[:, :, :, 0].clone()
    for g in range(1, G):
        acc = acc + xf[:, :, :, g]
    return acc.to(BF16)


def _names(log):
    return [r["name"] for r in log]


# ----------------------------------------------------------------------------- 6. forward
FWD = [(4, 64, 8, 200, 200, True, 0, "attn_fwd_res<8>"), (2, 6, 2, 256, 256, False, 0, "attn_fwd_res<4>"),
       (2, 6, 2, 256, 256, True, 0, "attn_fwd_res<4>"), (1, 4, 1, 40, 40, False, 0, "attn_fwd_res<4>"),
       (1, 4, 2, 100, 257, False, 0, "attn_fwd_tiled<1>"), (1, 4, 1, 200, 700, True, 500, "attn_fwd_tiled<1>")]


@pytest.mark.parametrize("B,H,Hkv,Sq,Sk,causal,off,inst", FWD)
def test_forward_bits(B, H, Hkv, Sq, Sk, causal, off, inst):
    hip = _hip()
    q, k, v, _ = _inputs(B, H, Hkv, Sq, Sk)
    G = H // Hkv
    with hip.launch_log() as base:
        ox, lsex = hip.attn_fwd_lse(q, _expand(k, G), _expand(v, G), SCALE, causal, off)
    with hip.launch_log() as log:
        o, lse = hip.attn_fwd_lse(q, k, v, SCALE, causal, off)
    torch.cuda.synchronize()
    assert torch.equal(o, ox) and torch.equal(lse, lsex) and lse.shape == (B, H, Sq)
    assert len(log) == 1 and len(base) == 1 and log[0] == base[0], (log, base)
    assert log[0]["name"] == inst, log


def test_forward_strided_kv():
    """K / V as the two adjacent column blocks of one [T][2 Hkv 64] buffer, and seq-major."""
    hip = _hip()
    B, H, Hkv, Sq, Sk = 2, 6, 2, 256, 256
    q, k, v, _ = _inputs(B, H, Hkv, Sq, Sk, seed=1)
    want = hip.attn_fwd_lse(q, _expand(k, 3), _expand(v, 3), SCALE, True, 0)
    buf = torch.empty(B, Sk, 2, Hkv, 64, dtype=BF16, device="cuda")
    buf[:, :, 0], buf[:, :, 1] = k, v
    got = hip.attn_fwd_lse(q, buf[:, :, 0], buf[:, :, 1], SCALE, True, 0)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    ks, vs = (torch.empty(Sk, B, Hkv, 64, dtype=BF16, device="cuda").permute(1, 0, 2, 3) for _ in range(2))
    ks.copy_(k), vs.copy_(v)
    assert ks.stride(1) > ks.stride(0)
    got = hip.attn_fwd_lse(q, ks, vs, SCALE, True, 0)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # through hip.attention (the autograd function): the same output
    assert torch.equal(hip.attention(q, ks, vs, SCALE, True, 0), want[0])


@pytest.mark.parametrize("cuts", [(100,), (64, 192)], ids=["modes13", "modes123"])
def test_forward_acc_modes(cuts):
    """attn_fwd_acc over two (modes 1, 3) and three (1, 2, 3) key blocks."""
    hip = _hip()
    B, H, Hkv, Sq, Sk = 1, 4, 2, 130, 257
    q, k, v, _ = _inputs(B, H, Hkv, Sq, Sk, seed=2)
    edges = (0,) + cuts + (Sk,)

    def run(kk, vv):
        oacc = torch.empty(B, Sq, H, 64, dtype=F32, device="cuda")
        lse = torch.empty(B, H, Sq, dtype=F32, device="cuda")
        recs = []
        for i, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
            mode = 1 if i == 0 else (3 if b == Sk else 2)
            with hip.launch_log() as log:
                out = hip.attn_fwd_acc(q, kk[:, a:b], vv[:, a:b], SCALE, True, 200 - a, oacc, lse, mode)
            recs += list(log)
        return out, lse, oacc, recs

    got, want = run(k, v), run(_expand(k, 2), _expand(v, 2))
    torch.cuda.synchronize()
    for a, b in zip(got[:3], want[:3]):
        assert torch.equal(a, b)
    assert got[3] == want[3] and [r["acc_mode"] for r in got[3]] == [1] + [2] * (len(cuts) - 1) + [3]


def _strides(t):
    return (ctypes.c_long * 3)(t.stride(0), t.stride(1), t.stride(2))


def _fwd_raw(fn, q, k, v, H, Hkv=None):
    hip = _hip()
    B, Sq = q.shape[:2]
    o = torch.empty_like(q)
    lse = torch.empty(B, H, Sq, dtype=F32, device="cuda")
    heads = (H,) if Hkv is None else (H, Hkv)
    with hip.launch_log() as log:
        rc = getattr(hip.lib(), fn)(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), B, Sq,
                                    k.shape[1], *heads, _strides(q), _strides(k), _strides(v), _strides(o), SCALE, 1, 0,
                                    hip._stream(q))
    torch.cuda.synchronize()
    return rc, o, lse, list(log)


def test_new_entry_with_one_group_is_the_old_entry():
    q, k, v, _ = _inputs(2, 6, 6, 256, 256, seed=3)
    old, new = _fwd_raw("ljs_attn_fwd", q, k, v, 6), _fwd_raw("ljs_attn_fwd_gqa", q, k, v, 6, 6)
    assert old[0] == 0 and new[0] == 0
    assert torch.equal(old[1], new[1]) and torch.equal(old[2], new[2])
    assert old[3] == new[3] and len(old[3]) == 1


# ----------------------------------------------------------------------------- 7. backward
def _bwd_pair(B, H, Hkv, Sq, Sk, causal, off, seed=0):
    """((dq, dk, dv), names) of the GQA backward block and of the baseline on expanded K / V."""
    hip = _hip()
    q, k, v, do = _inputs(B, H, Hkv, Sq, Sk, seed)
    G = H // Hkv
    kx, vx = _expand(k, G), _expand(v, G)
    o, lse = hip.attn_fwd_lse(q, kx, vx, SCALE, causal, off)
    with hip.launch_log() as base:
        want = hip.attn_bwd_block(q, kx, vx, o, do, lse, SCALE, causal, off)
    with hip.launch_log() as log:
        got = hip.attn_bwd_block(q, k, v, o, do, lse, SCALE, causal, off)
    torch.cuda.synchronize()
    return got, want, list(log), list(base)


def _check_bwd(B, H, Hkv, Sq, Sk, causal, off, inst):
    got, want, log, base = _bwd_pair(B, H, Hkv, Sq, Sk, causal, off)
    assert _names(base) == list(inst), (base, inst)
    # the baseline's instance(s) with their grids, then one gqa_reduce
    assert log[:-1] == base and log[-1]["name"] == "gqa_reduce" and len(log) == len(base) + 1, (log, base)
    assert torch.equal(got[0], want[0]), "dq"
    assert got[1].shape == (B, Sk, Hkv, 64) and got[2].shape == (B, Sk, Hkv, 64)
    assert torch.equal(got[1].cpu(), _fold(want[1], Hkv)), "dk"
    assert torch.equal(got[2].cpu(), _fold(want[2], Hkv)), "dv"


FUSED = [(2, 6, 2, 256, 256, False, 0, "attn_bwd_fused<dma=0,sw=1>"),
         (2, 6, 2, 256, 256, True, 0, "attn_bwd_fused<dma=0,sw=0>"),
         (2, 6, 2, 128, 256, False, 0, "attn_bwd_fused<dma=1,sw=1>")]


@pytest.mark.parametrize("B,H,Hkv,Sq,Sk,causal,off,inst", FUSED)
def test_backward_bits_fused(B, H, Hkv, Sq, Sk, causal, off, inst):
    hip = _hip()
    hip.set_attention_bwd_fused(True)
    try:
        _check_bwd(B, H, Hkv, Sq, Sk, causal, off, [inst])
    finally:
        hip.set_attention_bwd_fused(None)


PAIR32 = [(2, 6, 3, 192, 128, False, 0), (2, 6, 2, 320, 320, True, 0), (1, 4, 1, 200, 700, True, 500),
          (1, 2, 1, 1, 1, False, 0)]


@pytest.mark.parametrize("B,H,Hkv,Sq,Sk,causal,off", PAIR32)
def test_backward_bits_pair32(B, H, Hkv, Sq, Sk, causal, off):
    """The default below 128 (batch, head) pairs."""
    _check_bwd(B, H, Hkv, Sq, Sk, causal, off, ["attn_bwd_pair32<dq32=1>"])


@pytest.mark.parametrize("pair", [True, False], ids=["pair", "dq+dkv"])
def test_backward_bits_split(pair):
    hip = _hip()
    hip.set_attention_dkv32(False)
    hip.set_attention_bwd_pair(pair)
    try:
        _check_bwd(2, 6, 2, 130, 256, True, 64, ["attn_bwd_pair"] if pair else ["attn_bwd_dq", "attn_bwd_dkv"])
    finally:
        hip.set_attention_dkv32(None)
        hip.set_attention_bwd_pair(None)


def test_backward_column_block_destination():
    """k / v the adjacent column blocks of one [T][2 Hkv 64] buffer: dk and dv come back as the same
    column blocks of ONE fresh buffer, with the values of the dense run."""
    hip = _hip()
    B, H, Hkv, Sq, Sk = 2, 6, 2, 256, 256
    q, k, v, do = _inputs(B, H, Hkv, Sq, Sk, seed=4)
    buf = torch.empty(B, Sk, 2, Hkv, 64, dtype=BF16, device="cuda")
    buf[:, :, 0], buf[:, :, 1] = k, v
    kb, vb = buf[:, :, 0].requires_grad_(True), buf[:, :, 1].requires_grad_(True)
    q1 = q.clone().requires_grad_(True)
    with hip.launch_log() as log:
        dq, dk, dv = torch.autograd.grad(hip.attention(q1, kb, vb, SCALE, True, 0), [q1, kb, vb], do)
    q2, k2, v2 = (t.clone().requires_grad_(True) for t in (q, k, v))
    wq, wk, wv = torch.autograd.grad(hip.attention(q2, k2, v2, SCALE, True, 0), [q2, k2, v2], do)
    torch.cuda.synchronize()
    assert _names(log)[-1] == "gqa_reduce" and _names(log).count("gqa_reduce") == 1
    assert torch.equal(dq, wq) and torch.equal(dk, wk) and torch.equal(dv, wv)
    row = 2 * Hkv * 64
    assert dk.stride() == (Sk * row, row, 64, 1) and dv.stride() == dk.stride()
    assert dv.data_ptr() - dk.data_ptr() == Hkv * 64 * 2
    assert wk.is_contiguous()


# ----------------------------------------------------------------------------- 8. gqa_reduce alone
def _reduce_case(B, Sk, H, Hkv, layout, seed=0):
    gen = torch.Generator().manual_seed(seed + H + 10 * Hkv + Sk)
    dkx, dvx = (torch.randn(B, Sk, H, 64, generator=gen).to(BF16).cuda() for _ in range(2))
    if layout == "dense":
        dk, dv = (torch.empty(B, Sk, Hkv, 64, dtype=BF16, device="cuda") for _ in range(2))
    elif layout == "columns":
        buf = torch.full((B, Sk, 2, Hkv, 64), 7.0, dtype=BF16, device="cuda")
        dk, dv = buf[:, :, 0], buf[:, :, 1]
    else:
        dk, dv = (torch.empty(Sk, B, Hkv, 64, dtype=BF16, device="cuda").permute(1, 0, 2, 3) for _ in range(2))
    return dkx, dvx, dk, dv


@pytest.mark.parametrize("max_blocks", [None, 1], ids=["grid", "one-block"])
@pytest.mark.parametrize("B,Sk,H,Hkv,layout", [(2, 37, 4, 2, "dense"), (2, 37, 6, 2, "columns"), (3, 5, 8, 1, "seq-major"),
                                               (2, 1, 6, 3, "dense"), (1, 300, 16, 2, "columns")])
def test_gqa_reduce_bits(B, Sk, H, Hkv, layout, max_blocks):
    hip = _hip()
    dkx, dvx, dk, dv = _reduce_case(B, Sk, H, Hkv, layout)
    hip.set_gqa_max_blocks(max_blocks)
    try:
        with hip.launch_log() as log:
            hip.gqa_reduce(dkx, dvx, dk, dv)
        torch.cuda.synchronize()
    finally:
        hip.set_gqa_max_blocks(None)
    assert _names(log) == ["gqa_reduce"] and log[0]["block"] == 256
    items = 2 * B * Sk * Hkv * 8        # (tensor, batch, key, kv head, chunk): under a block per CU here
    assert log[0]["blocks"] == (1 if max_blocks else -(-items // 256))
    assert torch.equal(dk.cpu(), _fold(dkx, Hkv)) and torch.equal(dv.cpu(), _fold(dvx, Hkv))


def test_rejections_launch_nothing():
    hip = _hip()
    dkx, dvx, dk, dv = _reduce_case(2, 8, 4, 2, "dense")
    off = torch.empty(2 * 8 * 2 * 64 + 4, dtype=BF16, device="cuda")[4:].view(2, 8, 2, 64)   # 8 bytes off
    assert off.data_ptr() % 16 == 8
    odd = torch.empty(2, 8, 2, 68, dtype=BF16, device="cuda")[..., :64]                        # strides % 8 != 0
    with hip.launch_log() as log:
        assert hip.gqa_reduce_raw(dkx, dvx, off, dv) != 0
        assert hip.gqa_reduce_raw(dkx, dvx, dk, odd) != 0
        assert hip.gqa_reduce_raw(dkx[:, :, :3], dvx[:, :, :3], dk, dv) != 0      # 3 heads onto 2
        q, k, v, _ = _inputs(1, 6, 4, 64, 64)
        assert _fwd_raw("ljs_attn_fwd_gqa", q, k, v, 6, 4)[0] != 0
        assert _fwd_raw("ljs_attn_fwd_gqa", q, k, v, 6, 0)[0] != 0
        d = torch.empty(1, 6, 64, dtype=F32, device="cuda")
        out = [torch.empty_like(q) for _ in range(3)]
        rc = hip.lib().ljs_attn_bwd_gqa(q.data_ptr(), k.data_ptr(), v.data_ptr(), q.data_ptr(), q.data_ptr(),
                                        d.data_ptr(), d.data_ptr(), *[t.data_ptr() for t in out], 1, 64, 64, 6, 4,
                                        *[_strides(t) for t in (q, k, v, q, q, q, q, q)], SCALE, 0, 0, hip._stream(q))
        assert rc != 0
    torch.cuda.synchronize()
    assert log.total == 0 and not log
    with pytest.raises(ValueError, match="4 key/value heads"):
        hip.attn_fwd_lse(q, k, v, SCALE)
    with pytest.raises(ValueError, match="k has 4 heads and v has 2"):
        hip.attention(q, k, v[:, :, :2], SCALE)


# ----------------------------------------------------------------------------- 9. float64 oracle
def test_attention_against_the_oracle():
    """(2, 6, 2, 256, 256, causal) through hip.attention.  O, lse and dQ: attn_oracle.check / check_lse
    as they stand, on the expanded K / V.  dK / dV: the sum over the group of attn_oracle.bound's
    per-head allowances, plus 2^-7 |bf16(want)| for the final rounding (the triangle inequality over
    what tests/test_attention_oracle_gpu.py holds each head to)."""
    hip = _hip()
    B, H, Hkv, S, G = 2, 6, 2, 256, 3
    q, _, _, do = AO.inputs("plain", B, H, S, S, SCALE)
    _, k, v, _ = AO.inputs("plain", B, Hkv, S, S, SCALE)
    kx, vx = k.repeat_interleave(G, 2), v.repeat_interleave(G, 2)
    o64, lse64 = AO.forward(q, kx, vx, SCALE, True)
    m_o, m_lse = AO.forward(q, kx, vx, SCALE, True, rounded=True)
    want = AO.backward(q, kx, vx, o64, lse64, do, SCALE, True)
    model = AO.backward(q, kx, vx, m_o, m_lse, do, SCALE, True, rounded=True)
    qg, kg, vg = (t.cuda().requires_grad_(True) for t in (q, k, v))
    o = hip.attention(qg, kg, vg, SCALE, True, 0)
    dq, dk, dv = torch.autograd.grad(o, [qg, kg, vg], do.cuda())
    _, lse = hip.attn_fwd_lse(qg.detach(), kg.detach(), vg.detach(), SCALE, True, 0)
    torch.cuda.synchronize()
    AO.check("gqa o", o.detach().cpu(), o64, m_o)
    AO.check_lse(lse.cpu(), lse64, AO.lse2_f32(q, kx, SCALE, True, 0, device="cuda"), "gqa lse")
    AO.check("gqa dq", dq.cpu(), want[0], model[0])
    for name, got, w, m in (("gqa dk", dk, want[1], model[1]), ("gqa dv", dv, want[2], model[2])):
        per_head, _ = AO.bound(w, m, BF16, axis=1)
        w_sum = w.view(B, S, Hkv, G, 64).sum(3)
        allowed = per_head.view(B, S, Hkv, G, 64).sum(3) + 2.0 ** -7 * AO._bf16(w_sum).abs()
        err = (got.cpu().to(F64) - w_sum).abs()
        frac = (err / allowed).max().item()
        print(f"attn-figures {name} max_err={err.max().item():.3e} worst_fraction_of_bound={frac:.3f}")
        assert got.shape == w_sum.shape and torch.isfinite(got).all()
        assert frac <= 1.0, (name, err.max().item(), frac)


# ----------------------------------------------------------------------------- 10. gates
def test_fused_paths_refuse_grouped_kv():
    hip = _hip()
    B, H, Hkv, S, M = 32, 8, 2, 256, 128
    q, k, v, _ = _inputs(B, H, Hkv, S, S, seed=5)
    kx, vx = _expand(k, 4), _expand(v, 4)
    # the fused projection + forward's registry entry is not taken (and is left for its owner)
    o = torch.empty_like(q)
    lse = torch.empty(B, H, S, dtype=F32, device="cuda")
    hip._FUSED_ATTN[hip._fused_key(q, SCALE)] = (o.view(B * S, H * 64), lse, (B * S, 3 * H * 64), H)
    try:
        assert hip._take_fused_attention(q, k, v, SCALE, False, 0) is None
        assert len(hip._FUSED_ATTN) == 1
    finally:
        hip.clear_fused_attention()
    dy = torch.randn(B * S, M, device="cuda").to(BF16)
    w = torch.randn(H * 64, M, device="cuda").to(BF16)
    hip.set_attention_bwd_proj(True)
    try:
        assert hip.attn_bwd_proj_ok(q, kx, vx, o, dy, M, w, False)       # (the gate takes the shape itself)
        assert not hip.attn_bwd_proj_ok(q, k, v, o, dy, M, w, False)
        # a pending out-projection hand-over is materialised as the GEMM it stands for
        qg, kg, vg = (t.clone().requires_grad_(True) for t in (q, k, v))
        out = hip.attention(qg, kg, vg, SCALE, False, 0)
        dx = torch.randn(B, S, H, 64, device="cuda").to(BF16)
        ran = []
        before = dict(hip.ATTN_BWD_PROJ_STATS)
        hip.defer_out_proj(dy, M, w, dx, lambda: ran.append(1))
        with hip.launch_log() as log:
            torch.autograd.grad(out, [qg, kg, vg], dx)
        torch.cuda.synchronize()
        assert ran == [1] and not hip._PROJ_PENDING
        assert hip.ATTN_BWD_PROJ_STATS["materialised"] == before["materialised"] + 1
        assert hip.ATTN_BWD_PROJ_STATS["taken"] == before["taken"]
        assert "attn_bwd_proj" not in _names(log) and _names(log)[-1] == "gqa_reduce", log
    finally:
        hip._PROJ_PENDING.clear()
        hip.set_attention_bwd_proj(None)


def test_switch_runs_the_expanded_baseline(monkeypatch):
    """LJS_GQA_KERNELS=0: torch expands K / V in front of the multi-head kernels; forward and dQ are the
    same bits, dK / dV come from autograd's sum, and no gqa_reduce is recorded."""
    hip = _hip()
    B, H, Hkv, S = 2, 6, 2, 256
    q, k, v, do = _inputs(B, H, Hkv, S, S, seed=6)

    def run():
        ls = [t.clone().requires_grad_(True) for t in (q, k, v)]
        with hip.launch_log() as log:
            out = hip.attention(*ls, SCALE, True, 0)
            gs = torch.autograd.grad(out, ls, do)
        torch.cuda.synchronize()
        return out.detach(), gs, _names(log)

    o1, g1, n1 = run()
    monkeypatch.setenv("LJS_GQA_KERNELS", "0")
    o0, g0, n0 = run()
    assert torch.equal(o1, o0) and torch.equal(g1[0], g0[0])
    assert n1.count("gqa_reduce") == 1 and "gqa_reduce" not in n0
    assert [n for n in n1 if n.startswith("attn_")] == [n for n in n0 if n.startswith("attn_")]
    assert g0[1].shape == g1[1].shape == (B, S, Hkv, 64)
    for a, b in zip(g1[1:], g0[1:]):   # one more bf16 rounding per term on the baseline's side
        assert (a.float() - b.float()).abs().max() <= 2.0 ** -6 * a.float().abs().max()
