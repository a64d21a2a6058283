"""Every attention kernel instance of csrc/kernels/attention.hip against the float64 oracle of
tests/attn_oracle.py, inside the bound measured from the rounding model (run on a real MI355X:
-m gpu).  D = 64, scale 0.125; shapes are (B, H, Sq, Sk, causal, q_offset).  Each case asserts from
the launch record which instance ran, and prints one ``attn-figures`` line per output
(profiles/attention/figures.txt)."""
import pytest
import torch

import attn_oracle as AO

pytestmark = pytest.mark.gpu

dev = torch.device("cuda", 0)
SCALE = 0.125
F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from learning_jax_sharding_amd.ops import hip as H
    H.lib()
    return H


def _sid(s):
    B, H, Sq, Sk, causal, off = s
    return f"{B}x{H}x{Sq}x{Sk}{'c' if causal else 'n'}{off:+d}"


def _all(tag, checks):
    """Run every (name, thunk) check, so that each prints its figures, then fail on any that missed."""
    missed = []
    for name, thunk in checks:
        try:
            thunk()
        except AssertionError as e:
            missed.append((name, str(e)[:200]))
    assert not missed, (tag, missed)


def _gpu(c, *names):
    return tuple(c[n].to(dev) for n in names)


def _assert_planned(hip, kind, log, causal, q_off, **ts):
    """The launcher's plan step (hip.attn_plan, under the switches now set) for the call on these
    tensors -- their real addresses and strides -- against the launch log, entry for entry."""
    q, k = ts["q"], ts["k"]
    plan = hip.attn_plan(kind, q.shape[0], q.shape[1], k.shape[1], q.shape[2], causal=causal, q_offset=q_off,
                         strides={n: hip._strides3(t) for n, t in ts.items()},
                         addrs={n: t.data_ptr() for n, t in ts.items()})
    keys = ("name", "grid", "block", "acc_mode")
    assert plan["err"] == 0 and [[r[x] for x in keys] for r in plan["launches"]] == [[r[x] for x in keys] for r in log], \
        (plan, list(log))


# ============================================================================ forward: O and lse
_FWD_RES = {"attn_fwd_tiled<1>": 0, "attn_fwd_res<4>": 4, "attn_fwd_res<8>": 8}


def _fwd_instances(shape):
    """The forward instances a shape can run: the resident ones up to 256 keys, 8 waves only from
    256 blocks of 128 queries (the launcher's demotion rule)."""
    B, H, Sq, Sk, _, _ = shape
    out = ["attn_fwd_tiled<1>"]
    if Sk <= 256:
        out.append("attn_fwd_res<4>")
        if -(-Sq // 128) * H * B >= 256:
            out.append("attn_fwd_res<8>")
    return out


_FWD_CASES = ([("plain", s, inst) for s in AO.FWD_SHAPES for inst in _fwd_instances(s)]
              + [(kind, s, inst) for kind in ("peaked", "offset100") for s in AO.FWD_KIND_SHAPES
                 for inst in _fwd_instances(s)])


def test_forward_cases_cover_what_they_claim():
    assert all(_fwd_instances(s) == ["attn_fwd_tiled<1>"] for s in AO.FWD_TILED_ONLY)
    assert {inst for _, _, inst in _FWD_CASES} == set(_FWD_RES)
    assert _fwd_instances((4, 64, 200, 200, True, 0))[-1] == "attn_fwd_res<8>"


@pytest.mark.parametrize("kind,shape,inst", _FWD_CASES, ids=[f"{k}-{_sid(s)}-{i}" for k, s, i in _FWD_CASES])
def test_forward_against_oracle(hip, kind, shape, inst):
    B, H, Sq, Sk, causal, q_off = shape
    c = AO.case(kind, *shape, bwd=False)
    q, k, v = _gpu(c, "q", "k", "v")
    hip.set_attention_fwd_resident(_FWD_RES[inst])
    try:
        with hip.launch_log() as log:
            o, lse = hip.attn_fwd_lse(q, k, v, SCALE, causal, q_off)
        torch.cuda.synchronize()
        _assert_planned(hip, "fwd", log, causal, q_off, q=q, k=k, v=v, o=o)
    finally:
        hip.set_attention_fwd_resident(-1)
    assert [(r["name"], r["acc_mode"]) for r in log] == [(inst, 0)], list(log)
    tag = f"{inst} {kind} {shape}"
    ref32 = AO.lse2_f32(c["q"], c["k"], SCALE, causal, q_off, device=dev)
    _all(tag, [("o", lambda: AO.check(f"{tag} o", o, c["o"], c["m_o"])),
               ("lse", lambda: AO.check_lse(lse, c["lse2"], ref32, name=f"{tag} lse"))])
    if q_off < 0:                                       # rows 0 .. -q_off - 1 see no key
        assert (o[:, :-q_off] == 0).all() and torch.isposinf(lse[:, :, :-q_off]).all()


# ============================================================================ merged forward (modes 1, 2, 3)
@pytest.mark.parametrize("mask", ["noncausal", "last_block_masked", "last_block_partly_masked"])
@pytest.mark.parametrize("sk,inst", [(128, "attn_fwd_res<4>"), (300, "attn_fwd_tiled<1>")])
def test_merged_forward_against_oracle(hip, sk, inst, mask):
    """Three key blocks merged in the kernels' epilogue.  Causal with q_off = sk the per-block offsets
    are sk, 0, -sk: the last block is fully masked; with q_off = sk + 37 partly.  The final O and the
    final running lse (state[1], which the blockwise backward consumes) against the oracle over all
    keys."""
    from learning_jax_sharding_amd.ops import kernels as K
    B, H, Sq = 2, 4, 128
    causal = mask != "noncausal"
    q_off = {"noncausal": 0, "last_block_masked": sk, "last_block_partly_masked": sk + 37}[mask]
    c = AO.case("plain", B, H, Sq, 3 * sk, causal, q_off, bwd=False)
    q, k, v = _gpu(c, "q", "k", "v")
    state, out = [None, None], None
    with hip.launch_log() as log:
        for i in range(3):
            out = K.attention_fwd_merge(q, k[:, i * sk:(i + 1) * sk], v[:, i * sk:(i + 1) * sk], SCALE, causal,
                                        q_off - i * sk, state, last=i == 2)
    torch.cuda.synchronize()
    assert [(r["name"], r["acc_mode"]) for r in log] == [(inst, m) for m in (1, 2, 3)], list(log)
    tag = f"{inst} merged sk={sk} {mask}"
    ref32 = AO.lse2_f32(c["q"], c["k"], SCALE, causal, q_off, device=dev)
    _all(tag, [("o", lambda: AO.check(f"{tag} o", out, c["o"], c["m_o"])),
               ("lse", lambda: AO.check_lse(state[1], c["lse2"], ref32, name=f"{tag} lse"))])


# ============================================================================ backward: dQ, dK, dV
# instance -> (fused, kv_dma, dkv32, dq32, pair): the switches that select it (None: the default)
_BWD_SWITCHES = {"attn_bwd_fused<dma=0>": (True, False, None, None, None),
                 "attn_bwd_fused<dma=1>": (True, True, None, None, None),
                 "attn_bwd_pair32<dq32=1>": (False, None, True, True, None),
                 "attn_bwd_pair32<dq32=0>": (False, None, True, False, None),
                 "attn_bwd_pair": (False, None, False, None, True),
                 "attn_bwd_dq+attn_bwd_dkv": (False, None, False, None, False)}
_FUSED, _SPLIT = list(_BWD_SWITCHES)[:2], list(_BWD_SWITCHES)[2:]


def _bwd_names(inst, shape):
    """The launch names of an instance at a shape: the fused kernel's sweep instance follows the
    shape (sw = 1: Sq % 64 == 0, Sk == 256, not causal, 16-byte aligned outputs)."""
    _, _, Sq, Sk, causal, _ = shape
    if inst.startswith("attn_bwd_fused"):
        sw = int(Sq % 64 == 0 and Sk == 256 and not causal)
        return [inst[:-1] + f",sw={sw}>"]
    return inst.split("+")


def _bwd_instances(shape):
    return (_FUSED if shape[3] <= 256 and shape not in AO.BWD_SPLIT_ONLY else []) + _SPLIT


class _switches:
    def __init__(self, hip, inst):
        self.hip, self.sw = hip, _BWD_SWITCHES[inst]

    def __enter__(self):
        fused, dma, dkv32, dq32, pair = self.sw
        self.hip.set_attention_bwd_fused(fused)
        self.hip.set_attention_bwd_kv_dma(dma)
        self.hip.set_attention_dkv32(dkv32)
        self.hip.set_attention_dq32(dq32)
        self.hip.set_attention_bwd_pair(pair)

    def __exit__(self, *exc):
        self.hip.set_attention_bwd_fused(None)
        self.hip.set_attention_bwd_kv_dma(None)
        self.hip.set_attention_dkv32(None)
        self.hip.set_attention_dq32(None)
        self.hip.set_attention_bwd_pair(None)


def _run_bwd(hip, inst, shape, q, k, v, o, do, lse, q_off=None, names_shape=None):
    """attn_bwd_block under the instance's switches (restored on the way out), the launch asserted."""
    causal = shape[4]
    with _switches(hip, inst):
        with hip.launch_log() as log:
            got = hip.attn_bwd_block(q, k, v, o, do, lse, SCALE, causal, shape[5] if q_off is None else q_off)
        torch.cuda.synchronize()
        _assert_planned(hip, "bwd", log, causal, shape[5] if q_off is None else q_off, q=q, k=k, v=v, o=o, dout=do,
                        dq=got[0], dk=got[1], dv=got[2])
    assert [r["name"] for r in log] == _bwd_names(inst, names_shape or shape), list(log)
    return got


def _check_grads(tag, c, dq, dk, dv):
    _all(tag, [("dq", lambda: AO.check(f"{tag} dq", dq, c["dq"], c["m_dq"])),
               ("dk", lambda: AO.check(f"{tag} dk", dk, c["dk"], c["m_dk"])),
               ("dv", lambda: AO.check(f"{tag} dv", dv, c["dv"], c["m_dv"]))])


_BWD_CASES = ([("plain", s, inst) for s in AO.BWD_SHAPES for inst in _bwd_instances(s)]
              + [(kind, AO.BWD_KIND_SHAPE, inst) for kind in ("peaked", "offset100")
                 for inst in ("attn_bwd_fused<dma=0>", "attn_bwd_pair32<dq32=1>")])


def test_backward_cases_cover_every_instance():
    names = {n for _, s, inst in _BWD_CASES for n in _bwd_names(inst, s)}
    assert names == {"attn_bwd_fused<dma=0,sw=0>", "attn_bwd_fused<dma=0,sw=1>", "attn_bwd_fused<dma=1,sw=0>",
                     "attn_bwd_fused<dma=1,sw=1>", "attn_bwd_pair32<dq32=0>", "attn_bwd_pair32<dq32=1>",
                     "attn_bwd_pair", "attn_bwd_dq", "attn_bwd_dkv"}
    assert all(_bwd_instances(s) == _SPLIT for s in AO.BWD_SPLIT_ONLY)


@pytest.mark.parametrize("kind,shape,inst", _BWD_CASES, ids=[f"{k}-{_sid(s)}-{i}" for k, s, i in _BWD_CASES])
def test_backward_against_oracle(hip, kind, shape, inst):
    """Every shape on every instance whose gate takes it.  At (1, 2, 1, 1, False, 0) the true dQ and
    dK are exactly 0 (one key: P = 1, dP = delta); what the kernels give there (dQ 1.6e-7, dK 1.4e-7,
    the same on all six instances) is the f32 rounding of dP - delta, which the model carries for
    this case (profiles/attention/figures.txt has the figures without and with it)."""
    B, H, Sq, Sk, causal, q_off = shape
    c = AO.case(kind, *shape)
    q, k, v, do = _gpu(c, "q", "k", "v", "do")
    o, lse = hip.attn_fwd_lse(q, k, v, SCALE, causal, q_off)
    dq, dk, dv = _run_bwd(hip, inst, shape, q, k, v, o, do, lse)
    _check_grads(f"{'+'.join(_bwd_names(inst, shape))} {kind} {shape}", c, dq, dk, dv)


@pytest.mark.parametrize("inst", list(_BWD_SWITCHES))
def test_backward_negative_offset(hip, inst):
    """q_offset = -40: queries 0 .. 39 see no key (lse = +inf).  Their dQ is exactly 0 and nothing
    is nan or inf.  (The kernels' causal bounds -- kend = min(Sk, q_offset + ..), qstart = max(0, ..) --
    only shorten the loops for a negative offset, and every load and store is guarded by the row
    index against Sq / Sk, never by the offset.)"""
    shape = AO.BWD_NEG_OFFSET
    B, H, Sq, Sk, causal, q_off = shape
    c = AO.case("plain", *shape)
    q, k, v, do = _gpu(c, "q", "k", "v", "do")
    o, lse = hip.attn_fwd_lse(q, k, v, SCALE, causal, q_off)
    assert torch.isposinf(lse[:, :, :-q_off]).all() and torch.isfinite(lse[:, :, -q_off:]).all()
    dq, dk, dv = _run_bwd(hip, inst, shape, q, k, v, o, do, lse)
    assert all(torch.isfinite(t).all() for t in (dq, dk, dv))
    assert (dq[:, :-q_off] == 0).all()
    _check_grads(f"{'+'.join(_bwd_names(inst, shape))} plain {shape}", c, dq, dk, dv)


@pytest.mark.parametrize("inst", ["attn_bwd_fused<dma=1>", "attn_bwd_pair32<dq32=1>"])
def test_backward_two_key_blocks(hip, inst):
    """A blockwise backward: 256 keys as two blocks of 128 with the global o / lse and the offsets
    128 and 0.  The dQ parts added in f32 and each block's dK / dV against the oracle over all keys;
    the model rounds each part to bf16 as the kernels do."""
    shape, sk = (2, 3, 128, 256, True, 128), 128
    B, H, Sq, Sk, causal, q_off = shape
    c = AO.case("plain", *shape)
    q, k, v, do = _gpu(c, "q", "k", "v", "do")
    o, lse = hip.attn_fwd_lse(q, k, v, SCALE, causal, q_off)
    parts, m_parts = [], []
    for i in range(2):
        sl = slice(i * sk, (i + 1) * sk)
        blk = (B, H, Sq, sk, causal, q_off - i * sk)
        parts.append(_run_bwd(hip, inst, blk, q, k[:, sl], v[:, sl], o, do, lse))
        m_parts.append(AO.backward(c["q"], c["k"][:, sl], c["v"][:, sl], c["m_o"], c["m_lse2"], c["do"], SCALE, causal,
                                   q_off - i * sk, rounded=True))
    dq = parts[0][0].float() + parts[1][0].float()
    dk, dv = (torch.cat([p[j] for p in parts], 1) for j in (1, 2))
    m_dq = m_parts[0][0] + m_parts[1][0]
    m_dk, m_dv = (torch.cat([p[j] for p in m_parts], 1) for j in (1, 2))
    tag = f"{_bwd_names(inst, (B, H, Sq, sk, causal, 0))[0]} two-blocks {shape}"
    _all(tag, [("dq", lambda: AO.check(f"{tag} dq(f32 sum)", dq, c["dq"], m_dq)),
               ("dk", lambda: AO.check(f"{tag} dk", dk, c["dk"], m_dk)),
               ("dv", lambda: AO.check(f"{tag} dv", dv, c["dv"], m_dv))])


@pytest.mark.parametrize("shape,fwd,bwd", [((2, 8, 256, 256, False, 0), "attn_fwd_res<4>", "attn_bwd_pair32<dq32=1>"),
                                           ((1, 4, 200, 200, True, 0), "attn_fwd_res<4>", "attn_bwd_pair32<dq32=1>")],
                         ids=["2x8x256n", "1x4x200c"])
def test_fused_qkv_slices_through_autograd(hip, shape, fwd, bwd):
    """q / k / v as slices of one [B, S, 3, H, 64] buffer through autograd of hip.attention: the
    strided operands and the backward that writes one dqkv buffer."""
    B, H, Sq, Sk, causal, q_off = shape
    c = AO.case("plain", *shape)
    qkv = torch.stack([c["q"], c["k"], c["v"]], 2).to(dev).requires_grad_(True)
    q, k, v = (qkv[:, :, i] for i in range(3))
    assert q.stride() == (Sq * 3 * H * 64, 3 * H * 64, 64, 1)
    with hip.launch_log() as log:
        out = hip.attention(q, k, v, SCALE, causal, q_off)
        out.backward(c["do"].to(dev))
    torch.cuda.synchronize()
    assert [r["name"] for r in log if r["name"].startswith("attn_")] == [fwd, bwd], list(log)
    g = qkv.grad
    tag = f"{fwd}+{bwd} qkv-slices {shape}"
    _all(tag, [("o", lambda: AO.check(f"{tag} o", out.detach(), c["o"], c["m_o"]))])
    _check_grads(tag, c, g[:, :, 0], g[:, :, 1], g[:, :, 2])


# ============================================================================ attn_bwd_proj, qkv_attn_fwd
def test_attn_bwd_proj_against_oracle(hip):
    """The fused backward that forms dO = dy . w^T itself, at the smallest shape its gate accepts
    (one (batch, head), 256 x 256, M = 32): the oracle forms dO in float64, the model rounds it to
    bf16 as the kernel's LDS image of it does."""
    B, H, S, M = 1, 1, 256, 32
    q, k, v, _ = AO.inputs("plain", B, H, S, S)
    gen = torch.Generator(device="cpu").manual_seed(5)
    w = (torch.randn(H * 64, M, generator=gen) * M ** -0.5).to(BF16)
    dy = torch.randn(B * S, M, generator=gen).to(BF16)
    do64 = (dy.to(F64) @ w.to(F64).t()).view(B, S, H, 64)
    o64, lse64 = AO.forward(q, k, v, SCALE)
    want = AO.backward(q, k, v, o64, lse64, do64, SCALE)
    m_o, m_lse = AO.forward(q, k, v, SCALE, rounded=True)
    # attention.hip:2023 "one rounding to bf16": dO_h leaves the projection's accumulators as bf16
    model = AO.backward(q, k, v, m_o, m_lse, do64.to(BF16), SCALE, rounded=True)
    qg, kg, vg, wg, dyg = (t.to(dev) for t in (q, k, v, w, dy))
    o, lse = hip.attn_fwd_lse(qg, kg, vg, SCALE)
    hip.set_attention_bwd_fused(True)
    hip.set_attention_bwd_proj(True)
    try:
        assert hip.attn_bwd_proj_ok(qg, kg, vg, o, dyg, M, wg, False)
        with hip.launch_log() as log:
            got = hip.attn_bwd_proj_block(qg, kg, vg, o, dyg, M, wg, lse, SCALE)
        torch.cuda.synchronize()
    finally:
        hip.set_attention_bwd_fused(None)
        hip.set_attention_bwd_proj(None)
    assert [r["name"] for r in log] == ["attn_bwd_proj"], list(log)
    tag = f"attn_bwd_proj plain {(B, H, S, S, False, 0)} M={M}"
    _all(tag, [(n, lambda n=n, g=g, a=a, b=b: AO.check(f"{tag} {n}", g, a, b))
               for n, g, a, b in zip(("dq", "dk", "dv"), got, want, model)])


def test_qkv_attn_fwd_against_oracle(hip):
    """The fused Q/K/V projection + forward at the smallest shape it accepts (one batch of 256
    tokens, K = 128): o and lse against the oracle evaluated on the q / k / v the kernel wrote."""
    B, H, K = 1, 2, 128
    T, N = B * 256, 64 * H
    gen = torch.Generator(device="cpu").manual_seed(6)
    x = torch.randn(T, K, generator=gen).to(BF16).to(dev)
    wt = (torch.randn(3, N, K, generator=gen) * 0.05).to(BF16).to(dev)
    out = torch.full((T, 3 * N), float("nan"), device=dev).to(BF16)
    with hip.launch_log() as log:
        o, lse = hip.qkv_attn_fwd(x, wt, out, H, SCALE)
    torch.cuda.synchronize()
    assert [r["name"] for r in log] == ["qkv_attn_fwd"], list(log)
    assert torch.isfinite(out).all()
    q, k, v = (out.view(B, 256, 3, H, 64)[:, :, i].cpu() for i in range(3))
    o64, lse64 = AO.forward(q, k, v, SCALE)
    m_o, _ = AO.forward(q, k, v, SCALE, rounded=True)
    tag = f"qkv_attn_fwd {(B, H, 256, 256, False, 0)} K={K}"
    ref32 = AO.lse2_f32(q, k, SCALE, device=dev)
    _all(tag, [("o", lambda: AO.check(f"{tag} o", o.view(B, 256, H, 64), o64, m_o)),
               ("lse", lambda: AO.check_lse(lse.view(B, H, 256), lse64, ref32, name=f"{tag} lse"))])
