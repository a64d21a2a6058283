"""The head_dim 128 attention kernels (csrc/kernels/attention128.hip) against the float64 oracle of
tests/attn_oracle.py, inside the oracle module's own bound (run on a real MI355X: -m gpu).  D = 128,
scale 128 ** -0.5; cases are (B, H, Hkv, Sq, Sk, causal, q_offset).  Grouped heads take every G-th head
of the generated k / v; the oracle sees the repeat_interleaved copies and its dK / dV (and the rounding
model's) are summed in float64 over each group.  Every check prints one ``attn-figures`` line."""
import pytest
import torch

import attn_oracle as AO

pytestmark = pytest.mark.gpu

dev = torch.device("cuda", 0)
D, SCALE = 128, 128 ** -0.5

CASES = [(1, 1, 1, 1, 1, False, 0),          # a single key: dP - delta cancels exactly
         (1, 2, 2, 40, 40, False, 0),        # less than one tile in both axes
         (2, 4, 2, 128, 128, True, 0),       # exactly one query block, G = 2, the diagonal
         (1, 4, 1, 200, 200, True, 0),       # ragged tails, all heads on one K/V head
         (1, 2, 2, 130, 257, False, 0),      # a 2-row query tail, a 1-key tail after four tiles
         (1, 2, 1, 130, 256, True, 64),      # positive offset, boundary tile not on the block diagonal
         (1, 2, 2, 70, 130, True, -40),      # negative offset: rows with no key, lse = +inf, zero gradients
         (2, 8, 2, 320, 320, True, 0)]       # several query blocks and key tiles, skipped tiles, longest first
KIND_CASES = [CASES[2], CASES[4]]
PARAMS = [("plain", c) for c in CASES] + [(k, c) for k in ("peaked", "offset100") for c in KIND_CASES]


@pytest.fixture()
def hip(monkeypatch):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from learning_jax_sharding_amd.ops import hip as H
    H.lib()
    monkeypatch.setenv("LJS_ATTN_D128", "1")
    return H


_CACHE = {}


def _case(kind, case):
    """Inputs (bf16, CPU; k / v of Hkv heads), oracle and rounding model of one case, computed once."""
    if (kind, case) not in _CACHE:
        B, H, Hkv, Sq, Sk, causal, off = case
        G = H // Hkv
        q, k, v, do = AO.inputs(kind, B, H, Sq, Sk, SCALE, D=D)
        k, v = k[:, :, ::G].contiguous(), v[:, :, ::G].contiguous()
        kx, vx = k.repeat_interleave(G, 2), v.repeat_interleave(G, 2)
        c = {"q": q, "k": k, "v": v, "do": do}
        c["o"], c["lse2"] = AO.forward(q, kx, vx, SCALE, causal, off)
        c["m_o"], m_lse2 = AO.forward(q, kx, vx, SCALE, causal, off, rounded=True)
        c["ref32"] = AO.lse2_f32(q, kx, SCALE, causal, off)
        fold = lambda t: t.reshape(B, Sk, Hkv, G, D).sum(3)
        c["dq"], dk, dv = AO.backward(q, kx, vx, c["o"], c["lse2"], do, SCALE, causal, off)
        c["m_dq"], m_dk, m_dv = AO.backward(q, kx, vx, c["m_o"], m_lse2, do, SCALE, causal, off, rounded=True)
        c["dk"], c["dv"], c["m_dk"], c["m_dv"] = fold(dk), fold(dv), fold(m_dk), fold(m_dv)
        _CACHE[(kind, case)] = c
    return _CACHE[(kind, case)]


def _run(hip, c, causal, off):
    q, k, v, do = (c[n].to(dev) for n in ("q", "k", "v", "do"))
    o, lse = hip.attn_fwd_lse(q, k, v, SCALE, causal, off)
    return (o, lse) + tuple(hip.attn_bwd_block(q, k, v, o, do, lse, SCALE, causal, off))


@pytest.mark.parametrize("kind,case", PARAMS, ids=lambda p: p if isinstance(p, str) else "x".join(map(str, p)))
def test_attn128_matches_oracle(hip, kind, case):
    B, H, Hkv, Sq, Sk, causal, off = case
    c = _case(kind, case)
    with hip.launch_log() as log:
        o, lse, dq, dk, dv = _run(hip, c, causal, off)
    mask = int(causal or Sk % 64 != 0)
    nqb, nkt = -(-Sq // 128), -(-Sk // 64)
    assert [(r["name"], r["blocks"], r["block"]) for r in log] == [
        (f"attn128_fwd<mask={mask}>", nqb * H * B, 256), (f"attn128_bwd<mask={mask}>", (nqb * H + nkt * Hkv) * B, 256)]
    assert dk.shape == (B, Sk, Hkv, D) and dv.shape == dk.shape
    missed = []
    for name, got, axis in (("o", o, 1), ("dq", dq, 1), ("dk", dk, 1), ("dv", dv, 1)):
        try:
            AO.check(f"{kind} {case} {name}", got, c[name], c["m_" + name], axis)
        except AssertionError as e:
            missed.append(str(e)[:200])
    try:
        AO.check_lse(lse, c["lse2"], c["ref32"], f"{kind} {case} lse")
    except AssertionError as e:
        missed.append(str(e)[:200])
    assert not missed, missed
    if off < 0:   # rows that see no key: exact zeros, not merely small
        empty = torch.isposinf(c["lse2"]).permute(0, 2, 1).to(dev)
        assert empty.any() and not o[empty].any() and not dq[empty].any()


def test_attn128_same_bits_every_run(hip):
    case = CASES[7]
    c = _case("plain", case)
    a, b = _run(hip, c, case[5], case[6]), _run(hip, c, case[5], case[6])
    assert all(torch.equal(x.view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32),
                           y.view(torch.int16 if y.dtype == torch.bfloat16 else torch.int32)) for x, y in zip(a, b))


def test_attn128_fused_qkv_views(hip):
    """q / k / v as the column blocks of one [B, S, 3 H 128] buffer (strided, aligned): through
    hip.attention and autograd, with dq / dk / dv coming back as the column blocks of one buffer."""
    case = (1, 2, 2, 200, 200, True, 0)
    B, H, _, S, _, causal, off = case
    c = _case("plain", case)
    buf = torch.cat([c[n].reshape(B, S, H * D) for n in ("q", "k", "v")], -1).to(dev)
    q, k, v = (buf[..., i * H * D:(i + 1) * H * D].view(B, S, H, D).requires_grad_() for i in range(3))
    with hip.launch_log() as log:
        o = hip.attention(q, k, v, SCALE, causal, off)
        dq, dk, dv = torch.autograd.grad(o, (q, k, v), c["do"].to(dev))
    assert [r["name"] for r in log] == ["attn128_fwd<mask=1>", "attn128_bwd<mask=1>"]
    assert dq.stride() == q.stride() and dk.data_ptr() == dq.data_ptr() + 2 * H * D and \
        dv.data_ptr() == dq.data_ptr() + 4 * H * D
    for name, got in (("o", o), ("dq", dq), ("dk", dk), ("dv", dv)):
        AO.check(f"fused-views {name}", got, c[name], c["m_" + name])


def test_attn128_misaligned_view_runs_torch(hip):
    """A base 8 bytes off the 16-byte grid: the kernel entry rejects it and launches nothing, and
    kernels.attention returns the torch result."""
    from learning_jax_sharding_amd.ops import kernels as K
    case = CASES[1]
    B, H, _, Sq, Sk, causal, off = case
    c = _case("plain", case)
    flat = torch.zeros(c["q"].numel() + 4, dtype=torch.bfloat16, device=dev)
    q = flat[4:].view(c["q"].shape).copy_(c["q"])
    k, v = c["k"].to(dev), c["v"].to(dev)
    assert q.data_ptr() % 16 == 8
    with hip.launch_log() as log:
        with pytest.raises(RuntimeError, match="ljs_attn128_fwd"):
            hip.attn_fwd_lse(q, k, v, SCALE, causal, off)
    assert log.total == 0
    with pytest.warns(UserWarning, match="head_dim 128"):
        K._WARNED_DH.clear()
        o = K.attention(q, k, v, SCALE, causal, off)
    AO.check("misaligned o (torch)", o, c["o"], c["m_o"])
