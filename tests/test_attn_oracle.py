"""The attention oracle itself (tests/attn_oracle.py), on the CPU: it equals float64 autograd, the
package's torch fallbacks stay inside its bound, an independent f32 flash-style evaluation has room
under the bound, and the same evaluation with one deliberate mistake does not."""
import math

import pytest
import torch

import attn_oracle as AO

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
SCALE = 0.125


# ============================================================================ oracle against autograd
def _autograd(q, k, v, do, scale, causal, q_offset):
    """float64 autograd of the masked-softmax formulation; rows without a key give o = 0."""
    qs, ks, vs = (t.to(F64).requires_grad_(True) for t in (q, k, v))
    s = torch.einsum("bqhd,bkhd->bhqk", qs, ks) * scale
    Sq, Sk = q.shape[1], k.shape[1]
    keep = torch.ones(Sq, Sk, dtype=torch.bool)
    if causal:
        keep = torch.arange(Sk)[None, :] <= torch.arange(Sq)[:, None] + q_offset
    has = keep.any(-1)                                                  # [Sq]
    # a row with no key: softmax over an all -inf row is nan, so those rows are computed on
    # unmasked scores and then multiplied by 0 (their output and every gradient through them is 0)
    s = s.masked_fill(~(keep | ~has[:, None]), float("-inf"))
    p = torch.softmax(s, -1) * has[:, None].to(F64)
    o = torch.einsum("bhqk,bkhd->bqhd", p, vs)
    lse = torch.logsumexp(s, -1) * AO.LOG2E
    lse = torch.where(has, lse, torch.full_like(lse, float("inf")))
    dq, dk, dv = torch.autograd.grad(o, (qs, ks, vs), do.to(F64))
    return o.detach(), lse.detach(), dq, dk, dv


def _rel(a, b):
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-300)


@pytest.mark.parametrize("B,H,Sq,Sk,causal,q_offset", [(2, 2, 70, 70, False, 0), (2, 2, 70, 70, True, 0),
                                                       (1, 2, 50, 130, True, 64), (1, 2, 70, 130, True, -40),
                                                       (1, 1, 130, 40, True, 0), (1, 2, 33, 97, False, 0)])
def test_oracle_equals_float64_autograd(B, H, Sq, Sk, causal, q_offset):
    q, k, v, do = AO.inputs("plain", B, H, Sq, Sk)
    o, lse2 = AO.forward(q, k, v, SCALE, causal, q_offset)
    dq, dk, dv = AO.backward(q, k, v, o, lse2, do, SCALE, causal, q_offset)
    ro, rlse, rdq, rdk, rdv = _autograd(q, k, v, do, SCALE, causal, q_offset)
    assert torch.equal(torch.isposinf(lse2), torch.isposinf(rlse))
    fin = ~torch.isposinf(rlse)
    assert _rel(lse2[fin], rlse[fin]) <= 1e-12
    for name, a, b in (("o", o, ro), ("dq", dq, rdq), ("dk", dk, rdk), ("dv", dv, rdv)):
        assert _rel(a, b) <= 1e-12, (name, _rel(a, b))
    if q_offset < 0:
        n = -q_offset                                   # rows 0 .. n-1 see no key
        assert torch.isposinf(lse2[:, :, :n]).all() and fin[:, :, n:].all()
        assert (o[:, :n] == 0).all() and (dq[:, :n] == 0).all()
        assert (ro[:, :n] == 0).all() and (rdq[:, :n] == 0).all()
        # and the rounding model keeps them exactly 0 too
        mo, mlse = AO.forward(q, k, v, SCALE, causal, q_offset, rounded=True)
        mdq, _, _ = AO.backward(q, k, v, mo, mlse, do, SCALE, causal, q_offset, rounded=True)
        assert (mo[:, :n] == 0).all() and (mdq[:, :n] == 0).all()


def test_blockwise_backward_sums_to_the_whole():
    """backward() of each key block with the global o / lse2 and the per-block offset: the dQ parts
    sum to, and the dK / dV parts are, the backward over all keys."""
    B, H, Sq, sk, q_off = 1, 2, 70, 50, 60
    q, k, v, do = AO.inputs("plain", B, H, Sq, 3 * sk)
    o, lse2 = AO.forward(q, k, v, SCALE, True, q_off)
    dq, dk, dv = AO.backward(q, k, v, o, lse2, do, SCALE, True, q_off)
    parts = [AO.backward(q, k[:, i * sk:(i + 1) * sk], v[:, i * sk:(i + 1) * sk], o, lse2, do, SCALE, True,
                         q_off - i * sk) for i in range(3)]
    assert _rel(sum(p[0] for p in parts), dq) <= 1e-12
    assert _rel(torch.cat([p[1] for p in parts], 1), dk) <= 1e-12
    assert _rel(torch.cat([p[2] for p in parts], 1), dv) <= 1e-12


def test_bound_is_per_tile_and_checks_every_element():
    want = torch.zeros(1, 130, 1, 2, dtype=F64)
    want[0, :, 0, 0] = 1.0
    model = want.clone()
    model[0, 5, 0, 0] += 1e-3           # tile 0: E = 1e-3
    model[0, 129, 0, 1] += 1e-5         # tile 2 (rows 128..129): E = 1e-5; tile 1: E = 0
    allowed, E = AO.bound(want, model, BF16)
    assert torch.allclose(E[:64], torch.full((64,), 1e-3, dtype=F64)) and (E[64:128] == 0).all()
    assert torch.allclose(E[128:], torch.full((2,), 1e-5, dtype=F64))
    floor = 2.0 ** -23
    assert math.isclose(allowed[0, 70, 0, 0].item(), 2.0 ** -7 + floor)
    assert math.isclose(allowed[0, 70, 0, 1].item(), floor)
    got = want.to(BF16)
    assert AO.check("unit", got, want, model) == 0.0
    bad = got.clone()
    bad[0, 70, 0, 1] = 1e-4             # one element, in the tile whose E is 0
    with pytest.raises(AssertionError):
        AO.check("unit", bad, want, model)
    bad = got.clone()
    bad[0, 3, 0, 1] = float("nan")
    with pytest.raises(AssertionError):
        AO.check("unit", bad, want, model)


# ============================================================================ the package's torch fallbacks
@pytest.mark.parametrize("B,H,Sq,Sk,causal,q_offset", [(2, 3, 130, 130, False, 0), (1, 2, 100, 200, True, 64),
                                                       (1, 2, 70, 130, True, -40)])
def test_package_fallbacks_fwd_bwd(B, H, Sq, Sk, causal, q_offset):
    from learning_jax_sharding_amd.ops import kernels as K
    c = AO.case("plain", B, H, Sq, Sk, causal, q_offset)
    q, k, v, do = c["q"], c["k"], c["v"], c["do"]
    o, lse = K.attention_fwd_lse(q, k, v, SCALE, causal, q_offset)
    tag = f"fallback {(B, H, Sq, Sk, causal, q_offset)}"
    AO.check(f"{tag} o", o, c["o"], c["m_o"])
    AO.check_lse(lse, c["lse2"], AO.lse2_f32(q, k, SCALE, causal, q_offset), name=f"{tag} lse")
    dq, dk, dv = K.attention_bwd_block(q, k, v, o, do, lse, SCALE, causal, q_offset)
    AO.check(f"{tag} dq", dq, c["dq"], c["m_dq"])
    AO.check(f"{tag} dk", dk, c["dk"], c["m_dk"])
    AO.check(f"{tag} dv", dv, c["dv"], c["m_dv"])
    if q_offset < 0:
        assert (o[:, :-q_offset] == 0).all() and (dq[:, :-q_offset] == 0).all()


@pytest.mark.parametrize("causal,extra", [(False, 0), (True, 0), (True, 37)])
def test_package_fallback_merge(causal, extra):
    """Three key blocks; causal with q_off = sk the per-block offsets are sk, 0, -sk (the last block
    fully masked), with q_off = sk + 37 the last block is partly masked."""
    from learning_jax_sharding_amd.ops import kernels as K
    B, H, Sq, sk = 2, 2, 100, 100
    q_off = sk + extra if causal else 0
    c = AO.case("plain", B, H, Sq, 3 * sk, causal, q_off)
    q, k, v = c["q"], c["k"], c["v"]
    state, out = [None, None], None
    for i in range(3):
        out = K.attention_fwd_merge(q, k[:, i * sk:(i + 1) * sk], v[:, i * sk:(i + 1) * sk], SCALE, causal,
                                    q_off - i * sk, state, last=i == 2)
    tag = f"fallback-merge causal={int(causal)} q_off={q_off}"
    AO.check(f"{tag} o", out, c["o"], c["m_o"])
    AO.check_lse(state[1], c["lse2"], AO.lse2_f32(q, k, SCALE, causal, q_off), name=f"{tag} lse")


# ============================================================================ an independent f32 flash-style evaluation
# (delta taken from the unrounded instead of the bf16 O was tried as a fifth mistake: it stays inside
# the bound on every shape here -- worst dK fraction 0.424 against the unmutated 0.601 -- so it is no
# test of the bound's teeth; profiles/attention/figures.txt)
MUTATIONS = ("dq_times_1.05", "mask_ge", "l_without_last_tile", "lse_natural_log")


def emu_forward(q, k, v, scale, causal, q_offset, mut=None):
    """f32, 64-key tiles, online max, un-normalised P rounded to bf16 before P . V: (o bf16, lse2 f32)."""
    B, Sq, H, D = q.shape
    Sk = k.shape[1]
    qf, kf, vf = q.to(F32), k.to(F32), v.to(F32)
    sl2 = torch.tensor(scale * AO.LOG2E, dtype=F32)
    m = torch.full((B, H, Sq), float("-inf"), dtype=F32)
    l = torch.zeros(B, H, Sq, dtype=F32)
    o = torch.zeros(B, H, Sq, D, dtype=F32)
    qi = torch.arange(Sq)[:, None] + q_offset
    ntiles = -(-Sk // AO.TILE)
    for t in range(ntiles):
        k0, k1 = t * AO.TILE, min(Sk, (t + 1) * AO.TILE)
        s = torch.einsum("bqhd,bkhd->bhqk", qf, kf[:, k0:k1]) * sl2
        if causal:
            ki = torch.arange(k0, k1)[None, :]
            s = s.masked_fill((ki >= qi) if mut == "mask_ge" else (ki > qi), float("-inf"))
        m_new = torch.maximum(m, s.amax(-1))
        m_use = torch.where(torch.isneginf(m_new), torch.zeros_like(m_new), m_new)
        alpha = torch.exp2(m - m_use)
        p = torch.exp2(s - m_use[..., None])
        if not (mut == "l_without_last_tile" and t == ntiles - 1):
            l = l * alpha + p.sum(-1)
        else:
            l = l * alpha
        o = o * alpha[..., None] + torch.einsum("bhqk,bkhd->bhqd", p.to(BF16).to(F32), vf[:, k0:k1])
        m = m_new
    has = l > 0
    inv = torch.where(has, 1.0 / l, torch.zeros_like(l))
    o32 = (o * inv[..., None]).permute(0, 2, 1, 3).contiguous()
    lse2 = torch.where(has, m + torch.log2(l), torch.full_like(l, float("inf")))
    if mut == "lse_natural_log":
        lse2 = torch.where(has, lse2 / AO.LOG2E, lse2)
    return o32.to(BF16), lse2


def emu_backward(q, k, v, o, lse2, do, scale, causal, q_offset, mut=None):
    """f32 backward per 64-key tile from the emulation's own (o, lse2): bf16 (dq, dk, dv)."""
    B, Sq, H, D = q.shape
    Sk = k.shape[1]
    qf, kf, vf, dof = q.to(F32), k.to(F32), v.to(F32), do.to(F32)
    sl2 = torch.tensor(scale * AO.LOG2E, dtype=F32)
    delta = (dof * o.to(F32)).sum(-1).permute(0, 2, 1)[..., None]
    qi = torch.arange(Sq)[:, None] + q_offset
    dq = torch.zeros(B, Sq, H, D, dtype=F32)
    dk, dv = torch.zeros(B, Sk, H, D, dtype=F32), torch.zeros(B, Sk, H, D, dtype=F32)
    for t in range(-(-Sk // AO.TILE)):
        k0, k1 = t * AO.TILE, min(Sk, (t + 1) * AO.TILE)
        s = torch.einsum("bqhd,bkhd->bhqk", qf, kf[:, k0:k1])
        p = torch.exp2(s * sl2 - lse2[..., None])
        if causal:
            ki = torch.arange(k0, k1)[None, :]
            p = p.masked_fill((ki >= qi) if mut == "mask_ge" else (ki > qi), 0.0)
        dp = torch.einsum("bqhd,bkhd->bhqk", dof, vf[:, k0:k1])
        ds = (p * (dp - delta)).to(BF16).to(F32)
        dq += torch.einsum("bhqk,bkhd->bqhd", ds, kf[:, k0:k1])
        dk[:, k0:k1] = torch.einsum("bhqk,bqhd->bkhd", ds, qf)
        dv[:, k0:k1] = torch.einsum("bhqk,bqhd->bkhd", p.to(BF16).to(F32), dof)
    dq = dq * scale * (1.05 if mut == "dq_times_1.05" else 1.0)
    return dq.to(BF16), (dk * scale).to(BF16), dv.to(BF16)


def emulate(c, mut=None, bwd=True):
    q, k, v, do = c["q"], c["k"], c["v"], c["do"]
    o, lse2 = emu_forward(q, k, v, c["scale"], c["causal"], c["q_offset"], mut)
    got = {"o": o, "lse2": lse2}
    if bwd:
        got["dq"], got["dk"], got["dv"] = emu_backward(q, k, v, o, lse2, do, c["scale"], c["causal"], c["q_offset"],
                                                       mut)
    return got


def _check_all(tag, c, got):
    """check / check_lse of every output in ``got``, all of them before anything is raised: (the
    worst fraction per output, the names of those that missed)."""
    fr, missed = {}, []
    for name in got:
        try:
            if name == "lse2":
                ref32 = AO.lse2_f32(c["q"], c["k"], c["scale"], c["causal"], c["q_offset"])
                fr[name] = AO.check_lse(got["lse2"], c["lse2"], ref32, name=f"{tag} lse")
            else:
                fr[name] = AO.check(f"{tag} {name}", got[name], c[name], c["m_" + name])
        except AssertionError:
            missed.append(name)
    return fr, missed


def _emu_cases():
    """Every shape of tests/test_attention_oracle_gpu.py; forward and backward, but for the 256-head
    forward shape (forward only, as there)."""
    seen, out = set(), []
    for kind, shapes in (("plain", AO.FWD_SHAPES + AO.BWD_SHAPES + [AO.BWD_NEG_OFFSET]), ("peaked", AO.FWD_KIND_SHAPES),
                         ("offset100", AO.FWD_KIND_SHAPES)):
        for s in shapes:
            if (kind, s) not in seen:
                seen.add((kind, s))
                out.append((kind,) + s)
    return out


_WORST = {}


@pytest.mark.parametrize("kind,B,H,Sq,Sk,causal,q_offset", _emu_cases())
def test_bound_has_room_for_an_f32_flash_evaluation(kind, B, H, Sq, Sk, causal, q_offset):
    """An implementation other than the model -- f32, 64-key tiles, online max, un-normalised P to
    bf16, backward from its own f32 lse2 -- stays inside the bound: worst fraction 0.60 (dK, offset100
    at (1, 2, 200, 700, True, 500)), 0.41 on the plain inputs of more than one key.

    (1, 2, 1, 1, False, 0) is the case that needs the model's f32 rounding of dP - delta: with one
    key P = 1 and dP = delta, so the true dQ and dK are exactly 0, and a model with the bf16
    roundings alone is exactly 0 too and allows nothing, while every f32 evaluation keeps the
    rounding of the two cancelling sums (this one dQ 1.7e-7, dK 1.6e-7: over an allowed 0 without
    that rounding in the model, 0.55 and 0.56 of the bound with it)."""
    bwd = H <= 8
    c = AO.case(kind, B, H, Sq, Sk, causal, q_offset, bwd=bwd)
    fr, missed = _check_all(f"emulation {kind} {(B, H, Sq, Sk, causal, q_offset)}", c, emulate(c, bwd=bwd))
    for name, f in fr.items():
        _WORST[name] = max(_WORST.get(name, 0.0), f)
    print("attn-figures emulation worst so far " + " ".join(f"{n}={f:.3f}" for n, f in sorted(_WORST.items())))
    assert not missed, missed


# (mutation, the case it is shown on, the outputs that must miss the bound there)
_TEETH = [("dq_times_1.05", ("plain", 2, 3, 256, 256, True, 0), ("dq",)),
          ("dq_times_1.05", ("peaked", 2, 3, 256, 256, True, 0), ("dq",)),
          ("mask_ge", ("plain", 2, 3, 256, 256, True, 0), ("o", "lse2")),
          ("l_without_last_tile", ("plain", 2, 3, 256, 256, False, 0), ("o", "lse2")),
          ("l_without_last_tile", ("plain", 1, 2, 200, 700, True, 500), ("o", "lse2")),
          ("lse_natural_log", ("plain", 2, 3, 256, 256, False, 0), ("lse2", "dq", "dk", "dv"))]


@pytest.mark.parametrize("mut,case,outs", _TEETH, ids=[f"{m}-{c[0]}-{c[3]}x{c[4]}" for m, c, _ in _TEETH])
def test_bound_has_teeth(mut, case, outs):
    """The emulation with one deliberate mistake misses the bound on each named output (and the
    unmutated emulation passes on the same case: test_bound_has_room...)."""
    assert mut in MUTATIONS
    c = AO.case(*case)
    got = emulate(c, mut)
    ref32 = AO.lse2_f32(c["q"], c["k"], c["scale"], c["causal"], c["q_offset"])
    for name in outs:
        with pytest.raises(AssertionError):
            if name == "lse2":
                AO.check_lse(got["lse2"], c["lse2"], ref32, name=f"mutant {mut} lse")
            else:
                AO.check(f"mutant {mut} {name}", got[name], c[name], c["m_" + name])
