"""A float64 oracle of scaled-dot-product attention, a model of the HIP kernels' roundings, and the
bound the attention tests hold an implementation to.  Plain torch on the CPU; nothing here reads
the package under test.

Tensors are ``[B, S, H, D]`` (batch, sequence, heads, head_dim); ``lse2`` is ``[B, H, Sq]``: log2 of
the partition function of the scaled scores, ``+inf`` for a query with no unmasked key (the HIP
kernels' convention).  With ``causal`` query ``i`` sees keys ``j <= i + q_offset``.

``forward`` / ``backward`` with ``rounded=False`` are the oracle.  ``rounded=True`` is the rounding
model: the same float64 arithmetic with values rounded to bf16 at the points where
``csrc/kernels/attention.hip`` rounds them (each marked below with the line that does it), plus
the f32 of the one difference that cancels, dP - delta; nowhere else.  Its distance from the
oracle is the error that the kernels' number formats alone explain; ``bound`` turns that into what
an output may differ by:

    E        max |model - oracle| over each 64-row tile of the sequence axis (all batches, heads, d)
    allowed  2^-7 |bf16(oracle)| + 4 E + 2^-23 max|oracle|      for a bf16 output
             4 E + 2^-23 max|oracle|                            for an f32 output

The factor 4 and the two floors are those of tests/test_norm_gpu.py and tests/test_xent_gpu.py (one
bf16 ulp of the rounded oracle; another equally valid evaluation order; outputs that are exact);
nothing is derived from the kernels' results."""
import math

import torch

LOG2E = math.log2(math.e)
TILE = 64
F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16


def _bf16(x):
    """Round an f64 tensor to bf16 (nearest even), back in f64."""
    return x.to(F32).to(BF16).to(F64)


def _f32(x):
    """Round an f64 tensor to f32, back in f64."""
    return x.to(F32).to(F64)


def scores(q, k, scale, causal=False, q_offset=0, dtype=F64):
    """(scaled scores [B,H,Sq,Sk] in ``dtype``, masked [Sq,Sk] bool: True where the key is not seen)."""
    s = torch.einsum("bqhd,bkhd->bhqk", q.to(dtype), k.to(dtype)) * scale
    Sq, Sk = q.shape[1], k.shape[1]
    if causal:
        qi = torch.arange(Sq, device=q.device)[:, None] + q_offset
        ki = torch.arange(Sk, device=q.device)[None, :]
        masked = ki > qi
    else:
        masked = torch.zeros(Sq, Sk, dtype=torch.bool, device=q.device)
    return s, masked


def forward(q, k, v, scale, causal=False, q_offset=0, rounded=False):
    """(o [B,Sq,H,D], lse2 [B,H,Sq]) in float64; a row with no unmasked key has o = 0, lse2 = +inf."""
    s, masked = scores(q, k, scale, causal, q_offset)
    s = s.masked_fill(masked, float("-inf"))
    m = s.amax(-1, keepdim=True)
    empty = torch.isneginf(m)
    m = torch.where(empty, torch.zeros_like(m), m)
    p = torch.exp(s - m)
    l = p.sum(-1, keepdim=True)
    lse2 = ((m + torch.log(l)) * LOG2E).squeeze(-1)
    lse2 = torch.where(empty.squeeze(-1), torch.full_like(lse2, float("inf")), lse2)
    p = p / torch.where(empty, torch.ones_like(l), l)
    if rounded:
        # attention.hip:5 "probabilities rounded to bf16"; :355 fwd_tile `pb = frag_acc(s[..], s[..])`
        # (pack_bf16x2 of the P tile that feeds the P . V MFMA), :418 the same in fwd_pv2
        p = _bf16(p)
    o = torch.einsum("bhqk,bkhd->bqhd", p, v.to(F64))
    if rounded:
        # attention.hip:249 store_row_T / :267 stage_rows16 `pack_bf16x2(acc * mul, ..)` (O = acc / l
        # to bf16), :476 fwd_store's merged output
        o = _bf16(o)
    return o, lse2


def backward(q, k, v, o, lse2, do, scale, causal=False, q_offset=0, rounded=False):
    """(dq, dk, dv) in float64 of the keys ``k`` / ``v`` alone, given the output ``o`` and the ``lse2``
    of the whole attention (all key blocks): one block of a blockwise backward, or with every key
    the backward itself.

        P = exp2(s log2e - lse2)   dP = dO V^T   delta = rowsum(dO o O)   dS = P o (dP - delta)
        dQ = scale dS K            dK = scale dS^T Q                     dV = P^T dO
    """
    q, k, v, o, do, lse2 = (t.to(F64) for t in (q, k, v, o, do, lse2))
    s, masked = scores(q, k, scale, causal, q_offset)
    p = torch.exp2(s * LOG2E - lse2[..., None])            # lse2 = +inf: exp2(-inf) = 0
    p = p.masked_fill(masked, 0.0)
    if rounded:
        # attention.hip:1026 delta_to_lds / :1379 dq_body / :1527 dq32_body / :1763 fused_delta: delta is
        # the dot product of the bf16 dO with the *stored* (bf16) O
        o = _bf16(o)
    dp = torch.einsum("bqhd,bkhd->bhqk", do, v)
    delta = (do * o).sum(-1).permute(0, 2, 1)[..., None]   # [B,H,Sq,1]
    if rounded:
        # The one place where the f32 of the accumulators shows: dP - delta cancels (to exactly 0
        # with a single key, where P = 1 and O = V), so what is left is the f32 rounding of its two
        # terms.  attention.hip:1384 dq_body `dl_q = -s` / :1031 delta_to_lds / :1224 dkv32_body
        # finish / :1531 dq32_body / :1767 fused_delta: delta is an f32 sum; :944 dkv_tile `dp =
        # rc.dl[t]` / :1115 dkv32_tile / :1316 dq_tile / :1458 dq32_tile / :1685 fused_tile `dp = ndl`:
        # the f32 dP accumulators start at -delta, so dP - delta leaves the MFMA chain as one f32
        delta = _f32(delta)
        dpd = _f32(dp - delta)
    else:
        dpd = dp - delta
    ds = p * dpd
    if rounded:
        # attention.hip:974 dkv_tile `pb = frag_acc(p[..])`, :1141 dkv32_tile / :1714 fused_tile
        # `pbu = pack_bf16x2(pv..)`: P to bf16 before dV^T = dO^T P
        p = _bf16(p)
        # attention.hip:975 dkv_tile `sb = frag_acc(ds[..])`, :1143 dkv32_tile, :1347 dq_tile,
        # :1486 dq32_tile, :1716 fused_tile `sbu = pack_bf16x2(dsv..)`: dS to bf16 before the dQ
        # and dK products
        ds = _bf16(ds)
    dq = scale * torch.einsum("bhqk,bkhd->bqhd", ds, k)
    dk = scale * torch.einsum("bhqk,bqhd->bkhd", ds, q)
    dv = torch.einsum("bhqk,bqhd->bkhd", p, do)
    if rounded:
        # attention.hip:249 store_row_T / :267 stage_rows16 (dK, dV; the split kernels' dQ), :1802
        # fused_dq_stage / :1980 the fused kernel's per-lane dQ: `pack_bf16x2(acc * scale, ..)`
        dq, dk, dv = _bf16(dq), _bf16(dk), _bf16(dv)
    return dq, dk, dv


def lse2_f32(q, k, scale, causal=False, q_offset=0, device="cpu"):
    """torch's own f32 evaluation of lse2 (logsumexp of f32 scores) on ``device``, as f64 on the
    CPU: the reference whose error sizes check_lse's tolerance."""
    s, masked = scores(q.to(device), k.to(device), scale, causal, q_offset, dtype=F32)
    lse = torch.logsumexp(s.masked_fill(masked, float("-inf")), -1) * LOG2E
    lse = torch.where(torch.isneginf(lse), torch.full_like(lse, float("inf")), lse)
    return lse.to(F64).cpu()


def _tile_max(err, axis=1):
    """max of ``err`` over each TILE-row tile of ``axis`` (and every other axis), per row of ``axis``."""
    S = err.shape[axis]
    other = [d for d in range(err.dim()) if d != axis]
    per_row = err.amax(other) if other else err
    n = -(-S // TILE)
    padded = torch.zeros(n * TILE, dtype=err.dtype)
    padded[:S] = per_row
    per_tile = padded.view(n, TILE).amax(1)
    return per_tile.repeat_interleave(TILE)[:S]


def bound(want64, model, got_dtype, axis=1):
    """(allowed [like want64], E per row of ``axis``): the module docstring's rule."""
    want64, model = want64.to(F64), model.to(F64)
    E = _tile_max((model - want64).abs(), axis)
    shape = [1] * want64.dim()
    shape[axis] = -1
    slack = 4.0 * E.view(shape) + 2.0 ** -23 * want64.abs().max()
    if got_dtype == BF16:
        allowed = 2.0 ** -7 * _bf16(want64).abs() + slack
    else:
        allowed = slack.expand_as(want64).clone()
    return allowed, E


def fraction(got, want64, model, axis=1):
    """(worst err / allowed over every element, max err, E): 0/0 counts as 0, x/0 as inf."""
    allowed, E = bound(want64, model, got.dtype, axis)
    want = _bf16(want64.to(F64)) if got.dtype == BF16 else want64.to(F64)
    err = (got.detach().to(F64).cpu() - want).abs()
    frac = torch.where(allowed > 0, err / allowed, torch.where(err > 0, torch.full_like(err, float("inf")),
                                                               torch.zeros_like(err)))
    frac = torch.nan_to_num(frac, nan=float("inf"), posinf=float("inf"))
    return frac.max().item(), err.max().item(), E


def check(name, got, want64, model, axis=1):
    """Assert one output (O, dQ: ``axis`` = the query axis; dK, dV: the key axis) against the bound;
    prints the figures first.  Returns the worst fraction of the bound."""
    frac, err, E = fraction(got, want64, model, axis)
    print(f"attn-figures {name} max_err={err:.3e} E_min={E.min().item():.3e} E_max={E.max().item():.3e} "
          f"worst_fraction_of_bound={frac:.3f}")
    assert torch.isfinite(got).all(), name
    assert frac <= 1.0, (name, err, frac)
    return frac


def check_lse(got, want64, ref32, name="lse"):
    """lse2 against the oracle: the same +inf pattern, and on the finite entries
    |got - want| <= 4 E_ref + 2^-23 |want|, E_ref the max error of ``ref32`` (lse2_f32)."""
    got = got.detach().to(F64).cpu()
    inf = torch.isposinf(want64)
    assert torch.equal(torch.isposinf(ref32), inf), name
    fin = ~inf
    e_ref = (ref32 - want64)[fin].abs().max().item() if fin.any() else 0.0
    err = (got - want64)[fin].abs()
    allowed = 4.0 * e_ref + 2.0 ** -23 * want64[fin].abs()
    frac = (err / allowed).max().item() if fin.any() else 0.0
    print(f"attn-figures {name} max_err={err.max().item() if fin.any() else 0.0:.3e} E_ref={e_ref:.3e} "
          f"inf_rows={int(inf.sum())} worst_fraction_of_bound={frac:.3f}")
    assert torch.equal(torch.isposinf(got), inf), name
    assert torch.isfinite(got[fin]).all(), name
    assert frac <= 1.0, (name, err.max().item(), e_ref, frac)
    return frac


KINDS = ("plain", "peaked", "offset100")


def inputs(kind, B, H, Sq, Sk, scale=0.125, D=64, seed=0):
    """(q, k, v, do) bf16 on the CPU from a seeded generator.  ``plain``: randn; ``peaked``: q and k
    times 3; ``offset100``: one vector c with scale |c|^2 = 100 added to every q row and every k
    row, so every score carries the common term 100 (exp of it overflows f32 unless the running
    max is subtracted first)."""
    assert kind in KINDS
    gen = torch.Generator(device="cpu").manual_seed(1000 * seed + 7 * Sq + 3 * Sk + 131 * B + H + KINDS.index(kind))
    q = torch.randn(B, Sq, H, D, generator=gen)
    k = torch.randn(B, Sk, H, D, generator=gen)
    v = torch.randn(B, Sk, H, D, generator=gen)
    do = torch.randn(B, Sq, H, D, generator=gen)
    if kind == "peaked":
        q, k = 3.0 * q, 3.0 * k
    elif kind == "offset100":
        c = torch.randn(D, generator=gen)
        c = c * math.sqrt(100.0 / scale) / c.norm()
        q, k = q + c, k + c
    return tuple(t.to(BF16) for t in (q, k, v, do))


_CACHE = {}


def case(kind, B, H, Sq, Sk, causal, q_offset, scale=0.125, bwd=True):
    """Inputs, oracle and model of one case, computed once and left unchanged: a dict with q, k, v,
    do (bf16), o, lse2 (oracle) and m_o, m_lse2 (model), and with ``bwd`` dq, dk, dv and m_dq, m_dk,
    m_dv; all f64."""
    key = (kind, B, H, Sq, Sk, causal, q_offset, scale)
    if key not in _CACHE:
        q, k, v, do = inputs(kind, B, H, Sq, Sk, scale)
        c = {"q": q, "k": k, "v": v, "do": do, "scale": scale, "causal": causal, "q_offset": q_offset}
        c["o"], c["lse2"] = forward(q, k, v, scale, causal, q_offset)
        c["m_o"], c["m_lse2"] = forward(q, k, v, scale, causal, q_offset, rounded=True)
        _CACHE[key] = c
    c = _CACHE[key]
    if bwd and "dq" not in c:
        q, k, v, do = c["q"], c["k"], c["v"], c["do"]
        c["dq"], c["dk"], c["dv"] = backward(q, k, v, c["o"], c["lse2"], do, scale, causal, q_offset)
        c["m_dq"], c["m_dk"], c["m_dv"] = backward(q, k, v, c["m_o"], c["m_lse2"], do, scale, causal, q_offset,
                                                   rounded=True)
    return c


# The shapes of tests/test_attention_oracle_gpu.py, (B, H, Sq, Sk, causal, q_offset); the CPU
# emulation of tests/test_attn_oracle.py runs on the same ones.
FWD_SHAPES = [(2, 3, 256, 256, False, 0), (2, 3, 256, 256, True, 0), (1, 2, 200, 200, True, 0),
              (1, 3, 40, 40, False, 0), (1, 1, 1, 1, False, 0), (2, 2, 130, 256, True, 64), (1, 2, 64, 100, True, 0),
              (1, 2, 100, 257, False, 0), (1, 2, 200, 700, True, 500), (1, 2, 70, 130, True, -40),
              (4, 64, 200, 200, True, 0)]
FWD_TILED_ONLY = [(1, 2, 100, 257, False, 0), (1, 2, 200, 700, True, 500)]
FWD_KIND_SHAPES = [(2, 3, 256, 256, True, 0), (1, 2, 200, 700, True, 500)]
BWD_SHAPES = [(2, 3, 256, 256, False, 0), (2, 3, 256, 256, True, 0), (2, 3, 192, 128, False, 0),
              (2, 3, 130, 256, True, 64), (1, 2, 64, 100, True, 0), (2, 3, 320, 320, True, 0),
              (1, 2, 200, 700, True, 500), (1, 2, 1, 1, False, 0)]
BWD_SPLIT_ONLY = [(2, 3, 320, 320, True, 0), (1, 2, 200, 700, True, 500)]
BWD_KIND_SHAPE = (2, 3, 256, 256, True, 0)
BWD_NEG_OFFSET = (1, 2, 70, 130, True, -40)
