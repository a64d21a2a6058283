"""Per-device compute: hand-written HIP kernels on MI355X, torch on host devices.

Every function here takes and returns *local* torch tensors (one device's
shard).  On a ROCm tensor the call goes to the gfx950 HIP extension
(:mod:`.hip`); that path fails loudly if the extension is not built - there
is no silent torch fallback for GPU tensors (``LJS_ALLOW_TORCH_FALLBACK=1``
opts in, for debugging only).  Host-device (CPU) tensors use torch, which is
also the numerical oracle the GPU tests compare against.

Numerics follow the reference's bf16 recipe (``case6_attention.py:46,120-130``):
bf16 operands, f32 accumulation, f32 softmax, probabilities rounded to bf16
before P·V.
"""
from __future__ import annotations

import os
from typing import List, Optional, Sequence, Tuple

import torch

__all__ = ["cast", "reduce_sum", "dot_general", "linear", "softmax", "attention", "use_hip"]

_LOW = (torch.bfloat16, torch.float16)


def use_hip(t: torch.Tensor) -> bool:
    return t.is_cuda and not t.is_meta


def _hip():
    from . import hip
    return hip


# ----------------------------------------------------------------------------- casts / reductions
def cast(t: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    if t.dtype == dtype:
        return t
    if use_hip(t) and _hip().supports_cast(t.dtype, dtype):
        return _hip().cast(t, dtype)
    return t.to(dtype)


def reduce_sum(t: torch.Tensor, axes: Sequence[int], keepdim: bool, acc_dtype: torch.dtype) -> torch.Tensor:
    if not axes:
        return t.to(acc_dtype)
    if use_hip(t) and len(axes) == t.dim() and not keepdim:
        return _hip().sum_all(t, acc_dtype)
    return t.sum(dim=tuple(axes), keepdim=keepdim, dtype=acc_dtype)


def mse_loss(y: torch.Tensor, t: torch.Tensor, scale: float) -> torch.Tensor:
    """``scale * sum((y - t)^2)`` of one shard in f32 (fused HIP pass with its gradient on GPU)."""
    if use_hip(y):
        return _hip().mse_loss(y, t, scale)
    return ((y.float() - t.float()) ** 2).sum() * scale


# ----------------------------------------------------------------------------- layer / rms norm
def norm_reference(x: torch.Tensor, scale: Optional[torch.Tensor], bias: Optional[torch.Tensor], eps: float,
                   kind: str = "layer", out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """Plain torch LayerNorm (``kind='layer'``) / RMSNorm (``'rms'``, no bias) over the last dim:
    f32 statistics, the variance from the centred values."""
    xc = x.float()
    if kind == "layer":
        xc = xc - xc.mean(-1, keepdim=True)
    y = xc * torch.rsqrt((xc * xc).mean(-1, keepdim=True) + eps)
    if scale is not None:
        y = y * scale.float()
    if bias is not None and kind == "layer":
        y = y + bias.float()
    return y.to(out_dtype or x.dtype)


_WARNED_NORM_D = set()
_NORM_DTYPES = (torch.float32, torch.bfloat16)


def fused_norm_enabled() -> bool:
    # LJS_FUSED_NORM=0: LayerNorm / RMSNorm on GPU shards as the composite of elementwise and
    # reduction ops instead of the fused HIP kernels (A/B timing; escape hatch)
    return os.environ.get("LJS_FUSED_NORM", "1") != "0"


def _hip_norm(x: torch.Tensor, out_dtype: torch.dtype) -> bool:
    """Whether the fused HIP norm kernels take this shard: a GPU tensor, f32 or bf16 in and out, a
    feature count that is a multiple of 8 in 8..8192.  Another feature count on a GPU runs the
    torch formulation there, with a one-time warning per count."""
    if not use_hip(x) or not fused_norm_enabled():
        return False
    D = x.shape[-1] if x.dim() else 0
    if not (D % 8 == 0 and 8 <= D <= 8192):
        if D not in _WARNED_NORM_D:
            _WARNED_NORM_D.add(D)
            import warnings
            warnings.warn(f"HIP norm kernels take 8..8192 features in multiples of 8; {D} features run the torch "
                          "formulation on the GPU")
        return False
    return x.dtype in _NORM_DTYPES and out_dtype in _NORM_DTYPES and x.numel() > 0


def layer_norm(x: torch.Tensor, scale: Optional[torch.Tensor], bias: Optional[torch.Tensor], eps: float,
               kind: str = "layer", out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """LayerNorm / RMSNorm of one shard over its last dim (``scale`` / ``bias``: ``[D]`` or None)."""
    out_dtype = out_dtype or x.dtype
    if _hip_norm(x, out_dtype):
        return _hip().norm(x, scale, bias, eps, kind, out_dtype)
    return norm_reference(x, scale, bias, eps, kind, out_dtype)


# ----------------------------------------------------------------------------- softmax cross-entropy
def fused_xent_enabled() -> bool:
    # LJS_FUSED_XENT=0: softmax cross-entropy on GPU shards as the torch formulation below instead
    # of the fused HIP kernels of csrc/kernels/xent.hip (A/B timing; escape hatch)
    return os.environ.get("LJS_FUSED_XENT", "1") != "0"


def _hip_xent(logits: torch.Tensor, labels: torch.Tensor) -> bool:
    return use_hip(logits) and fused_xent_enabled() and _hip().xent_supported(logits, labels)


def xent_stats_reference(logits: torch.Tensor, labels: torch.Tensor, vocab_offset: int = 0):
    """Plain torch ``(m, log s, t)`` of one vocabulary shard over its last dim, in f64 for f64 logits
    (the oracle) and f32 otherwise: ``m`` the row maximum (a constant to autograd), ``s = sum exp(x - m)``,
    ``t = x[label] - m`` where ``vocab_offset <= label < vocab_offset + V``, else 0."""
    x = logits if logits.dtype == torch.float64 else logits.float()
    V = x.shape[-1]
    m = x.detach().amax(-1)
    s = torch.exp(x - m.unsqueeze(-1)).sum(-1)
    col = labels.long() - int(vocab_offset)
    own = (labels >= 0) & (col >= 0) & (col < V)
    xl = torch.gather(x, -1, col.clamp(0, V - 1).unsqueeze(-1)).squeeze(-1)
    t = torch.where(own, xl - m, torch.zeros_like(m))
    return m, torch.log(s), t


def softmax_xent_reference(logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """Plain torch ``log(sum exp(x - m)) - (x[label] - m)`` per row, 0 where the label is negative."""
    m, ls, t = xent_stats_reference(logits, labels, 0)
    return torch.where(labels >= 0, ls - t, torch.zeros_like(ls))


def softmax_xent(logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """Softmax cross-entropy rows of one shard that holds the whole vocabulary: f32 of shape
    ``logits.shape[:-1]``; a label < 0 marks an ignored row (loss 0, zero gradient)."""
    if _hip_xent(logits, labels):
        return _hip().xent(logits, labels)
    return softmax_xent_reference(logits, labels)


def softmax_xent_stats(logits: torch.Tensor, labels: torch.Tensor, vocab_offset: int = 0):
    """``(m, log s, t)`` of one vocabulary shard whose column 0 is global column ``vocab_offset``."""
    if _hip_xent(logits, labels):
        return _hip().xent_stats(logits, labels, vocab_offset)
    return xent_stats_reference(logits, labels, vocab_offset)


# ----------------------------------------------------------------------------- embedding lookup
# whether LJS_FUSED_EMBED=1 (the default) includes the deterministic fused backward, or only the
# forward with torch's index_add_ behind it (profiles/PERF_NOTES.md "Fused embedding")
_EMBED_BWD_BY_DEFAULT = True


def fused_embed_mode() -> int:
    # LJS_FUSED_EMBED=0: the embedding lookup on GPU shards as the torch formulation below instead of
    # the fused HIP kernels of csrc/kernels/embed.hip (A/B timing; escape hatch); 1 (default): the
    # fused kernels; 2: the fused forward and the deterministic fused backward whatever the default
    v = os.environ.get("LJS_FUSED_EMBED", "1")
    return 0 if v == "0" else (2 if v == "2" else 1)


def fused_embed_enabled() -> bool:
    return fused_embed_mode() != 0


def _hip_embed(table: torch.Tensor, ids: torch.Tensor, out_dtype: Optional[torch.dtype] = None) -> bool:
    return (use_hip(table) and use_hip(ids) and fused_embed_enabled()
            and _hip().embed_supported(table, ids, out_dtype))


def embed_reference(table: torch.Tensor, ids: torch.Tensor, vocab_offset: int = 0,
                    out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """Plain torch ``table[ids - vocab_offset]`` as ``[*ids.shape, D]``: a row of zeros where ``ids -
    vocab_offset`` is outside ``[0, V)`` (a mask, a clamped index and ``where``), in the table's dtype
    (f64 for an f64 table: the oracle) cast to ``out_dtype``; the backward is torch's."""
    V = table.shape[0]
    loc = ids.long() - int(vocab_offset)
    own = (loc >= 0) & (loc < V)
    rows = table[loc.clamp(0, V - 1)]
    rows = torch.where(own.unsqueeze(-1), rows, torch.zeros((), dtype=rows.dtype, device=rows.device))
    return rows if out_dtype is None or out_dtype == rows.dtype else rows.to(out_dtype)


def embed(table: torch.Tensor, ids: torch.Tensor, vocab_offset: int = 0,
          out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """Rows of one table shard (``[V, D]``, its row 0 global id ``vocab_offset``) by id; an id the shard
    does not hold gives a row of zeros and no gradient."""
    if _hip_embed(table, ids, out_dtype):
        mode = fused_embed_mode()
        return _hip().embed(table, ids, vocab_offset, out_dtype, fused_bwd=mode == 2 or _EMBED_BWD_BY_DEFAULT)
    return embed_reference(table, ids, vocab_offset, out_dtype)


# ----------------------------------------------------------------------------- rotary embedding
# Convention (pinned by tests/test_rope.py): half-split pairs, as in MaxText and Llama-HF.  For a head
# vector x[0:D] at global position p, with h = D / 2 and i in [0, h):
#
#     ang      = p * theta^(-2 i / D)
#     y[i]     = x[i]     cos(ang) - x[i + h] sin(ang)
#     y[i + h] = x[i + h] cos(ang) + x[i]     sin(ang)
#
# and the backward is the same map with -ang.  cos / sin come from a table: the angle and its cos /
# sin in float64 on the host, rounded once to f32, [P][h] each.  (Evaluated in f32, p * inv_freq
# alone would be off by about p * 2^-24 radians.)
_ROPE_MIN_ROWS = 1024


def rope_table_host(rows: int, D: int, theta: float, start: int = 0, dtype: torch.dtype = torch.float32):
    """(cos, sin) of positions ``start .. start + rows``, ``[rows, D / 2]`` each: the angle ``p *
    theta^(-2 i / D)`` and its cos / sin in float64, rounded once to ``dtype`` (float64: the oracle's
    table).  Pure host arithmetic."""
    if D < 2 or D % 2:
        raise ValueError(f"rope: head_dim must be even, got {D}")
    import numpy as np
    inv_freq = np.power(np.float64(theta), -2.0 * np.arange(D // 2, dtype=np.float64) / D)
    ang = np.arange(start, start + rows, dtype=np.float64)[:, None] * inv_freq[None, :]
    return torch.from_numpy(np.cos(ang)).to(dtype), torch.from_numpy(np.sin(ang)).to(dtype)


class RopeTableCache:
    """The f32 tables per (device, D, theta).  A table grows by doubling; a superseded table stays
    alive, because a captured graph holds its address.  A table is created only outside a graph
    capture (``jit``'s warm-up call does that): a capture that needs more rows than exist raises."""

    def __init__(self):
        self.live = {}         # key -> (cos, sin)
        self.superseded = []   # every table a longer one replaced

    @staticmethod
    def _key(device: torch.device, D: int, theta: float):
        return (device.type, device.index, int(D), float(theta))

    def get(self, device: torch.device, D: int, theta: float, rows: int):
        """(cos, sin) on ``device`` with at least ``rows`` rows."""
        key = self._key(device, D, theta)
        cur = self.live.get(key)
        if cur is not None and cur[0].shape[0] >= rows:
            return cur
        if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError(
                f"rope: the cos/sin table for head_dim {D}, theta {theta} on {device} has "
                f"{0 if cur is None else cur[0].shape[0]} rows and {rows} are needed, and a table cannot be "
                "created during a graph capture: run the function once outside the capture first")
        n = _ROPE_MIN_ROWS if cur is None else 2 * cur[0].shape[0]
        while n < rows:
            n *= 2
        cos, sin = rope_table_host(n, D, theta)
        new = (cos.to(device), sin.to(device))
        if cur is not None:
            self.superseded.append(cur)
        self.live[key] = new
        return new


_ROPE_TABLES = RopeTableCache()


def rope_table(device: torch.device, D: int, theta: float, rows: int):
    return _ROPE_TABLES.get(device, D, theta, rows)


def fused_rope_enabled() -> bool:
    # LJS_FUSED_ROPE=0: the rotary embedding on GPU shards as the torch formulation below instead of
    # the fused HIP kernel of csrc/kernels/rope.hip (A/B timing; escape hatch)
    return os.environ.get("LJS_FUSED_ROPE", "1") != "0"


def _rope_one(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, out_dtype: torch.dtype) -> torch.Tensor:
    h = x.shape[-1] // 2
    xf = x.float()
    a, b = xf[..., :h], xf[..., h:]
    return torch.cat([a * cos - b * sin, b * cos + a * sin], dim=-1).to(out_dtype)


def rope_reference(q: torch.Tensor, k: Optional[torch.Tensor] = None, pos_offset: int = 0, theta: float = 10000.0,
                   out_dtype: Optional[torch.dtype] = None):
    """Plain torch rotary embedding of ``(B, S, H, D)`` shards whose first position is ``pos_offset``,
    from the same f32 table as the HIP kernel and in f32 arithmetic: ``(q', k')`` (``k'`` None without
    ``k``).  The backward is torch's: the rotation by ``-ang`` of the cotangent."""
    S, D = q.shape[1], q.shape[-1]
    cos, sin = rope_table(q.device, D, theta, pos_offset + S)
    cos = cos[pos_offset:pos_offset + S].view(1, S, 1, D // 2)
    sin = sin[pos_offset:pos_offset + S].view(1, S, 1, D // 2)
    qo = _rope_one(q, cos, sin, out_dtype or q.dtype)
    return qo, (None if k is None else _rope_one(k, cos, sin, out_dtype or k.dtype))


_WARNED_ROPE_D = set()


def _hip_rope(q: torch.Tensor, k: Optional[torch.Tensor], out_dtype: Optional[torch.dtype]) -> bool:
    """Whether the fused HIP kernel takes these shards: GPU tensors ``(B, S, H, D)``, f32 or bf16 in
    and out, D a multiple of 16 in 16..256 contiguous, bases and strides 16-byte aligned.  Anything
    else on a GPU runs the torch formulation there, with a one-time warning per D."""
    if not use_hip(q) or not fused_rope_enabled():
        return False
    ts = [q] + ([k] if k is not None else [])
    D = q.shape[-1]
    ok = all(t.shape == q.shape and t.dtype == q.dtype and _hip().rope_supported(t, out_dtype) for t in ts)
    if not ok and D not in _WARNED_ROPE_D:
        _WARNED_ROPE_D.add(D)
        import warnings
        warnings.warn(f"HIP rope kernel takes f32 / bf16 (B, S, H, D) shards with D a multiple of 16 in 16..256 and "
                      f"16-byte aligned bases and strides; {q.dtype} {tuple(q.shape)} strides {q.stride()} runs the "
                      "torch formulation on the GPU")
    return ok


def rope(q: torch.Tensor, k: Optional[torch.Tensor] = None, pos_offset: int = 0, theta: float = 10000.0,
         out_dtype: Optional[torch.dtype] = None):
    """Rotary embedding of one device's ``(B, S, H, D)`` shards of q and (optionally) k, whose first
    position is ``pos_offset``: ``(q', k')``, one HIP launch for both on a GPU."""
    if _hip_rope(q, k, out_dtype):
        return _hip().rope(q, k, pos_offset, theta, out_dtype)
    return rope_reference(q, k, pos_offset, theta, out_dtype)


# ----------------------------------------------------------------------------- SwiGLU
# h = silu(g) u = g sigma(g) u, the activation of a gated feed-forward.  With e = exp(-|g|) and
# r = 1 / (1 + e): sigma = r for g >= 0 and e r below, c = 1 - sigma = e r for g >= 0 and r below: one exp
# of a non-positive argument, and c never formed by subtraction (which loses it once sigma rounds
# to 1).  The backward recomputes them from g: du = dh sigma g, dg = dh sigma u (1 + g c).
def fused_swiglu_enabled() -> bool:
    # LJS_FUSED_SWIGLU=0: the gated feed-forward's activation on GPU shards as the torch formulation
    # below instead of the fused HIP kernels of csrc/kernels/swiglu.hip (A/B timing; escape hatch)
    return os.environ.get("LJS_FUSED_SWIGLU", "1") != "0"


def _sigmoid_pair(g: torch.Tensor):
    e = torch.exp(-g.abs())
    r = 1.0 / (1.0 + e)
    er = e * r
    pos = g >= 0
    return torch.where(pos, r, er), torch.where(pos, er, r)


class _SwigluReference(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g, u, out_dtype):
        ctx.save_for_backward(g, u)
        gf, uf = (t if t.dtype == torch.float64 else t.float() for t in (g, u))
        sg, _ = _sigmoid_pair(gf)
        return (gf * sg * uf).to(out_dtype)

    @staticmethod
    def backward(ctx, dh):
        g, u = ctx.saved_tensors
        gf, uf, df = (t if t.dtype == torch.float64 else t.float() for t in (g, u, dh))
        sg, c = _sigmoid_pair(gf)
        ds = df * sg
        dg = ds * uf * (1.0 + gf * c) if ctx.needs_input_grad[0] else None
        du = ds * gf if ctx.needs_input_grad[1] else None
        return (None if dg is None else dg.to(g.dtype)), (None if du is None else du.to(u.dtype)), None


def swiglu_reference(g: torch.Tensor, u: torch.Tensor, out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """Plain torch ``silu(g) * u`` by the stable formulas above: f32 arithmetic (f64 for f64 inputs), one
    rounding to ``out_dtype`` (default: g's), and an explicit backward by the same formulas (not the
    autograd of a ``silu * u`` composite)."""
    return _SwigluReference.apply(g, u, out_dtype or g.dtype)


_WARNED_SWIGLU = set()


def _hip_swiglu(g: torch.Tensor, u: torch.Tensor, out_dtype: Optional[torch.dtype]) -> bool:
    """Whether the fused HIP kernels take these shards: GPU tensors of one shape, f32 or bf16 in and
    out, the last dim a contiguous multiple of 8, bases and strides 16-byte aligned.  Anything else on
    a GPU runs the torch formulation there, with a one-time warning per feature count."""
    if not use_hip(g) or not use_hip(u) or not fused_swiglu_enabled():
        return False
    ok = _hip().swiglu_supported(g, u, out_dtype)
    F = g.shape[-1] if g.dim() else 0
    if not ok and F not in _WARNED_SWIGLU:
        _WARNED_SWIGLU.add(F)
        import warnings
        warnings.warn(f"HIP swiglu kernels take f32 / bf16 shards whose last dim is a contiguous multiple of 8 with "
                      f"16-byte aligned bases and strides; {g.dtype} {tuple(g.shape)} strides {g.stride()} (u "
                      f"{u.dtype} strides {u.stride()}) runs the torch formulation on the GPU")
    return ok


def swiglu(g: torch.Tensor, u: torch.Tensor, out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """``silu(g) * u`` of one device's shards of the gate and up projections, in ``out_dtype`` (default:
    g's): one HIP launch forward and one backward on a GPU."""
    if _hip_swiglu(g, u, out_dtype):
        return _hip().swiglu(g, u, out_dtype)
    return swiglu_reference(g, u, out_dtype)


# ----------------------------------------------------------------------------- matmuls
def _to_bmk(a: torch.Tensor, batch, free, contract):
    perm = list(batch) + list(free) + list(contract)
    x = a.permute(perm)
    B = 1
    for i in batch:
        B *= a.shape[i]
    M = 1
    for i in free:
        M *= a.shape[i]
    Kd = 1
    for i in contract:
        Kd *= a.shape[i]
    return x.reshape(B, M, Kd)


def dot_general(a: torch.Tensor, b: torch.Tensor, lc, rc, lb, rb, out_dtype: torch.dtype) -> torch.Tensor:
    lf = [i for i in range(a.dim()) if i not in lc and i not in lb]
    rf = [i for i in range(b.dim()) if i not in rc and i not in rb]
    A = _to_bmk(a, lb, lf, lc)                       # (B, M, K)
    Bt = _to_bmk(b, rb, rf, rc)                      # (B, N, K)
    out_shape = [a.shape[i] for i in lb] + [a.shape[i] for i in lf] + [b.shape[i] for i in rf]
    if use_hip(a):
        C = _hip().bmm_nt(A, Bt, out_dtype)          # C[b] = A[b] @ Bt[b]^T
    else:
        if A.dtype in _LOW or Bt.dtype in _LOW:
            C = torch.bmm(A.float(), Bt.float().transpose(1, 2)).to(out_dtype)
        else:
            C = torch.bmm(A.to(out_dtype if out_dtype.is_floating_point else A.dtype),
                          Bt.to(out_dtype if out_dtype.is_floating_point else Bt.dtype).transpose(1, 2)).to(out_dtype)
    return C.reshape(out_shape)


def linear(x: torch.Tensor, ws: Sequence[torch.Tensor], b: Optional[torch.Tensor], compute_dtype: torch.dtype,
           relu: bool = False, out_dtype: Optional[torch.dtype] = None, fp8: bool = False,
           residual: Optional[torch.Tensor] = None) -> List[torch.Tensor]:
    """``[x @ w (+ b)(relu) for w in ws]`` in ``compute_dtype`` (flax ``Dense`` semantics);
    ``fp8`` = MX-fp8 forward GEMMs (HIP block-scaled MFMA, exact emulation on CPU).
    ``residual`` (one kernel): ``out + residual`` in the output dtype, both operands rounded to
    it first (the GPU fuses the add into the GEMM epilogue)."""
    out_dtype = out_dtype or compute_dtype
    if fp8:
        from . import fp8 as F8
        outs = [F8.linear_fp8(x, w, b, relu, out_dtype) for w in ws]
        if residual is not None:
            outs[0] = outs[0] + residual.to(outs[0].dtype)
        return outs
    if use_hip(x):
        return _hip().linear(x, list(ws), b, compute_dtype, relu, out_dtype, residual=residual)
    if residual is not None:
        outs = linear(x, ws, b, compute_dtype, relu, out_dtype)
        return [outs[0] + residual.to(outs[0].dtype)] + outs[1:]
    lead = x.shape[:-1]
    x2 = x.reshape(-1, x.shape[-1])
    xc = x2.to(compute_dtype)
    outs = []
    for w in ws:
        wc = w.to(compute_dtype)
        if compute_dtype in _LOW:
            y = xc.float() @ wc.float()
            if b is not None:
                y = y + b.to(compute_dtype).float()
        else:
            y = xc @ wc
            if b is not None:
                y = y + b.to(compute_dtype)
        if relu:
            y = torch.relu(y)
        outs.append(y.to(out_dtype).reshape(tuple(lead) + (w.shape[-1],)))
    return outs


# ----------------------------------------------------------------------------- softmax / attention
def softmax(t: torch.Tensor, axis: int) -> torch.Tensor:
    if use_hip(t) and axis % t.dim() == t.dim() - 1 and t.dtype == torch.float32:
        return _hip().softmax_lastdim(t)
    return torch.softmax(t.float(), dim=axis).to(t.dtype)


def kv_groups(q, k, v) -> int:
    """G = heads // kv_heads of (b, s, heads, h) ``q`` against (b, s, kv_heads, h) ``k`` / ``v``
    (grouped-query attention: query head n reads key/value head n // G, so the G query heads of a
    group are adjacent); 1 is multi-head attention."""
    H, Hk, Hv = q.shape[2], k.shape[2], v.shape[2]
    if Hk != Hv:
        raise ValueError(f"attention: k has {Hk} heads and v has {Hv}; they must have the same head count")
    if Hk < 1 or H % Hk != 0:
        raise ValueError(f"attention: {H} query heads are not a multiple of {Hk} key/value heads")
    return H // Hk


def expand_kv(t: torch.Tensor, G: int) -> torch.Tensor:
    """(b, s, kv_heads, h) with every head repeated G times in place (``repeat_interleave`` on the head
    dim); ``t`` itself for G == 1."""
    if G == 1:
        return t
    b, s, n, h = t.shape
    return t.unsqueeze(3).expand(b, s, n, G, h).reshape(b, s, n * G, h)


def _group_sum(t: torch.Tensor, G: int) -> torch.Tensor:
    """f32 (b, s, heads, h) per-query-head gradients summed over each group of G adjacent heads."""
    if G == 1:
        return t
    b, s, n, h = t.shape
    return t.reshape(b, s, n // G, G, h).sum(3)


def attention_reference(q, k, v, scale: float, causal: bool = False, q_offset: int = 0) -> torch.Tensor:
    """Plain torch oracle of ``case6_attention.py:120-133`` on (b, s, n, h) tensors; k / v may have
    fewer heads than q (:func:`kv_groups`)."""
    G = kv_groups(q, k, v)
    k, v = expand_kv(k, G), expand_kv(v, G)
    qf, kf = q.float(), k.float()
    s = torch.einsum("btnh,bfnh->bnft", kf, qf) * scale
    if causal:
        sq, sk = q.shape[1], k.shape[1]
        qi = torch.arange(sq, device=q.device)[:, None] + q_offset
        ki = torch.arange(sk, device=q.device)[None, :]
        s = s.masked_fill(ki > qi, float("-inf"))
    p = torch.softmax(s, dim=-1).to(v.dtype)
    o = torch.einsum("bnft,btnh->bfnh", p.float(), v.float())
    return o.to(v.dtype)


_WARNED_DH = set()


def _hip_attn(q, k, v) -> bool:
    """Whether the HIP attention kernels take these (b, s, heads, head_dim) operands: GPU tensors
    with head_dim 64 (the reference's, ``case6_attention.py``) contiguous in the last dim.  Other
    head dims run the torch formulation below on the GPU (same math, autograd through torch),
    with a one-time warning."""
    if not use_hip(q):
        return False
    kv_groups(q, k, v)   # (raises on unequal K / V head counts or heads that do not divide)
    if all(t.shape[-1] == 64 and t.stride(-1) == 1 for t in (q, k, v)):
        return True
    key = (q.shape[-1], v.shape[-1])
    if key not in _WARNED_DH:
        _WARNED_DH.add(key)
        import warnings
        warnings.warn(f"HIP attention kernels take head_dim 64; head_dim {q.shape[-1]} (v {v.shape[-1]}) runs "
                      "the torch attention formulation on the GPU")
    return False


def attention(q, k, v, scale: float, causal: bool = False, q_offset: int = 0) -> torch.Tensor:
    if _hip_attn(q, k, v):
        return _hip().attention(q, k, v, scale, causal, q_offset)
    return attention_reference(q, k, v, scale, causal, q_offset)


_LOG2E = 1.4426950408889634


def _block_scores(q, k, scale, causal, q_offset):
    s = torch.einsum("bqhd,bkhd->bhqk", q.float(), k.float()) * scale
    if causal:
        Sq, Sk = q.shape[1], k.shape[1]
        qi = torch.arange(Sq, device=q.device)[:, None] + q_offset
        ki = torch.arange(Sk, device=q.device)[None, :]
        s = s.masked_fill(ki > qi, float("-inf"))
    return s


def attention_fwd_lse(q, k, v, scale: float, causal: bool = False, q_offset: int = 0):
    """One (q block, kv block) flash forward: (o normalised within the block, lse) with lse in
    the HIP kernels' convention - log2 of the scaled-score partition function, +inf for rows
    without any unmasked key."""
    if _hip_attn(q, k, v):
        return _hip().attn_fwd_lse(q, k, v, scale, causal, q_offset)
    G = kv_groups(q, k, v)
    k, v = expand_kv(k, G), expand_kv(v, G)
    s = _block_scores(q, k, scale, causal, q_offset)
    m = s.amax(-1, keepdim=True)
    empty = torch.isinf(m) & (m < 0)
    m = torch.where(empty, torch.zeros_like(m), m)
    p = torch.exp(s - m)
    l = p.sum(-1, keepdim=True)
    probs = (p / l.clamp(min=1e-30)).to(v.dtype).float()
    o = torch.einsum("bhqk,bkhd->bqhd", probs, v.float()).to(v.dtype)
    lse = ((m + torch.log(l)) * _LOG2E).squeeze(-1)
    lse = torch.where(empty.squeeze(-1), torch.full_like(lse, float("inf")), lse)
    return o, lse


def attention_fwd_merge(q, k, v, scale: float, causal: bool, q_offset: int, state, last: bool):
    """One key block of a blockwise forward merged into ``state`` = [o_acc f32, lse] (None before the
    first block).  On GPU the merge happens in the kernel's epilogue; ``last`` makes it write and
    return the final output in v's dtype (else returns None)."""
    if _hip_attn(q, k, v):
        B, Sq, H, D = q.shape
        if state[0] is None:
            state[0] = torch.empty((B, Sq, H, D), dtype=torch.float32, device=q.device)
            state[1] = torch.empty((B, H, Sq), dtype=torch.float32, device=q.device)
            mode = 1
        else:
            mode = 3 if last else 2
        if mode == 1 and last:
            # a single block: the plain forward (bf16 out + lse)
            o, lse = _hip().attn_fwd_lse(q, k, v, scale, causal, q_offset)
            state[1] = lse
            return o
        out = _hip().attn_fwd_acc(q, k, v, scale, causal, q_offset, state[0], state[1], mode)
        return out if last else None
    o_s, l_s = attention_fwd_lse(q, k, v, scale, causal, q_offset)
    if state[0] is None:
        state[0], state[1] = o_s.float(), l_s
    else:
        state[0], state[1] = _merge_lse(state[0], state[1], o_s, l_s)
    return state[0].to(v.dtype) if last else None


def _merge_lse(o, lse, o_s, lse_s):
    """Merge two partial attention results (o normalised per part, lse in log2; +inf = no keys)."""
    neg = torch.full_like(lse, float("-inf"))
    a = torch.where(torch.isinf(lse) & (lse > 0), neg, lse)
    b = torch.where(torch.isinf(lse_s) & (lse_s > 0), neg, lse_s)
    m = torch.maximum(a, b)
    m0 = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    wa, wb = torch.exp2(a - m0), torch.exp2(b - m0)
    tot = wa + wb
    lse_new = torch.where(tot > 0, m0 + torch.log2(tot), torch.full_like(m, float("inf")))
    inv = torch.where(tot > 0, 1.0 / tot, torch.zeros_like(tot))
    ca = (wa * inv).permute(0, 2, 1)[..., None]
    cb = (wb * inv).permute(0, 2, 1)[..., None]
    return o.float() * ca + o_s.float() * cb, lse_new


def attention_bwd_block(q, k, v, o, do, lse, scale: float, causal: bool = False, q_offset: int = 0):
    """One kv block's (dq, dk, dv) given the final output ``o`` and global (log2) ``lse``."""
    if _hip_attn(q, k, v):
        return _hip().attn_bwd_block(q, k, v, o, do, lse, scale, causal, q_offset)
    G = kv_groups(q, k, v)
    kd, vd = k.dtype, v.dtype
    k, v = expand_kv(k, G), expand_kv(v, G)
    s = _block_scores(q, k, scale, causal, q_offset)
    p = torch.exp(s - (lse / _LOG2E)[..., None])
    dof = do.float()
    dp = torch.einsum("bqhd,bkhd->bhqk", dof, v.float())
    delta = (dof * o.float()).sum(-1).permute(0, 2, 1)[..., None]       # [b,h,q,1]
    ds = p * (dp - delta)
    dq = torch.einsum("bhqk,bkhd->bqhd", ds, k.float()) * scale
    dk = _group_sum(torch.einsum("bhqk,bqhd->bkhd", ds, q.float()) * scale, G)
    dv = _group_sum(torch.einsum("bhqk,bqhd->bkhd", p.to(v.dtype).float(), dof), G)
    return dq.to(q.dtype), dk.to(kd), dv.to(vd)


# ----------------------------------------------------------------------------- KV cache / decode
# The cache append and single-query attention over a cache (csrc/kernels/decode.hip).  ``lens`` is an
# int32 [B] tensor ON THE DEVICE: nothing below reads it on the host, so a captured step stays valid
# while the sequences grow.  Neither function takes a gradient (decoding runs under no_grad).
def fused_decode_enabled() -> bool:
    # LJS_FUSED_DECODE=0: the cache append and the decode attention on GPU shards as the torch
    # formulations below instead of the HIP kernels of csrc/kernels/decode.hip (A/B timing; escape hatch)
    return os.environ.get("LJS_FUSED_DECODE", "1") != "0"


def _append_rows(k, cap: int, lens, q, theta):
    """What both cache appends share: ``(k', q_out, rows, inside)`` -- k rotated at ``p = base[b] + t`` (as it is
    without ``theta``), the rotated q (zeros where ``p`` is outside, None without a q), the clamped rows ``p`` and
    whether ``p`` lies in ``[0, cap)``, both (B, T)."""
    B, T, _, D = k.shape
    t_idx = torch.arange(T, device=k.device)
    base = lens.long() if lens is not None else torch.zeros(B, dtype=torch.long, device=k.device)
    p = base[:, None] + t_idx[None, :]                        # (B, T)
    inside = (p >= 0) & (p < cap)
    rows = p.clamp(0, cap - 1)
    q_out = None
    if theta is not None:
        cos, sin = rope_table(k.device, D, theta, cap)
        cos, sin = cos[rows].unsqueeze(2), sin[rows].unsqueeze(2)   # (B, T, 1, D / 2)
        k = _rope_one(k, cos, sin, k.dtype)
        if q is not None:
            q_out = _rope_one(q, cos, sin, q.dtype)
            q_out = torch.where(inside[:, :, None, None], q_out, torch.zeros_like(q_out))
    elif q is not None:
        raise ValueError("kv_append: a q is rotated only with a theta")
    return k, q_out, rows, inside


def _scatter_rows(pairs, rows, inside):
    """``dst[b, rows[b, t]] = src[b, t]`` where ``inside[b, t]``, for every ``(src, dst)`` of ``pairs``."""
    ar = torch.arange(rows.shape[0], device=rows.device)
    keep = inside[:, :, None, None]
    for t in range(rows.shape[1]):                            # one row per sequence at a time: no duplicates
        r = rows[:, t]
        for src, dst in pairs:
            dst[ar, r] = torch.where(keep[:, t], src[:, t].to(dst.dtype), dst[ar, r])


def kv_append_reference(k, v, kc, vc, lens=None, q=None, theta: Optional[float] = None):
    """Plain torch cache append, in place: ``vc[b, p] = v[b, t]``, ``kc[b, p] = k'[b, t]`` for ``p = base[b] + t``
    with ``base = lens`` (int [B]) or 0 without it, rows with ``p >= cap`` dropped.  With ``theta``, ``k'`` is k
    rotated at position ``p`` exactly as :func:`rope_reference` does (same table, same f32 arithmetic),
    and a ``q`` is rotated the same way into the returned tensor (zeros where ``p >= cap``); without,
    ``k' = k``.  No host read of ``lens``."""
    k, q_out, rows, inside = _append_rows(k, kc.shape[1], lens, q, theta)
    _scatter_rows([(k, kc), (v, vc)], rows, inside)
    return q_out


def attn_decode_reference(q, kc, vc, lens, scale: float, extra: int = 1):
    """Plain torch single-query attention over a cache: q (B, 1, H, D) against rows ``[0, n_b)`` of kc / vc
    (B, cap, Hkv, D), ``n_b = min(lens[b] + extra, cap)``; query head h reads key/value head h // G.  Returns
    ``(o`` (B, 1, H, D) in vc's dtype, ``lse2`` f32 (B, H, 1)``)`` in the kernels' convention (log2 of the
    partition function of the scaled scores); ``n_b = 0`` gives ``o = 0``, ``lse2 = +inf``.  Rows at and beyond
    ``n_b`` are selected away before any arithmetic, so whatever they hold (NaN, Inf) has no influence.
    The recipe of :func:`attention_fwd_lse`: f32 scores, probabilities rounded to v's dtype before P.V."""
    G = kv_groups(q, kc, vc)
    cap = kc.shape[1]
    n = (lens.long() + int(extra)).clamp(0, cap)              # (B,)
    live = torch.arange(cap, device=q.device)[None, :] < n[:, None]      # (B, cap)
    sel = live[:, :, None, None]
    k = expand_kv(torch.where(sel, kc, torch.zeros_like(kc)), G)
    v = expand_kv(torch.where(sel, vc, torch.zeros_like(vc)), G)
    s = torch.einsum("bqhd,bkhd->bhqk", q.float(), k.float()) * scale
    s = s.masked_fill(~live[:, None, None, :], float("-inf"))
    m = s.amax(-1, keepdim=True)
    empty = torch.isinf(m) & (m < 0)
    m = torch.where(empty, torch.zeros_like(m), m)
    p = torch.exp(s - m)
    l = p.sum(-1, keepdim=True)
    probs = (p / l.clamp(min=1e-30)).to(v.dtype).float()
    o = torch.einsum("bhqk,bkhd->bqhd", probs, v.float()).to(v.dtype)
    lse = (m + torch.log(l)) * _LOG2E
    lse = torch.where(empty, torch.full_like(lse, float("inf")), lse)
    return o, lse.squeeze(-1)


_WARNED_DECODE = set()


def _hip_decode(what: str, ts, lens, G: int = 1) -> bool:
    """Whether decode.hip takes these shards: bf16 ``(B, S, H, 64)`` GPU tensors with 16-byte aligned bases
    and strides, an int32 lens and at most 16 query heads per key/value head.  Anything else on a GPU
    runs the torch formulation there, with a one-time warning per reason; host devices and
    ``LJS_FUSED_DECODE=0`` run it silently."""
    if not use_hip(ts[0]) or not fused_decode_enabled():
        return False
    hip = _hip()
    ok = hip.decode_supported(*ts) and (lens is None or lens.dtype == torch.int32) and G <= hip.decode_max_group()
    if not ok:
        key = (what, ts[0].dtype, ts[0].shape[-1], G > hip.decode_max_group())
        if key not in _WARNED_DECODE:
            _WARNED_DECODE.add(key)
            import warnings
            warnings.warn(f"HIP {what} kernel takes bf16 (B, S, H, 64) shards with 16-byte aligned bases and strides, "
                          f"an int32 lens and heads / kv_heads <= {hip.decode_max_group()}; {ts[0].dtype} "
                          f"{tuple(ts[0].shape)} strides {ts[0].stride()} with heads / kv_heads = {G} runs the torch "
                          "formulation on the GPU")
    return ok


def kv_append(k, v, kc, vc, lens=None, q=None, theta: Optional[float] = None):
    """Append one device's new ``k`` / ``v`` (B, T, Hkv, D) to its caches ``kc`` / ``vc`` (B, cap, Hkv, D) in place
    (:func:`kv_append_reference`'s semantics); returns the rotated ``q`` (or None).  One HIP launch on a GPU."""
    ts = [k, v, kc, vc] + ([q] if q is not None else [])
    if _hip_decode("kv_append", ts, lens):
        return _hip().kv_append(k, v, kc, vc, lens, q, theta)
    return kv_append_reference(k, v, kc, vc, lens, q, theta)


def attn_decode(q, kc, vc, lens, scale: float, extra: int = 1):
    """Single-query attention of one device's ``q`` (B, 1, H, D) over its caches: ``(o, lse2)``
    (:func:`attn_decode_reference`'s semantics).  One HIP launch, and a small merge launch when the
    key axis is split, on a GPU."""
    G = kv_groups(q, kc, vc)
    if _hip_decode("attn_decode", [q, kc, vc], lens, G):
        return _hip().attn_decode(q, kc, vc, lens, scale, extra)
    return attn_decode_reference(q, kc, vc, lens, scale, extra)


# ---- the MX-fp8 cache.  A quantised layer holds e4m3 bytes ``kc`` / ``vc`` (uint8 (B, cap, Hkv, D)) and e8m0
# scale bytes ``kcs`` / ``vcs`` (uint8 (B, cap, Hkv, D / 32), exponent + 127: what ``ljs_quant_mx_rows`` writes), one
# scale per 32 elements of a head row.  The two functions below state the semantics once.
def _mx_bytes(x: torch.Tensor):
    """``fp8.quantize_mx_ref`` of rows ``x[..., D]`` as stored: (e4m3 bytes, e8m0 bytes), both uint8."""
    from .fp8 import quantize_mx_ref
    qv, ex = quantize_mx_ref(x)
    return qv.view(torch.uint8), (ex + 127).to(torch.uint8)


def mx_cache_dequant(c: torch.Tensor, cs: torch.Tensor, dtype=torch.bfloat16) -> torch.Tensor:
    """``fp8.dequantize_mx_ref`` of a stored cache buffer, in ``dtype`` (exact in bf16 for blocks of normal
    magnitude: 4 significant bits times a power of two)."""
    from .fp8 import dequantize_mx_ref
    return dequantize_mx_ref(c.view(torch.float8_e4m3fn), cs.to(torch.int32) - 127).to(dtype)


def kv_append_q8_reference(k, v, kc, vc, kcs, vcs, lens=None, q=None, theta: Optional[float] = None):
    """Plain torch append into an MX-fp8 cache, in place: for every appended row, the bytes and scale bytes
    stored at ``p`` are ``fp8.quantize_mx_ref`` of the row :func:`kv_append_reference` would have stored there (k
    rotated at ``p`` and rounded to its dtype first, v as it is); rows with ``p`` outside ``[0, cap)`` write
    neither bytes nor scales.  Returns the rotated ``q`` exactly as :func:`kv_append_reference` does."""
    k, q_out, rows, inside = _append_rows(k, kc.shape[1], lens, q, theta)
    kq, ke = _mx_bytes(k)
    vq, ve = _mx_bytes(v)
    _scatter_rows([(kq, kc), (ke, kcs), (vq, vc), (ve, vcs)], rows, inside)
    return q_out


def attn_decode_q8_reference(q, kc, vc, kcs, vcs, lens, scale: float, extra: int = 1):
    """Plain torch single-query attention over an MX-fp8 cache: :func:`attn_decode_reference` on the dequantised
    cache in q's dtype.  Dead rows (at and beyond ``n_b``) are selected away BEFORE the dequantisation, so
    whatever their bytes and scale bytes hold (0x7F / 0xFF: the e4m3 and e8m0 NaNs) has no influence."""
    cap = kc.shape[1]
    n = (lens.long() + int(extra)).clamp(0, cap)
    sel = (torch.arange(cap, device=q.device)[None, :] < n[:, None])[:, :, None, None]
    z = lambda t: torch.where(sel, t, torch.zeros_like(t))   # noqa: E731
    return attn_decode_reference(q, mx_cache_dequant(z(kc), z(kcs), q.dtype), mx_cache_dequant(z(vc), z(vcs), q.dtype),
                                 lens, scale, extra)


def _hip_decode_q8(what: str, ts, cache, lens, G: int = 1) -> bool:
    """:func:`_hip_decode` for an MX-fp8 cache ``(kc, vc, kcs, vcs)``: bf16 ``(B, S, H, 64)`` ``ts`` next to uint8
    buffers decode.hip takes.  The same rule: anything else on a GPU runs the torch formulation there with a
    one-time warning per reason; host devices and ``LJS_FUSED_DECODE=0`` run it silently."""
    if not use_hip(ts[0]) or not fused_decode_enabled():
        return False
    hip = _hip()
    kc, vc, kcs, vcs = cache
    ok = hip.decode_supported(*ts) and hip.decode_q8_supported(kc, vc) and hip.decode_scale_supported(kcs, vcs) \
        and (lens is None or lens.dtype == torch.int32) and G <= hip.decode_max_group()
    if not ok:
        key = (what, ts[0].dtype, ts[0].shape[-1], G > hip.decode_max_group())
        if key not in _WARNED_DECODE:
            _WARNED_DECODE.add(key)
            import warnings
            warnings.warn(f"HIP {what} kernel takes bf16 (B, S, H, 64) shards and uint8 (B, cap, Hkv, 64) / (B, cap, Hkv, 2) "
                          f"cache buffers with 16-byte aligned bases and strides (even ones for the scales), an int32 lens "
                          f"and heads / kv_heads <= {hip.decode_max_group()}; {ts[0].dtype} {tuple(ts[0].shape)} strides "
                          f"{ts[0].stride()}, cache strides {kc.stride()} / {kcs.stride()} with heads / kv_heads = {G} "
                          "runs the torch formulation on the GPU")
    return ok


def kv_append_q8(k, v, kc, vc, kcs, vcs, lens=None, q=None, theta: Optional[float] = None):
    """Append one device's new ``k`` / ``v`` to its MX-fp8 caches in place (:func:`kv_append_q8_reference`'s
    semantics); returns the rotated ``q`` (or None).  One HIP launch on a GPU."""
    ts = [k, v] + ([q] if q is not None else [])
    if _hip_decode_q8("kv_append_q8", ts, (kc, vc, kcs, vcs), lens):
        return _hip().kv_append_q8(k, v, kc, vc, kcs, vcs, lens, q, theta)
    return kv_append_q8_reference(k, v, kc, vc, kcs, vcs, lens, q, theta)


def attn_decode_q8(q, kc, vc, kcs, vcs, lens, scale: float, extra: int = 1):
    """Single-query attention of one device's ``q`` over its MX-fp8 caches: ``(o, lse2)``
    (:func:`attn_decode_q8_reference`'s semantics).  The launches of :func:`attn_decode`, in their ``mx8`` instances."""
    G = kv_groups(q, kc, vc)
    if _hip_decode_q8("attn_decode_q8", [q], (kc, vc, kcs, vcs), lens, G):
        return _hip().attn_decode_q8(q, kc, vc, kcs, vcs, lens, scale, extra)
    return attn_decode_q8_reference(q, kc, vc, kcs, vcs, lens, scale, extra)


def lens_add(lens: torch.Tensor, n: int = 1) -> torch.Tensor:
    """``lens += n`` in place: one small HIP launch on a GPU, torch's ``add_`` elsewhere."""
    if use_hip(lens) and fused_decode_enabled() and lens.dtype == torch.int32 and lens.is_contiguous():
        return _hip().lens_add(lens, n)
    return lens.add_(n)


def lens_add_delta(lens: torch.Tensor, delta: torch.Tensor) -> torch.Tensor:
    """``lens[b] += delta[b]`` in place, ``delta`` an int32 ``(batch,)`` tensor on ``lens``' device (it may be negative:
    rows beyond the new length are dead and overwritten later).  No host read, so it can be captured."""
    if delta.dtype != torch.int32 or delta.shape != lens.shape or delta.device != lens.device:
        raise ValueError(f"lens_add_delta: delta must be an int32 {tuple(lens.shape)} tensor on {lens.device}, got "
                         f"{delta.dtype} {tuple(delta.shape)} on {delta.device}")
    return lens.add_(delta)


# ---- several new positions per sequence (csrc/kernels/decode.hip, attn_extend).  After an append of T positions at
# rows lens[b] .. lens[b] + T - 1 that lens does not count yet, position t attends to rows [0, lens[b] + t + 1): by
# definition the T stacked single-query results, which is what makes greedy speculative decoding exact.
EXTEND_MAX_POSITIONS = 64


def _stack_decode(fn, q, lens):
    outs = [fn(q[:, t:t + 1], t + 1) for t in range(q.shape[1])]
    return torch.cat([o for o, _ in outs], dim=1), torch.cat([l for _, l in outs], dim=-1)


def attn_extend_reference(q, kc, vc, lens, scale: float):
    """Plain torch attention of q (B, T, H, D) over a cache: position t is :func:`attn_decode_reference` of ``q[:, t]``
    with ``extra = t + 1``.  ``(o`` (B, T, H, D), ``lse2`` f32 (B, H, T)``)``."""
    return _stack_decode(lambda qt, e: attn_decode_reference(qt, kc, vc, lens, scale, extra=e), q, lens)


def attn_extend_q8_reference(q, kc, vc, kcs, vcs, lens, scale: float):
    """:func:`attn_extend_reference` over an MX-fp8 cache: the stacked :func:`attn_decode_q8_reference` results."""
    return _stack_decode(lambda qt, e: attn_decode_q8_reference(qt, kc, vc, kcs, vcs, lens, scale, extra=e), q, lens)


def attn_extend(q, kc, vc, lens, scale: float):
    """Attention of one device's ``q`` (B, T, H, D) over its caches, a key limit per position: ``(o, lse2)``
    (:func:`attn_extend_reference`'s semantics).  One HIP launch (and the merge launch of a split key axis) on a
    GPU; ``T == 1`` is :func:`attn_decode`'s."""
    G = kv_groups(q, kc, vc)
    if _hip_decode("attn_extend", [q, kc, vc], lens, G):
        return _hip().attn_extend(q, kc, vc, lens, scale)
    return attn_extend_reference(q, kc, vc, lens, scale)


def attn_extend_q8(q, kc, vc, kcs, vcs, lens, scale: float):
    """:func:`attn_extend` over one device's MX-fp8 caches (:func:`attn_extend_q8_reference`'s semantics)."""
    G = kv_groups(q, kc, vc)
    if _hip_decode_q8("attn_extend_q8", [q], (kc, vc, kcs, vcs), lens, G):
        return _hip().attn_extend_q8(q, kc, vc, kcs, vcs, lens, scale)
    return attn_extend_q8_reference(q, kc, vc, kcs, vcs, lens, scale)


# ----------------------------------------------------------------------------- sampling
# One token per row of logits: temperature, top-k, top-p, the Gumbel-max draw and the stop-token rule.
# ``at``, ``pos`` and ``done`` are tensors ON THE DEVICE: nothing below reads them on the host, so a captured
# decode step replays and still advances its random stream.
SAMPLE_STREAM = 0x5A3D      # Philox counter word 3 of a sampling draw
SAMPLE_MAX_EOS = 8
_PHILOX_M0, _PHILOX_M1, _PHILOX_W0, _PHILOX_W1, _MASK32 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF


def _philox_torch(c0, c1, c2, c3, k0: int, k1: int):
    """Philox4x32-10 on int64 tensors holding 32-bit words (``random._philox_np``'s stream).  A product of two
    32-bit words wraps in int64, which keeps all 64 of its bits."""
    for _ in range(10):
        p0, p1 = c0 * _PHILOX_M0, c2 * _PHILOX_M1
        hi0, lo0, hi1, lo1 = (p0 >> 32) & _MASK32, p0 & _MASK32, (p1 >> 32) & _MASK32, p1 & _MASK32
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + _PHILOX_W0) & _MASK32, (k1 + _PHILOX_W1) & _MASK32
    return c0, c1, c2, c3


def sample_params(V: int, key, temperature, top_k, top_p, eos=(), pad=0, done=True, what: str = "sample"):
    """The host-side checks of a sampling request (``ValueError`` before any launch) and its normal form:
    ``(top_k or None, top_p or None, eos tuple)`` with ``top_k >= V`` and ``top_p == 1`` turned into None."""
    if not float(temperature) > 0.0:
        raise ValueError(f"{what}: temperature must be > 0, got {temperature}")
    if top_k is not None and int(top_k) < 1:
        raise ValueError(f"{what}: top_k must be >= 1, got {top_k}")
    if top_p is not None and not 0.0 < float(top_p) <= 1.0:
        raise ValueError(f"{what}: top_p must be in (0, 1], got {top_p}")
    if key is None and (top_k is not None or top_p is not None):
        raise ValueError(f"{what}: top_k / top_p filter a random draw and need a key (without one the token is the "
                         "argmax)")
    eos = (int(eos),) if isinstance(eos, int) else tuple(int(e) for e in eos)
    if len(eos) > SAMPLE_MAX_EOS:
        raise ValueError(f"{what}: at most {SAMPLE_MAX_EOS} eos ids, got {len(eos)}")
    for name, ids in (("eos", eos), ("pad", (int(pad),) if done else ())):
        if any(i < 0 or i >= V for i in ids):
            raise ValueError(f"{what}: {name} ids {ids} must lie in the vocabulary [0, {V})")
    top_k = None if top_k is None or int(top_k) >= V else int(top_k)
    top_p = None if top_p is None or float(top_p) >= 1.0 else float(top_p)
    return top_k, top_p, eos


def _sample_rows(logits: torch.Tensor, at: Optional[torch.Tensor]) -> torch.Tensor:
    """The ``[B, V]`` rows to sample of ``[B, V]`` or ``[B, T, V]`` logits: position ``at[b]`` (clamped), default the last."""
    if logits.dim() == 2:
        return logits
    if at is None:
        return logits[:, -1]
    idx = at.long().clamp(0, logits.shape[1] - 1)
    return logits[torch.arange(logits.shape[0], device=logits.device), idx]


def sample_reference(logits, token_out, key=None, at=None, pos=None, batch_offset: int = 0, temperature: float = 1.0,
                     top_k=None, top_p=None, done=None, eos=(), pad: int = 0, stats: bool = False):
    """Plain torch sampling of one token per sequence: the contract a fused kernel will be held to.

    ``logits``: ``[B, V]`` or ``[B, T, V]`` (f32 / bf16 / any float); the row of sequence b is position ``at[b]`` (an int
    ``[B]`` tensor, clamped; default: the last).  ``token_out``: an int tensor of B elements, written in place and
    returned.  For one row ``x[0..V)``, with ``z_i = f32(x_i) * f32(1 / temperature)``:

    * ``top_k``: ``K = {i : x_i >= v_k}``, ``v_k`` the k-th largest value with multiplicity (ties at the threshold
      are all kept); ``top_k >= V`` or None: every index.
    * ``top_p`` (over K): ``w_i = exp(z_i - max_K z)`` in f32, ``S = sum_K w``; keep ``i`` iff ``sum {w_j : j in K,
      x_j > x_i} < p S`` (sums in f64).  The maximum's tie group is always kept; ``top_p = 1`` or None: no filter.
    * Both filters amount to a threshold ``tau`` on the raw x (the smallest kept value; ``-inf`` without a filter).
    * ``key`` (a ``random.Key``): ``token = argmax over {x >= tau} of z_i + g_i``, the lowest index on an exact tie, with
      ``g_i = -log(-log(u_i))`` in f64, ``u_i = ((word >> 8) + 0.5) 2^-24`` (``random._u01``), ``word`` = output ``i & 3`` of
      Philox4x32-10 at counter ``(i >> 2, lo, hi, 0x5A3D)``; ``hi = batch_offset + b``, ``lo = pos[b]`` (an int ``[B]``
      tensor; 0 without it), ``i`` the vocabulary index.  An entry of ``-inf`` is never drawn while a finite one
      exists.  Without a key: the lowest index of the row maximum, no filters, no random numbers.
    * ``done`` (int32 ``[B]``, updated in place): a sequence with ``done[b]`` writes ``pad``; otherwise the drawn
      token is written and ``done[b] = 1`` if it is one of ``eos``.

    ``stats=True`` also returns ``kept`` (int32 ``[B]``: ``|{x >= tau}|``) and ``tau`` (f32 ``[B]``).  No host read of a
    device tensor."""
    x = _sample_rows(logits, at)
    B, V = x.shape
    dev = x.device
    top_k, top_p, eos = sample_params(V, key, temperature, top_k, top_p, eos, pad, done is not None)
    if key is None:
        # the lowest index of the maximum (argmax's tie rule is not specified)
        idx = torch.arange(V, device=dev).expand(B, V)
        tok = torch.where(x == x.amax(-1, keepdim=True), idx, V).amin(-1).clamp(max=V - 1)
        kept = torch.full((B,), V, dtype=torch.int32, device=dev)
        tau = torch.full((B,), float("-inf"), dtype=torch.float32, device=dev)
    else:
        # f32(1 / T) as a host number: a tensor made from it on the device would be a copy a capture cannot record
        z = x.float() * float(torch.tensor(1.0 / float(temperature), dtype=torch.float32))
        tau = torch.full((B, 1), float("-inf"), dtype=x.dtype, device=dev)
        if top_k is not None:
            tau = x.topk(top_k, dim=-1).values[:, -1:]
        if top_p is not None:
            inK = x >= tau
            xs, order = torch.where(inK, x, float("-inf")).sort(dim=-1, descending=True, stable=True)
            zs = z.gather(-1, order)
            ins = inK.gather(-1, order)
            w = torch.where(ins, torch.exp(zs - zs[:, :1]), torch.zeros_like(zs)).double()
            cs = w.cumsum(-1)
            pos_i = torch.arange(V, device=dev).expand(B, V)
            new = torch.ones_like(ins)
            new[:, 1:] = xs[:, 1:] != xs[:, :-1]
            first = torch.where(new, pos_i, 0).cummax(-1).values          # start of each tie group
            above = torch.where(first > 0, cs.gather(-1, (first - 1).clamp(min=0)), torch.zeros_like(cs))
            keep = ins & (above < float(top_p) * cs[:, -1:])
            keep[:, 0] = True
            tau = torch.where(keep, xs, float("inf")).amin(-1, keepdim=True).to(x.dtype)
        keep = x >= tau
        i = torch.arange(V, dtype=torch.int64, device=dev).expand(B, V)
        rows = torch.arange(B, dtype=torch.int64, device=dev)
        hi = ((rows + int(batch_offset)) & _MASK32)[:, None].expand(B, V)
        lo = (pos.reshape(B).long() & _MASK32 if pos is not None else torch.zeros_like(rows))[:, None].expand(B, V)
        words = torch.stack(_philox_torch(i >> 2, lo, hi, torch.full_like(i, SAMPLE_STREAM), key.k0, key.k1), -1)
        word = words.gather(-1, (i & 3)[..., None]).squeeze(-1)
        u = ((word >> 8).double() + 0.5) * (1.0 / 16777216.0)
        score = torch.where(keep, z.double() - torch.log(-torch.log(u)), float("-inf"))
        tok = torch.where(score == score.amax(-1, keepdim=True), i, V).amin(-1).clamp(max=V - 1)
        kept = keep.sum(-1).to(torch.int32)
        tau = tau.reshape(B).float()
    if done is not None:
        was = done.reshape(B) != 0
        stop = torch.zeros_like(was)
        for e in eos:
            stop |= tok == e
        done.reshape(B).copy_(torch.where(was | stop, 1, 0).to(done.dtype))
        tok = torch.where(was, int(pad), tok)
    token_out.reshape(B).copy_(tok.to(token_out.dtype))
    return (token_out, kept, tau) if stats else token_out


def sample(logits, token_out, key=None, at=None, pos=None, batch_offset: int = 0, temperature: float = 1.0,
           top_k=None, top_p=None, done=None, eos=(), pad: int = 0, stats: bool = False):
    """Sample one token per sequence of one device's logits into ``token_out`` in place.  There is no HIP kernel
    for this yet: host devices and GPUs alike run :func:`sample_reference`, a composite of torch launches without a
    host read, which a captured decode step records and replays (like ``models.cache._greedy``, the other step of a
    decode iteration that is not a kernel of this project)."""
    return sample_reference(logits, token_out, key, at, pos, batch_offset, temperature, top_k, top_p, done, eos, pad,
                            stats)
