"""The case6 multi-head self-attention block (the north-star workload).

Same parameters, logical axes and sharding constraints as
``FlaxAttention`` in ``case6_attention.py:42-143``:

* ``to_q``/``to_k``/``to_v``: Dense(inner_dim, no bias), kernel axes ``('embed','heads')``
  (``case6_attention.py:56-82``);
* ``to_out_0``: Dense(query_dim, bias), kernel axes ``('heads','embed')``
  (``case6_attention.py:83-90``);
* constraints ``('batch','embed',None)`` on q/k/v (``:105-107``), the head split
  (``:109-116``), ``('batch','kv','heads')`` after merging heads (``:137``) and
  ``('batch','embed')`` on the output (``:141``).

MI355X design: the three projections run as ONE batched MFMA GEMM over the
concatenated kernels (``fused_qkv``), and QKᵀ → scale → softmax → P·V is one
flash-style HIP kernel (``impl="fused"``).  ``impl="einsum"`` runs the
reference's literal einsum/softmax formulation (used by the parity tests).

Beyond the reference: ``causal=True`` masks key positions after the query's (both formulations), and
``rope_theta`` rotates q and k after the head split by their global positions (``ops.core.rope``:
half-split pairs, ``y[i] = x[i] cos - x[i + h] sin``, ``y[i + h] = x[i + h] cos + x[i] sin`` with ``h =
dim_head / 2`` and angle ``p theta^(-2 i / dim_head)``).  Both default to off.

Grouped-query attention: ``kv_heads < heads`` gives ``to_k`` / ``to_v`` of ``kv_heads * dim_head``
columns; with ``G = heads // kv_heads``, query head ``h`` attends to key/value head ``h // G`` (the G
query heads of a group are adjacent: HF ``repeat_kv`` / MaxText order).  ``kv_heads=1`` is multi-query
attention; ``None`` or ``heads`` is multi-head attention with the earlier parameter tree and launches.

Decoding: ``cache=(k, v, lens)`` (a layer of :class:`~.cache.KVCache`) makes the call one step of a cached
decoder and returns ``(output, cache)``.  A call on more than one position is a prefill: positions 0 ..
T-1, the usual rope and causal kernels, and K (rotated) and V written to rows 0 .. T-1 of the cache; a
call on one position appends its K / V at row ``lens[b]`` and attends to the cache (``ops.core.
cached_attention``).  With ``extend=True`` a call on ``T >= 1`` positions
(at most 64) appends them at rows ``lens[b] .. lens[b] + T - 1`` and position ``t`` attends to rows ``[0, lens[b] + t + 1)``:
the result of ``T`` single steps in one append and one attention launch.  ``lens`` is advanced by the caller, once for
all layers.  A layer of an MX-fp8 cache is
``(k, v, lens, k_scale, v_scale)``: the prefill attends to its own unquantised K / V and stores them quantised, a
decode step stores its row quantised and attends to the fp8 rows.
"""
from __future__ import annotations

import contextlib
import os
from typing import Any, Optional

import torch

from .. import dtypes as _dt
from ..array import ShardedArray
from ..nn import initializers as init
from ..nn.layers import Dense, Dropout
from ..nn.module import Module
from ..nn.partitioning import with_logical_constraint, with_logical_partitioning
from ..ops import core

__all__ = ["MultiHeadAttention", "attention_block_flops"]


class MultiHeadAttention(Module):
    query_dim: int
    heads: int = 8
    dim_head: int = 64
    dropout: float = 0.0
    dtype: Any = torch.bfloat16
    impl: str = "fused"            # "fused" (HIP flash attention) | "einsum" (reference formulation)
    fused_qkv: bool = True
    kernel_axes_in: tuple = ("embed", "heads")
    kernel_axes_out: tuple = ("heads", "embed")
    verbose: bool = False
    causal: bool = False                  # query position p attends to key positions <= p only
    rope_theta: Optional[float] = None    # rotary position embedding of q and k with this base; None: none
    kv_heads: Optional[int] = None        # key/value heads shared by groups of heads // kv_heads query heads

    def setup(self):
        if self.kv_heads is not None and (self.kv_heads < 1 or self.heads % self.kv_heads):
            raise ValueError(f"MultiHeadAttention: kv_heads={self.kv_heads} must be a positive divisor of "
                             f"heads={self.heads}")
        self.n_kv = self.heads if self.kv_heads is None else self.kv_heads
        if self.rope_theta is not None and self.dim_head % 2:
            raise ValueError(f"MultiHeadAttention: rope_theta needs an even dim_head, got {self.dim_head}")
        inner_dim = self.dim_head * self.heads
        self.scale = self.dim_head ** -0.5
        qkv_init = with_logical_partitioning(init.lecun_normal(), self.kernel_axes_in)
        self.query = Dense(inner_dim, kernel_init=qkv_init, use_bias=False, dtype=self.dtype, name="to_q")
        kv_dim = self.dim_head * self.n_kv
        self.key = Dense(kv_dim, kernel_init=qkv_init, use_bias=False, dtype=self.dtype, name="to_k")
        self.value = Dense(kv_dim, kernel_init=qkv_init, use_bias=False, dtype=self.dtype, name="to_v")
        self.proj_attn = Dense(self.query_dim,
                               kernel_init=with_logical_partitioning(init.lecun_normal(), self.kernel_axes_out),
                               dtype=self.dtype, name="to_out_0")
        self.dropout_layer = Dropout(rate=self.dropout)

    def _prefetch_out_kernel(self, x: ShardedArray, dt):
        wo = self.proj_attn.kernel_param(self.dim_head * self.heads)
        if any(t.is_meta or not t.is_cuda for t in wo.local.values()):
            return None
        axis = _fsdp_axis(wo, x)
        if axis is None:
            return None
        from ..parallel.fsdp import Prefetcher
        return Prefetcher(wo.sharding.mesh, axis, bf16_shadows=dt == torch.bfloat16).prefetch([wo])

    def _prefetch_qkv(self, x: ShardedArray, ws, dt):
        from ..sharding import NamedSharding
        w0 = ws[0]
        if dt != torch.bfloat16 or any(t.is_meta or not t.is_cuda for w in ws for t in w.local.values()):
            return None
        if not qkv_prefetch_wanted(w0):
            return None
        sh, xs = w0.sharding, x.sharding
        if not isinstance(sh, NamedSharding) or not isinstance(xs, NamedSharding) or not sh.spec:
            return None
        if any(w.sharding != sh for w in ws):
            return None
        axis = sh.spec[0]
        if not isinstance(axis, str) or sh.mesh.shape[axis] < 2 or (len(sh.spec) > 1 and sh.spec[1] is not None):
            return None
        xspec = tuple(xs.spec) + (None,) * (x.ndim - len(xs.spec))
        if xspec[-1] is not None:
            return None
        from ..parallel.fsdp import Prefetcher
        return Prefetcher(sh.mesh, axis, bf16_shadows=True).prefetch_joint(ws)

    def _log(self, *a):
        if self.verbose:
            print(*a)

    def _cached(self, x: ShardedArray, cache, residual: Optional[ShardedArray], extend: bool = False):
        """The cached call (module docstring): no gradient, dropout the identity, no ``attention_next``
        hint and no weight prefetch; the projections are the uncached call's."""
        if not self.causal:
            raise ValueError("MultiHeadAttention: a cache needs causal=True (a decoder: every position attends to "
                             "the earlier ones only)")
        if self.impl != "fused":
            raise ValueError('MultiHeadAttention: impl="einsum" has no cached path; use impl="fused"')
        lens = cache[2]
        layer = (cache[0], cache[1]) + tuple(cache[3:])      # (k, v), or (k, v, k_scale, v_scale): an MX-fp8 layer
        dt = _dt.canonicalize(self.dtype)
        with torch.no_grad():
            m = x.shape[-1]
            wq, wk, wv = self.query.kernel_param(m), self.key.kernel_param(m), self.value.kernel_param(m)
            if not self.fused_qkv:
                q, k, v = self.query(x), self.key(x), self.value(x)
            elif self.n_kv != self.heads:
                q, = core.dense(x, [wq], None, compute_dtype=dt)
                k, v = core.dense(x, [wk, wv], None, compute_dtype=dt)
            else:
                q, k, v = core.dense(x, [wq, wk, wv], None, compute_dtype=dt)
            b = x.shape[0]
            q = core.reshape(with_logical_constraint(q, ("batch", "embed", None)), (b, -1, self.heads, self.dim_head))
            k = core.reshape(with_logical_constraint(k, ("batch", "embed", None)), (b, -1, self.n_kv, self.dim_head))
            v = core.reshape(with_logical_constraint(v, ("batch", "embed", None)), (b, -1, self.n_kv, self.dim_head))
            if extend:
                hidden = core.cached_attention(q, k, v, layer, lens, self.scale, self.rope_theta, extend=True)
            elif x.shape[1] == 1:
                hidden = core.cached_attention(q, k, v, layer, lens, self.scale, self.rope_theta)
            else:
                if self.rope_theta is not None:
                    q, k = core.rope(q, k, theta=self.rope_theta)
                hidden = core.dot_product_attention(q, k, v, self.scale, causal=True)
                core.cache_prefill(k, v, layer)
            hidden = core.reshape(hidden, (b, -1, self.heads * self.dim_head))
            hidden = with_logical_constraint(hidden, ("batch", "kv", "heads"))
            hidden = self.proj_attn(hidden, residual=residual)
            return with_logical_constraint(hidden, ("batch", "embed")), cache

    def __call__(self, hidden_states: ShardedArray, context: Optional[ShardedArray] = None,
                 deterministic: bool = True, residual: Optional[ShardedArray] = None, cache=None,
                 extend: bool = False):
        """``residual`` (the block's input, for a skip connection): returns
        ``residual + attention(...)`` in the compute dtype, the add fused into the output
        projection's GEMM epilogue when dropout is the identity.  ``cache``: one layer ``(k, v, lens)`` of a
        :class:`~.cache.KVCache`; the call then returns ``(output, cache)`` (module docstring).  ``extend=True`` (with a
        cache): the ``T >= 1`` positions of the call continue the cached sequence at rows ``lens[b] .. lens[b] + T - 1``
        instead of restarting it (``ops.core.cached_attention``)."""
        if extend and cache is None:
            raise ValueError("MultiHeadAttention: extend=True needs a cache (it continues a cached sequence)")
        if cache is not None:
            if context is not None:
                raise ValueError("MultiHeadAttention: a cache with a context (cross-attention) is not implemented: "
                                 "the cache holds the keys and values of the sequence being decoded")
            return self._cached(hidden_states, cache, residual, extend)
        self_attn = context is None
        if self.rope_theta is not None and not self_attn:
            raise ValueError("MultiHeadAttention: rope_theta with a context (cross-attention) is not defined: "
                             "queries and keys would be rotated by positions of two different sequences")
        context = hidden_states if context is None else context
        self._log("context.shape: ", context.shape)
        dt = _dt.canonicalize(self.dtype)
        # FSDP rules (case5_attention_dense.py:109-112: embed -> data) shard the out projection's
        # kernel over the batch axis: gather it on a side stream NOW, while the QKV projection and
        # the attention run, instead of at its use (parallel/fsdp.py Prefetcher, bf16 shadows)
        wo_pf = self._prefetch_out_kernel(hidden_states, dt)
        gqa = self.n_kv != self.heads
        if gqa:
            # a K/V projection whose columns are split more ways than there are key/value heads would
            # split a head (or need replicated key/value heads, which is not implemented)
            n = self.key.kernel_param(context.shape[-1]).tile.tile_shape[1]
            if self.n_kv % n:
                raise ValueError(f"MultiHeadAttention: kv_heads={self.n_kv} cannot be sharded {n} ways (the shard "
                                 f"count of the K/V projection's columns); kv_heads must be a multiple of {n}")
        if self.fused_qkv and self_attn and gqa:
            # K and V have equal widths and run as one fused two-kernel GEMM; Q, wider, is a GEMM of its
            # own.  No attention_next hint: the fused projection + forward kernel is multi-head only
            m = hidden_states.shape[-1]
            query_proj, = core.dense(hidden_states, [self.query.kernel_param(m)], None, compute_dtype=dt)
            key_proj, value_proj = core.dense(hidden_states, [self.key.kernel_param(m), self.value.kernel_param(m)],
                                              None, compute_dtype=dt)
        elif self.fused_qkv and self_attn:
            m = hidden_states.shape[-1]
            wq = self.query.kernel_param(m)
            wk = self.key.kernel_param(m)
            wv = self.value.kernel_param(m)
            # Q/K/V kernels sharded over their input features (the reference's 2-D rules: embed
            # -> model) while the activation's features are whole: their one stacked bf16 gather
            # runs on a side stream, and the projection GEMM waits for it only after queueing
            # the activation's cast pass (ops/linear.defer_wait)
            qkv_pf = self._prefetch_qkv(hidden_states, [wq, wk, wv], dt)
            if qkv_pf is not None:
                from ..ops import linear as _lin
                _lin.defer_wait(qkv_pf)
                ws = qkv_pf.tree()
            else:
                ws = [wq, wk, wv]
            # the attention forward rides in the projection kernel when every device holds whole
            # sequences and all heads (ops/linear.attention_next: single device / data parallel)
            from ..ops import linear as _lin
            # (not for a causal or rotary layer: the fused projection + forward kernel is non-causal
            # and consumes the un-rotated Q / K, so its launch would be wasted and its registry
            # entry left stale)
            hint = (self.impl == "fused" and not self.causal and self.rope_theta is None
                    and qkv_pf is None and hidden_states.ndim == 3
                    and tuple(hidden_states.tile.tile_shape[1:]) == (1, 1)
                    and all(tuple(w.tile.tile_shape) == (1, 1) for w in (wq, wk, wv)))
            with (_lin.attention_next(self.heads, self.dim_head, self.scale) if hint else contextlib.nullcontext()):
                query_proj, key_proj, value_proj = core.dense(hidden_states, ws, None, compute_dtype=dt)
            if qkv_pf is not None:
                qkv_pf.wait()
        else:
            query_proj = self.query(hidden_states)
            key_proj = self.key(context)
            value_proj = self.value(context)
        self._log("query_proj.shape: ", query_proj.shape)

        # (batch, seq, heads*head_dim); the head split is metadata-only because heads is replicated
        query_proj = with_logical_constraint(query_proj, ("batch", "embed", None))
        key_proj = with_logical_constraint(key_proj, ("batch", "embed", None))
        value_proj = with_logical_constraint(value_proj, ("batch", "embed", None))

        b = hidden_states.shape[0]
        q = core.reshape(query_proj, (b, -1, self.heads, self.dim_head))
        k = core.reshape(key_proj, (b, -1, self.n_kv, self.dim_head))
        v = core.reshape(value_proj, (b, -1, self.n_kv, self.dim_head))
        q = with_logical_constraint(q, ("batch", "embed", None, None))
        k = with_logical_constraint(k, ("batch", "embed", None, None))
        v = with_logical_constraint(v, ("batch", "embed", None, None))
        self._log("query_states.shape: ", q.shape)

        if self.rope_theta is not None:
            # after the head split, before either attention formulation: q and k in one launch per device
            q, k = core.rope(q, k, theta=self.rope_theta)

        if self.impl == "fused":
            hidden = core.dot_product_attention(q, k, v, self.scale, causal=self.causal)
        else:
            if gqa:
                # every key/value head repeated for the G query heads of its group
                def per_group(t):
                    bt, st = t.shape[0], t.shape[1]
                    t = core.reshape(t, (bt, st, self.n_kv, 1, self.dim_head))
                    t = core.broadcast_to(t, (bt, st, self.n_kv, self.heads // self.n_kv, self.dim_head))
                    return core.reshape(t, (bt, st, self.heads, self.dim_head))
                k, v = per_group(k), per_group(v)
            qf = core.convert(q, torch.float32)
            kf = core.convert(k, torch.float32)
            scores = core.einsum("b t n h, b f n h -> b n f t", kf, qf)
            scores = core.binary("mul", scores, self.scale)
            if self.causal:
                # (f, t) = (query, key): -inf above the diagonal, before the softmax
                nq, nk = q.shape[1], k.shape[1]
                above = torch.arange(nk)[None, :] > torch.arange(nq)[:, None]
                mask = torch.zeros(nq, nk).masked_fill_(above, float("-inf"))
                scores = core.binary("add", scores, core.asarray_like(mask, scores))
            probs = core.softmax(scores, axis=-1)
            probs = core.convert(probs, dt)
            hidden = core.einsum("b n f t, b t n h -> b f n h", probs, v)
        hidden = core.reshape(hidden, (b, -1, self.heads * self.dim_head))
        hidden = with_logical_constraint(hidden, ("batch", "kv", "heads"))
        drop_id = deterministic or self.dropout == 0.0
        wo = wo_pf.wait()[0] if wo_pf is not None else None
        if residual is not None and drop_id:
            hidden = self.proj_attn(hidden, residual=residual, kernel=wo)
            return with_logical_constraint(hidden, ("batch", "embed"))
        hidden = self.proj_attn(hidden, kernel=wo)
        hidden = with_logical_constraint(hidden, ("batch", "embed"))
        hidden = self.dropout_layer(hidden, deterministic=deterministic)
        if residual is not None:
            hidden = core.binary("add", core.convert(residual, dt), hidden)
        return hidden


# Measured: the gather overlaps the activation cast (profiles/r3k_v2x2_prefetch_overlap.md), but
# the side-stream branch costs more than it hides when the "gather" moves no bytes between GPUs:
# 2-D rehearsal 0.3378-0.3404 vs 0.3165-0.3172 ms, 4 virtual devices 1.79-1.80 vs 1.62 ms
# (gpurun_out/r3k).  Over xGMI it is a real transfer worth hiding.  LJS_QKV_PREFETCH: "1" on,
# "0" off, "auto" (default): on exactly when the gather crosses between distinct GPUs.
_QKV_PREFETCH = os.environ.get("LJS_QKV_PREFETCH", "auto").lower()


def qkv_prefetch_wanted(w: ShardedArray) -> bool:
    """Whether the Q/K/V weight gather of ``w``'s layout is prefetched on a side stream."""
    if _QKV_PREFETCH in ("0", "1"):
        return _QKV_PREFETCH == "1"
    from ..comm.backend import get_comm
    c = get_comm()
    if c.kind == "dist":
        return c.real_transfers()
    return c.real_transfers([t.device for t in w.local.values()])


def _fsdp_axis(w: ShardedArray, x: ShardedArray):
    """The mesh axis sharding both ``w`` and ``x``'s batch dim (the FSDP pattern), else None."""
    from ..sharding import NamedSharding
    ws, xs = w.sharding, x.sharding
    if not isinstance(ws, NamedSharding) or not isinstance(xs, NamedSharding) or not xs.spec:
        return None
    b = xs.spec[0]
    b_axes = set(b) if isinstance(b, tuple) else ({b} if b else set())
    for e in ws.spec:
        for a in (e if isinstance(e, tuple) else (e,)):
            if a is not None and a in b_axes and ws.mesh.shape[a] > 1:
                return a
    return None


def attention_block_flops(batch: int, seq: int, dim: int, heads: int, dim_head: int, train: bool,
                          kv_heads: Optional[int] = None) -> float:
    """Matmul FLOPs of the case6 block: fwd 6.442 GFLOP at B=8,S=256,M=640; train 15.30.
    ``kv_heads`` (grouped-query attention) narrows the K and V projections to ``kv_heads * dim_head``
    columns; the score and P.V products are per query head and unchanged."""
    t = batch * seq
    inner = heads * dim_head
    kv_inner = (heads if kv_heads is None else kv_heads) * dim_head
    qkv = 2 * t * dim * (inner + 2 * kv_inner)
    qk = 2 * batch * heads * seq * seq * dim_head
    pv = qk
    out = 2 * t * inner * dim
    fwd = qkv + qk + pv + out
    if not train:
        return float(fwd)
    # backward: dWo + dh (2 out-proj GEMMs), attention bwd (dV, dP, dQ, dK = 4 seq^2 GEMMs), dWqkv (no dx)
    bwd = 2 * out + 4 * qk + qkv
    return float(fwd + bwd)
