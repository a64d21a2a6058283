"""Attention + feed-forward transformer layer (north-star config "attention+FF, 2D mesh, fp8").

The reference declares the FF layer in comments only (``case6_attention.py:36-40``,
``y = Relu(Win x) Wout``) and maps its ``hidden`` logical axis to ``model``
(``case6_attention.py:186``).  This layer is the case6 attention block followed
by that FF block, each with a residual connection; ``fp8=True`` runs the FF
GEMMs on CDNA4's e4m3 MFMA path.  ``norm='layer'`` / ``'rms'`` makes it a pre-norm
layer (``h = x + attn(norm1(x))``, ``y = h + ff(norm2(h))``) that can be stacked.
"""
from __future__ import annotations

from typing import Any, Optional

import torch

from ..nn.layers import FeedForward, GatedFeedForward, LayerNorm, RMSNorm
from ..nn.module import Module
from ..ops import core
from .attention import MultiHeadAttention, attention_block_flops

__all__ = ["TransformerLayer", "transformer_layer_flops"]


def check_ff_kind(owner: str, kind, fp8: bool) -> None:
    """The ``ff`` option of TransformerLayer / TransformerLM: "relu" or "swiglu", the latter without fp8."""
    if kind not in ("relu", "swiglu"):
        raise ValueError(f"{owner} ff must be 'relu' or 'swiglu', got {kind!r}")
    if kind == "swiglu" and fp8:
        raise ValueError(f"{owner}: ff='swiglu' has no fp8 path (GatedFeedForward is bf16 / f32 only); use "
                         "fp8=False or ff='relu'")


class TransformerLayer(Module):
    query_dim: int
    heads: int = 8
    dim_head: int = 64
    ff_dim: int = 2560
    dtype: Any = torch.bfloat16
    fp8: bool = False
    norm: Optional[str] = None   # None (no normalisation), "layer" or "rms": pre-norm
    causal: bool = False                  # causal self-attention (MultiHeadAttention.causal)
    rope_theta: Optional[float] = None    # rotary position embedding of q and k (MultiHeadAttention.rope_theta)
    ff: str = "relu"                      # "relu": FeedForward; "swiglu": GatedFeedForward (no fp8)
    kv_heads: Optional[int] = None        # grouped-query attention (MultiHeadAttention.kv_heads)

    def __post_init__(self):
        super().__post_init__()
        check_ff_kind("TransformerLayer", self.ff, self.fp8)

    def setup(self):
        self.attn = MultiHeadAttention(self.query_dim, self.heads, self.dim_head, dtype=self.dtype,
                                       causal=self.causal, rope_theta=self.rope_theta, kv_heads=self.kv_heads,
                                       name="attn")
        # the field `ff` names the kind; on the bound module the submodule takes its place (callers
        # reach the block as `layer.ff`, and its parameters sit under "ff" either way).  The kind is
        # kept aside so that a copy of a module that is already set up builds its block again
        kind = self.__dict__.get("_ff_kind") or self.ff
        object.__setattr__(self, "_ff_kind", kind)
        check_ff_kind("TransformerLayer", kind, self.fp8)
        if kind == "relu":
            self.ff = FeedForward(self.ff_dim, dtype=self.dtype, fp8=self.fp8, name="ff")
        else:
            self.ff = GatedFeedForward(self.ff_dim, dtype=self.dtype, name="ff")
        if self.norm is not None:
            if self.norm not in ("layer", "rms"):
                raise ValueError(f"TransformerLayer norm must be None, 'layer' or 'rms', got {self.norm!r}")
            # the norms write the compute dtype: their output is the projections' operand as it is
            cls = LayerNorm if self.norm == "layer" else RMSNorm
            self.norm1 = cls(dtype=self.dtype, name="norm1")
            self.norm2 = cls(dtype=self.dtype, name="norm2")

    def __call__(self, x, cache=None, extend: bool = False):
        """``cache``: one layer ``(k, v, lens)`` of a :class:`~.cache.KVCache`: a cached decoder step or prefill
        (``MultiHeadAttention``), without gradient; returns ``(y, cache)``.  ``extend=True``: the call's positions
        continue the cached sequence (``MultiHeadAttention``)."""
        if extend and cache is None:
            raise ValueError("TransformerLayer: extend=True needs a cache (it continues a cached sequence)")
        if cache is not None:
            if self.fp8:
                raise ValueError("TransformerLayer: fp8=True has no cached path (the fp8 feed-forward under a cache "
                                 "is not implemented); use fp8=False")
            with torch.no_grad():
                xin = self.norm1(x) if self.norm is not None else x
                h, cache = self.attn(xin, residual=x, cache=cache, extend=extend)
                return self.ff(self.norm2(h) if self.norm is not None else h, residual=h), cache
        if self.norm is not None:
            # pre-norm: the skips carry the un-normalised stream.  The attention's stays in its
            # out-projection's epilogue; the FF's residual is not its input, so it takes
            # FeedForward's general path
            h = self.attn(self.norm1(x), residual=x)
            return self.ff(self.norm2(h), residual=h)
        # h = x + attn(x); y = h + ff(h), both skip connections fused into the output GEMMs'
        # epilogues (x is read in f32 and rounded to the compute dtype there, as convert(x) would)
        h = self.attn(x, residual=x)
        return self.ff(h, residual=h)


def transformer_layer_flops(batch, seq, dim, heads, dim_head, ff_dim, train: bool, gated: bool = False,
                            kv_heads: Optional[int] = None) -> float:
    """Matmul FLOPs of one layer step (the project's convention: the memory-bound norms of a
    pre-norm layer and the activation are not counted).  ``gated``: a GatedFeedForward, three GEMMs
    (gate, up, down) where the ReLU FeedForward has two.  ``kv_heads``: attention_block_flops'."""
    att = attention_block_flops(batch, seq, dim, heads, dim_head, train, kv_heads=kv_heads)
    ff = (3 if gated else 2) * 2 * batch * seq * dim * ff_dim
    return att + (3 * ff if train else ff)
