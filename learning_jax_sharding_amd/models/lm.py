"""A small language model from token ids to logits, through this project's kernels only: token (and
optional learned position) :class:`~..nn.layers.Embed`, a stack of pre-norm
:class:`~.transformer.TransformerLayer`, a final norm and a ``Dense(vocab_size)`` head.

``causal=True`` makes it a decoder: the logits at position p depend on the tokens at positions <= p
only, which is what :func:`lm_loss` on next-token labels needs.  With the default ``causal=False``
every position attends to the whole sequence (an encoder; next-token labels would let the model read
the tokens it is asked to predict).  Positions come from ``rope_theta`` (rotary embedding of q and k
in every layer) or from ``max_len`` (a learned additive table), not both; with neither the model sees
positions through the causal mask alone.

The embedding table's logical axes are ``("vocab", "embed")`` and the head kernel's ``("embed",
"vocab")``: under ``parallel.tensor.VOCAB_PARALLEL_RULES`` both ends of the model are vocab-parallel
(the lookup all-reduces activations, the loss merges per-shard statistics; no table or logits row
is ever gathered).  There is no tied head and no ``Embed.attend``: no dense here takes a transposed
weight.
"""
from __future__ import annotations

from typing import Any, Optional

import torch

from ..array import ShardedArray
from ..nn import initializers as init
from ..nn.layers import Dense, Embed, LayerNorm, RMSNorm
from ..nn.module import Module
from ..nn.partitioning import with_logical_constraint, with_logical_partitioning
from ..ops import core
from .transformer import TransformerLayer, check_ff_kind

__all__ = ["TransformerLM", "lm_loss"]


def _position_ids(ids: ShardedArray) -> ShardedArray:
    """``arange(S)`` along the last dim of ``ids``, with ids' shape, dtype and sharding: every position
    appears once per sequence."""
    loc = {}
    for d, t in ids.local.items():
        lo, hi = ids.tile.region(d, ids.shape)[-1]
        loc[d] = torch.arange(lo, hi, dtype=t.dtype, device=t.device).expand(t.shape)
    return ShardedArray(ids.shape, ids.dtype, ids.sharding, loc)


class TransformerLM(Module):
    vocab_size: int
    dim: int
    layers: int
    heads: int = 8
    dim_head: int = 64
    ff_dim: Optional[int] = None   # None: 4 * dim ("relu"); the multiple of 128 at or above 8 * dim / 3 ("swiglu")
    max_len: Optional[int] = None  # a learned position table of this many rows; None: no positions
    norm: str = "rms"
    dtype: Any = torch.bfloat16
    fp8: bool = False
    causal: bool = False                  # causal self-attention in every layer
    rope_theta: Optional[float] = None    # rotary position embedding with this base in every layer
    ff: str = "relu"                      # "relu": FeedForward; "swiglu": GatedFeedForward (no fp8)
    kv_heads: Optional[int] = None        # grouped-query attention in every layer (MultiHeadAttention.kv_heads)

    def default_ff_dim(self) -> int:
        """``ff_dim=None``: 4 dim for the ReLU feed-forward; for the gated one, whose three matrices then
        hold what the ReLU block's two do, the smallest multiple of 128 (the GEMM tiles) >= 8 dim / 3."""
        if self.ff == "swiglu":
            return -(-8 * self.dim // (3 * 128)) * 128
        return 4 * self.dim

    def __post_init__(self):
        super().__post_init__()
        check_ff_kind("TransformerLM", self.ff, self.fp8)

    def setup(self):
        if self.norm not in ("layer", "rms"):
            raise ValueError(f"TransformerLM norm must be 'layer' or 'rms', got {self.norm!r}")
        if self.rope_theta is not None and self.max_len is not None:
            raise ValueError("TransformerLM: rope_theta and max_len are two position schemes; give one")
        self.embed = Embed(self.vocab_size, self.dim, dtype=self.dtype, name="embed")
        if self.max_len is not None:
            self.pos_embed = Embed(self.max_len, self.dim, dtype=self.dtype, name="pos_embed")
        ff = self.ff_dim if self.ff_dim is not None else self.default_ff_dim()
        self.blocks = [TransformerLayer(self.dim, heads=self.heads, dim_head=self.dim_head, ff_dim=ff,
                                        dtype=self.dtype, fp8=self.fp8, norm=self.norm, causal=self.causal,
                                        rope_theta=self.rope_theta, ff=self.ff, kv_heads=self.kv_heads,
                                        name=f"layer_{i}")
                       for i in range(self.layers)]
        cls = LayerNorm if self.norm == "layer" else RMSNorm
        self.final_norm = cls(dtype=self.dtype, name="final_norm")
        self.head = Dense(self.vocab_size, use_bias=False, dtype=self.dtype, name="head",
                          kernel_init=with_logical_partitioning(init.lecun_normal(), ("embed", "vocab")))

    def __call__(self, ids: ShardedArray) -> ShardedArray:
        """Token ids ``[batch, length]`` (int32 / int64) -> logits ``[batch, length, vocab_size]``."""
        x = self.embed(ids)
        if self.max_len is not None:
            if ids.shape[-1] > self.max_len:
                raise ValueError(f"TransformerLM: sequence length {ids.shape[-1]} > max_len {self.max_len}")
            x = core.binary("add", x, self.pos_embed(_position_ids(ids)))
        x = with_logical_constraint(x, ("batch", "length", "embed"))
        for blk in self.blocks:
            x = blk(x)
        x = self.final_norm(x)
        return with_logical_constraint(self.head(x), ("batch", "length", "vocab"))


def lm_loss(model: TransformerLM, params, ids: ShardedArray, labels: ShardedArray) -> ShardedArray:
    """Mean softmax cross-entropy of ``model``'s logits for ``ids`` against integer ``labels`` (a negative
    label marks an ignored token: loss 0, counted in the mean)."""
    from .. import optim
    logits = model.apply({"params": params}, ids)
    return optim.softmax_cross_entropy_with_integer_labels(logits, labels).mean()
