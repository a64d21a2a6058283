"""A small language model from token ids to logits, through this project's kernels only: token (and
optional learned position) :class:`~..nn.layers.Embed`, a stack of pre-norm
:class:`~.transformer.TransformerLayer`, a final norm and a ``Dense(vocab_size)`` head.

``causal=True`` makes it a decoder: the logits at position p depend on the tokens at positions <= p
only, which is what :func:`lm_loss` on next-token labels needs.  With the default ``causal=False``
every position attends to the whole sequence (an encoder; next-token labels would let the model read
the tokens it is asked to predict).  Positions come from ``rope_theta`` (rotary embedding of q and k
in every layer) or from ``max_len`` (a learned additive table), not both; with neither the model sees
positions through the causal mask alone.

Decoding: :meth:`TransformerLM.init_cache` makes a :class:`~.cache.KVCache`; a call with ``cache=`` is a prefill
(more than one position) or one decode step (one position) and returns ``(logits, cache)``; with ``extend=True`` a
call on up to 64 positions continues the cache as that many decode steps would;
:func:`~.cache.generate` is greedy decoding on top of both.

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

    def init_cache(self, batch: int, max_len: int, sharding=None, quant=None):
        """A zero-filled :class:`~.cache.KVCache` for ``batch`` sequences of up to ``max_len`` positions, in the
        model's compute dtype; ``sharding``: of its ``(batch, max_len, kv_heads, dim_head)`` buffers.  On GPU
        devices the rope table grows to ``max_len`` rows here (never inside a graph capture).  ``quant="mxfp8"``:
        an MX-fp8 cache (e4m3 bytes with e8m0 scales per 32 elements, ``dim_head % 32 == 0``): a prefill attends to
        the prompt's unquantised K / V and stores them quantised; decode steps attend to the fp8 rows."""
        from .cache import KVCache
        if self.max_len is not None and max_len > self.max_len:
            raise ValueError(f"TransformerLM.init_cache: max_len {max_len} > the position table's {self.max_len} rows")
        kvh = self.heads if self.kv_heads is None else self.kv_heads
        cache = KVCache.zeros(self.layers, batch, max_len, kvh, self.dim_head, self.dtype, sharding, quant=quant)
        if self.rope_theta is not None:
            from ..ops import kernels as K
            for t in cache.lens.local.values():
                if t.is_cuda:
                    K.rope_table(t.device, self.dim_head, float(self.rope_theta), max_len)
        return cache

    def _cached(self, ids: ShardedArray, cache, prompt_lens, extend: bool = False):
        """Prefill (more than one position: restarts the cache), one decode step, or with ``extend`` a step of
        several positions that continues the cache (module docstring)."""
        for name, bad in (("causal=False", not self.causal), ("fp8=True", self.fp8)):
            if bad:
                raise ValueError(f"TransformerLM: {name} has no cached path (a cache needs a causal decoder "
                                 "without the fp8 feed-forward)")
        if len(cache) != self.layers:
            raise ValueError(f"TransformerLM: the cache has {len(cache)} layers, the model {self.layers}")
        T = ids.shape[-1]
        if extend:
            from ..ops.kernels import EXTEND_MAX_POSITIONS
            if prompt_lens is not None:
                raise ValueError("TransformerLM: extend=True continues the cache at cache.lens; prompt_lens goes with a "
                                 "prefill")
            if T > EXTEND_MAX_POSITIONS:
                raise ValueError(f"TransformerLM: extend=True takes at most {EXTEND_MAX_POSITIONS} positions per call, "
                                 f"got {T}")
        if T > cache.max_len:
            raise ValueError(f"TransformerLM: {T} positions do not fit the cache's max_len {cache.max_len}")
        if T == 1 and prompt_lens is not None:
            raise ValueError("TransformerLM: prompt_lens goes with a prefill (more than one position)")
        if prompt_lens is not None and not isinstance(prompt_lens, ShardedArray):
            import numpy as np
            from ..array import device_put
            prompt_lens = device_put(np.asarray(prompt_lens, dtype=np.int32).reshape(-1), cache.lens.sharding)
        with torch.no_grad():
            x = self.embed(ids)
            if self.max_len is not None:
                if T > self.max_len:
                    raise ValueError(f"TransformerLM: sequence length {T} > max_len {self.max_len}")
                if extend and T > 1:
                    # position lens[b] + t, on the devices
                    base = core.broadcast_to(core.reshape(cache.lens, (ids.shape[0], 1)), tuple(ids.shape))
                    pos = core.binary("add", base, core.convert(_position_ids(ids), cache.lens.dtype))
                else:
                    pos = _position_ids(ids) if T > 1 else core.reshape(cache.lens, (ids.shape[0], 1))
                x = core.binary("add", x, self.pos_embed(pos))
            x = with_logical_constraint(x, ("batch", "length", "embed"))
            for i, blk in enumerate(self.blocks):
                x, _ = blk(x, cache=cache.layer(i), extend=extend)
            if T == 1 or extend:
                core.cache_advance(cache.lens, T)       # after the last layer: one small launch
            else:
                core.cache_set_lens(cache.lens, T if prompt_lens is None else prompt_lens)
            x = self.final_norm(x)
            return with_logical_constraint(self.head(x), ("batch", "length", "vocab")), cache

    def __call__(self, ids: ShardedArray, cache=None, prompt_lens=None, extend: bool = False):
        """Token ids ``[batch, length]`` (int32 / int64) -> logits ``[batch, length, vocab_size]``.

        ``cache`` (a :class:`~.cache.KVCache` from :meth:`init_cache`): returns ``(logits, cache)``, the buffers
        updated in place, without gradient.  ``length > 1`` is a prefill that restarts the cache: positions 0
        .. length-1, K / V of every layer to rows 0 .. length-1, ``cache.lens := prompt_lens`` (an int
        ``(batch,)`` array laid out like ``cache.lens``: right-padded ragged prompts) or ``length``.  ``length == 1``
        is a decode step: the token of sequence b sits at position ``cache.lens[b]``, and ``lens += 1``.

        ``extend=True`` (with a cache, without ``prompt_lens``, ``length <= 64``): the tokens of sequence b sit at positions
        ``cache.lens[b] .. cache.lens[b] + length - 1`` and continue the cache instead of restarting it; the logits are those
        of ``length`` decode steps, in one step's launches, and ``lens += length``.  A caller that keeps fewer of the
        positions sets ``cache.lens`` back (``ops.core.cache_advance`` with a negative array): rows beyond ``lens`` are dead."""
        if extend and cache is None:
            raise ValueError("TransformerLM: extend=True needs a cache (it continues a cached sequence)")
        if cache is not None:
            return self._cached(ids, cache, prompt_lens, extend)
        if prompt_lens is not None:
            raise ValueError("TransformerLM: prompt_lens goes with a cache")
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
