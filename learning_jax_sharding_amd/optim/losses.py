"""``optax.losses`` equivalents."""
from __future__ import annotations

from ..array import ShardedArray
from ..ops import core

__all__ = ["softmax_cross_entropy_with_integer_labels"]


def softmax_cross_entropy_with_integer_labels(logits: ShardedArray, labels: ShardedArray) -> ShardedArray:
    """``optax.softmax_cross_entropy_with_integer_labels``: the cross-entropy between the softmax of
    ``logits`` ``[..., num_classes]`` and the classes ``labels`` ``[...]`` (int32 or int64), an f32 array of shape
    ``[...]``: ``logsumexp(logits) - logits[label]`` per row, not reduced.

    Extension: a negative label marks an ignored row (padding), whose loss and gradient row are
    zero (torch's ``ignore_index``); optax leaves negative labels undefined.

    The class dim may be sharded (a vocab-parallel LM head): per-shard statistics are merged over
    the vocabulary axis and the result is replicated over it (:func:`..ops.core.softmax_cross_entropy`).
    On GPU shards each direction is one fused HIP kernel over the logits."""
    if not isinstance(logits, ShardedArray) or not isinstance(labels, ShardedArray):
        raise TypeError("softmax_cross_entropy_with_integer_labels takes arrays (device_put the labels)")
    return core.softmax_cross_entropy(logits, labels)
