"""Global-norm gradient clipping (``optax.global_norm`` / ``optax.clip_by_global_norm``).

The norm of a tree of sharded arrays counts every distinct tile exactly once: a leaf contributes,
on device ``d``, only when ``tile.replica_index[d] == 0``, so a weight replicated over a mesh axis
is counted once and a weight sharded over an axis in every shard.  The per-device float64 partial
sums are all-gathered (one ``[1]``-element value per device; a device that owns nothing sends 0)
and added in device-id order on every device, so all devices get the same bits.  When every leaf
is replicated over the same devices (pure data parallelism: the gradients Adam reads are the
reduced buckets) each device already holds everything and there is no collective.

This module is the formula in torch on the tensors' own device, used on host devices and as the
fallback of the fused MI355X path (``chain(clip_by_global_norm(c), adam(...))``, optim/adam.py:
``grad_sumsq`` + ``step_hyper`` + the dynamic Adam instance, inside the captured step).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch

from ..array import ShardedArray
from ..utils import tree as T
from .adam import EmptyState, GradientTransformation

__all__ = ["global_norm", "clip_by_global_norm", "ClipByGlobalNorm"]


def _is_arr(x):
    return isinstance(x, ShardedArray)


def norm_plan(leaves: List[ShardedArray]) -> Tuple[Tuple[int, ...], bool]:
    """(the devices of the leaves' meshes, sorted; whether the partial sums differ by device and
    have to be gathered).  No gather: every leaf replicated over the same devices."""
    devs = sorted({d for l in leaves for d in l.tile.device_ids})
    same = all(l.tile.is_fully_replicated and tuple(l.tile.device_ids) == tuple(devs) for l in leaves)
    return tuple(devs), not same


def counted(leaf: ShardedArray, d: int, gather: bool) -> bool:
    """Whether device ``d`` counts its tile of ``leaf`` (see the module docstring)."""
    return not gather or leaf.tile.replica_index[d] == 0


def _f64_bits_as_f32(t: torch.Tensor) -> torch.Tensor:
    # a float64 [1] travels as its two 32-bit halves: every collective route moves f32
    return t.reshape(1).view(torch.float32).reshape(1, 2)


def gather_partials(partials: Dict[int, torch.Tensor], devs: Tuple[int, ...]) -> Dict[int, torch.Tensor]:
    """All-gather of one float64 ``[1]`` partial per device over ``devs``: per device the float64
    ``[len(devs)]`` vector in device-id order."""
    from ..comm import collectives as C
    out = C.all_gather({d: _f64_bits_as_f32(t) for d, t in partials.items()}, [list(devs)], 0, note="clip.norm")
    return {d: t.contiguous().view(torch.float64).reshape(-1) for d, t in out.items()}


def _sum_in_order(v: torch.Tensor) -> torch.Tensor:
    acc = v[0]
    for i in range(1, v.shape[0]):
        acc = acc + v[i]
    return acc


def _sumsq_f64(leaves: List[ShardedArray], local_of=None) -> Tuple[Dict[int, torch.Tensor], ShardedArray]:
    """Per local device the float64 0-d sum of squares of the whole tree (gathered when needed)."""
    local_of = local_of or (lambda l, d: l.local[d])
    devs, gather = norm_plan(leaves)
    mine: Dict[int, torch.device] = {}
    for l in leaves:
        for d in l.local:
            mine.setdefault(d, l.local[d].device)
    part = {}
    for d, dev in mine.items():
        acc = torch.zeros((), dtype=torch.float64, device=dev)
        for l in leaves:
            if d in l.local and counted(l, d, gather):
                acc = acc + torch.sum(local_of(l, d).to(torch.float64) ** 2)
        part[d] = acc
    if gather and len(devs) > 1:
        part = {d: _sum_in_order(v) for d, v in gather_partials(part, devs).items()}
    return part, leaves[0]


def _replicated_scalar(like: ShardedArray, devs, loc: Dict[int, torch.Tensor], dtype=torch.float32) -> ShardedArray:
    from ..sharding.shardings import GSPMDSharding
    from ..sharding.tile import TileAssignment
    sh = GSPMDSharding(tuple(like.sharding._device_assignment), TileAssignment.replicated(devs, 0))
    return ShardedArray((), dtype, sh, loc)


def global_norm(tree) -> ShardedArray:
    """sqrt(sum over the leaves of sum(x ** 2)): an f32 scalar, replicated, the same bits on every
    device.  Accumulated in float64 and rounded once."""
    leaves = [l for l in T.tree_leaves(tree, is_leaf=_is_arr) if _is_arr(l)]
    if not leaves:
        from ..array import device_put
        return device_put(torch.zeros((), dtype=torch.float32))
    with torch.no_grad():
        part, like = _sumsq_f64(leaves)
        devs, _ = norm_plan(leaves)
        return _replicated_scalar(like, devs, {d: torch.sqrt(s).to(torch.float32) for d, s in part.items()})


def clip_scale(sumsq: torch.Tensor, max_norm: float) -> torch.Tensor:
    """f32 scale from the float64 sum of squares: 1 if norm < max_norm else max_norm / norm."""
    norm = torch.sqrt(sumsq)
    return torch.where(norm < max_norm, torch.ones_like(norm), max_norm / norm).to(torch.float32)


class ClipByGlobalNorm(GradientTransformation):
    """The ``GradientTransformation`` of :func:`clip_by_global_norm`; ``chain`` recognises it in front
    of an Adam and fuses the pair."""

    def __new__(cls, max_norm: float):
        max_norm = float(max_norm)

        def init(params):
            return EmptyState()

        def update(grads, state, params=None):
            leaves = [l for l in T.tree_leaves(grads, is_leaf=_is_arr) if _is_arr(l)]
            if not leaves:
                return grads, state
            with torch.no_grad():
                part, _ = _sumsq_f64(leaves)
                sc = {d: clip_scale(s, max_norm) for d, s in part.items()}
                return T.tree_map(lambda g: ShardedArray(g.shape, g.dtype, g.sharding,
                                                         {d: t * sc[d].to(t.dtype) for d, t in g.local.items()})
                                  if _is_arr(g) else g, grads, is_leaf=_is_arr), state

        self = super().__new__(cls, init, update)
        self.max_norm = max_norm
        return self

    def __hash__(self):
        return hash(("clip_by_global_norm", self.max_norm))

    def __eq__(self, other):
        return isinstance(other, ClipByGlobalNorm) and self.max_norm == other.max_norm

    def __ne__(self, other):
        return not self == other


def clip_by_global_norm(max_norm: float) -> GradientTransformation:
    """Scale the gradients by ``1 if norm < max_norm else max_norm / norm`` (``norm``: their
    :func:`global_norm`).  A zero gradient gives scale 1; a non-finite norm propagates as the
    formula gives it.  State: ``EmptyState()``."""
    if not max_norm > 0:
        raise ValueError(f"clip_by_global_norm: max_norm must be positive, got {max_norm}")
    return ClipByGlobalNorm(max_norm)
