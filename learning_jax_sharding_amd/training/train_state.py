"""``flax.training.train_state.TrainState`` equivalent (``case6_attention.py:171-178,214``)."""
from __future__ import annotations

import dataclasses
from typing import Any, Callable

from ..array import ShardedArray
from ..utils import tree as T

__all__ = ["TrainState"]


def _counter(opt_state):
    """The optimizer's device-side step counter, wherever it sits in a (chained) state, or None."""
    from ..optim.adam import ScaleByAdamState
    if isinstance(opt_state, ScaleByAdamState):
        return opt_state.count
    if isinstance(opt_state, tuple):
        for s in opt_state:
            c = _counter(s)
            if c is not None:
                return c
    return None


@dataclasses.dataclass(eq=False)
class TrainState:
    step: Any
    apply_fn: Callable
    params: Any
    tx: Any
    opt_state: Any

    @classmethod
    def create(cls, *, apply_fn: Callable, params, tx, **kwargs) -> "TrainState":
        opt_state = tx.init(params)
        # the step counter is the optimizer's device-side counter when there is one
        count = _counter(opt_state)
        step = count if count is not None else 0
        return cls(step=step, apply_fn=apply_fn, params=params, tx=tx, opt_state=opt_state, **kwargs)

    def apply_gradients(self, *, grads, **kwargs) -> "TrainState":
        if hasattr(self.tx, "apply"):
            new_params, new_opt = self.tx.apply(self.params, grads, self.opt_state)
        else:
            from ..optim.adam import apply_updates
            updates, new_opt = self.tx.update(grads, self.opt_state, self.params)
            new_params = apply_updates(self.params, updates)
        count = _counter(new_opt)
        step = count if count is not None else self.step + 1
        return dataclasses.replace(self, step=step, params=new_params, opt_state=new_opt, **kwargs)

    def replace(self, **kwargs) -> "TrainState":
        return dataclasses.replace(self, **kwargs)


def _flatten(s: TrainState):
    return (s.step, s.params, s.opt_state), (s.apply_fn, s.tx)


def _unflatten(aux, ch):
    return TrainState(step=ch[0], apply_fn=aux[0], params=ch[1], tx=aux[1], opt_state=ch[2])


T.register_pytree_node(TrainState, _flatten, _unflatten)
TrainState.__pytree_child_names__ = ("step", "params", "opt_state")
