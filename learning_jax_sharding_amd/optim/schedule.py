"""Learning-rate schedules (``optax`` subset): small immutable, hashable objects.

A schedule is callable on a host ``int`` (the count *before* the step's increment: step 0 uses
``schedule(0)``) and returns a Python float computed in float64.  It carries its parameters
(``kind`` and five float64 ``params``) so that the optimizer's ``step_hyper`` HIP launch evaluates
the same formula on the device from the device-side step counter, inside a captured graph;
``torch_value`` is the same formula on a count tensor for host devices (no ``.item()``).

    linear          c = clip(count - begin, 0, steps);  (init - end) * (1 - c / steps) + end
    cosine          c = min(count, decay_steps);  init * ((1 - alpha) * 0.5 * (1 + cos(pi c / decay_steps)) + alpha)
    warmup-cosine   linear(init, peak, warmup_steps) below warmup_steps, then
                    cosine(peak, decay_steps - warmup_steps, alpha = end / peak) at count - warmup_steps
"""
from __future__ import annotations

import math

import torch

__all__ = ["Schedule", "constant_schedule", "linear_schedule", "cosine_decay_schedule",
           "warmup_cosine_decay_schedule"]

# kinds, as the step_hyper kernel numbers them (csrc/kernels/clip.hip)
CONSTANT, LINEAR, COSINE, WARMUP_COSINE = 0, 1, 2, 3
_NAMES = ("constant", "linear", "cosine_decay", "warmup_cosine_decay")


def _linear(init, end, steps, begin, count):
    if steps <= 0:
        return init
    c = min(max(count - begin, 0.0), steps)
    return (init - end) * (1.0 - c / steps) + end


def _cosine(init, decay_steps, alpha, count):
    c = min(count, decay_steps)
    return init * ((1.0 - alpha) * 0.5 * (1.0 + math.cos(math.pi * c / decay_steps)) + alpha)


def _linear_t(init, end, steps, begin, count):
    if steps <= 0:
        return torch.full_like(count, init)
    c = torch.clamp(count - begin, 0.0, steps)
    return (init - end) * (1.0 - c / steps) + end


def _cosine_t(init, decay_steps, alpha, count):
    c = torch.clamp(count, max=decay_steps)
    return init * ((1.0 - alpha) * 0.5 * (1.0 + torch.cos(math.pi * c / decay_steps)) + alpha)


class Schedule:
    """``kind`` (one of the four) and its parameters as five float64 values, unused ones 0:

        constant        (value)
        linear          (init, end, transition_steps, transition_begin)
        cosine          (init, decay_steps, alpha)
        warmup-cosine   (init, peak, warmup_steps, decay_steps - warmup_steps, end / peak)
    """
    __slots__ = ("kind", "params")

    def __init__(self, kind: int, *params: float):
        object.__setattr__(self, "kind", int(kind))
        object.__setattr__(self, "params", tuple(float(p) for p in params) + (0.0,) * (5 - len(params)))

    def __setattr__(self, k, v):
        raise AttributeError("schedules are immutable")

    def __hash__(self):
        return hash(("schedule", self.kind, self.params))

    def __eq__(self, other):
        return isinstance(other, Schedule) and (self.kind, self.params) == (other.kind, other.params)

    def __repr__(self):
        return f"{_NAMES[self.kind]}_schedule{self.params}"

    def __call__(self, count: int) -> float:
        p, c = self.params, float(count)
        if self.kind == CONSTANT:
            return p[0]
        if self.kind == LINEAR:
            return _linear(p[0], p[1], p[2], p[3], c)
        if self.kind == COSINE:
            return _cosine(p[0], p[1], p[2], c)
        if c < p[2]:
            return _linear(p[0], p[1], p[2], 0.0, c)
        return _cosine(p[1], p[3], p[4], c - p[2])

    def torch_value(self, count: torch.Tensor) -> torch.Tensor:
        """The schedule at a 0-d integer ``count`` tensor, in float64 on its device, as f32."""
        p, c = self.params, count.to(torch.float64)
        if self.kind == CONSTANT:
            v = torch.full_like(c, p[0])
        elif self.kind == LINEAR:
            v = _linear_t(p[0], p[1], p[2], p[3], c)
        elif self.kind == COSINE:
            v = _cosine_t(p[0], p[1], p[2], c)
        else:
            v = torch.where(c < p[2], _linear_t(p[0], p[1], p[2], 0.0, c), _cosine_t(p[1], p[3], p[4], c - p[2]))
        return v.to(torch.float32)


def constant_schedule(value: float) -> Schedule:
    return Schedule(CONSTANT, value)


def linear_schedule(init_value: float, end_value: float, transition_steps: int, transition_begin: int = 0) -> Schedule:
    return Schedule(LINEAR, init_value, end_value, transition_steps, transition_begin)


def cosine_decay_schedule(init_value: float, decay_steps: int, alpha: float = 0.0) -> Schedule:
    if not decay_steps > 0:
        raise ValueError(f"cosine_decay_schedule: decay_steps must be positive, got {decay_steps}")
    return Schedule(COSINE, init_value, decay_steps, alpha)


def warmup_cosine_decay_schedule(init_value: float, peak_value: float, warmup_steps: int, decay_steps: int,
                                 end_value: float = 0.0) -> Schedule:
    if not decay_steps > warmup_steps:
        raise ValueError(f"warmup_cosine_decay_schedule: decay_steps ({decay_steps}) must exceed warmup_steps "
                         f"({warmup_steps})")
    if peak_value == 0:
        raise ValueError("warmup_cosine_decay_schedule: peak_value must not be 0 (the decay's alpha is end / peak)")
    return Schedule(WARMUP_COSINE, init_value, peak_value, warmup_steps, decay_steps - warmup_steps,
                    end_value / peak_value)
