"""Float64 oracles and error bounds for global-norm clipping and the learning-rate schedules
(tests/test_clip_sched*.py).  Nothing here is derived from the results of the code under test.

Host bound (the rule of tests/test_norm_gpu.py and tests/test_xent_gpu.py): a result may differ
from the float64 oracle by ``4 E_ref + 2^-23 max|oracle|``, ``E_ref`` being the error of torch's own
f32 evaluation of the same quantity.

Bound of the ``grad_sumsq`` kernel, rounding by rounding, in units of u = 2^-24 (f32 round to
nearest: every rounding multiplies by (1 + d), |d| <= u).  Every term g^2 is non-negative, so the
relative error of the sum is at most the largest relative error any one term collects on its way
through the summation:

    1          the square g * g (0 when the compiler fuses it into the add)
    A          the thread's running f32 sum: a term takes part in at most A adds, A = 8 elements
               per 32 x 64 tile (4 columns x 2 rows, or 1 column x 8 rows) times the tiles a block
               walks, ceil(tiles / 1024) (1 for every shape tested here)
    6          the 64-lane xor butterfly: log2(64) adds
    3          the block's four wave sums added in wave order

    sumsq relative error <= (1 + u)^(A + 10) - 1,   allowed = (A + 10) u (1 + 2^-10)

(the last factor covers the second-order terms, (A + 10)^2 u^2 / 2 << 2^-10 (A + 10) u, and the
float64 stages: <= 1088 adds of 2^-53 each per launch).  The gradient the kernel squares is, for
split-K slabs, their f32 sum in slab_reduce's order -- the oracle squares exactly those f32 values
(``hip.slab_reduce``'s output), so the slab additions are not part of the bound.  The norm is
sqrt(sumsq) in float64 rounded once to f32: relative error <= half of the above + u.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
SUMSQ_MAX_BLOCKS, SUMSQ_TILE_ROWS = 1024, 32


# ---------------------------------------------------------------------------- schedules (float64)
def linear(init, end, steps, begin, count):
    init, end, steps, begin, count = (float(v) for v in (init, end, steps, begin, count))
    if steps <= 0:
        return init
    c = min(max(count - begin, 0.0), steps)
    return (init - end) * (1.0 - c / steps) + end


def cosine(init, decay_steps, alpha, count):
    init, decay_steps, alpha, count = (float(v) for v in (init, decay_steps, alpha, count))
    c = min(count, decay_steps)
    return init * ((1.0 - alpha) * 0.5 * (1.0 + math.cos(math.pi * c / decay_steps)) + alpha)


def warmup_cosine(init, peak, warmup, decay, end, count):
    if count < warmup:
        return linear(init, peak, warmup, 0, count)
    return cosine(peak, decay - warmup, float(end) / float(peak), count - warmup)


def ulps64(a, b):
    """|a - b| in units of the float64 spacing at b."""
    return abs(a - b) / np.spacing(np.float64(abs(b)) if b != 0 else np.float64(0.0))


def ulps32(a, b):
    """|a - b| in units of the f32 spacing at b (a an f32 value, b the float64 oracle)."""
    sp = np.spacing(np.float32(abs(b))) if b != 0 else np.spacing(np.float32(0.0))
    return abs(float(a) - float(b)) / float(sp)


# ---------------------------------------------------------------------------- norm and clipping
def sumsq64(tensors):
    return sum(float((t.detach().double().cpu() ** 2).sum()) for t in tensors)


def norm64(tensors):
    return math.sqrt(sumsq64(tensors))


def norm32(tensors):
    """torch's own f32 evaluation: the norm of the per-tensor f32 norms (torch._foreach_norm's way)."""
    return float(torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(t.float()) for t in tensors])))


def scale64(norm, max_norm):
    return 1.0 if norm < max_norm else max_norm / norm


def host_allowed(want64, ref32):
    """4 E_ref + 2^-23 max|oracle| (scalars or tensors)."""
    want64 = torch.as_tensor(want64, dtype=torch.float64)
    ref32 = torch.as_tensor(ref32).to(torch.float64)
    return 4.0 * (ref32 - want64).abs().max().item() + 2.0 ** -23 * want64.abs().max().item()


def clip_adamw(params, grads_per_step, schedule, max_norm, b1, b2, eps, wd, dtype):
    """The clipped AdamW loop on plain torch tensors in ``dtype``: per step the global norm of that
    step's gradients, scale = 1 if norm < max_norm else max_norm / norm, lr = schedule(count) with
    the count before the increment, bias corrections with count + 1.  Returns the parameter lists
    after every step."""
    p = [t.to(dtype).clone() for t in params]
    m = [torch.zeros_like(t) for t in p]
    v = [torch.zeros_like(t) for t in p]
    out = []
    for count, grads in enumerate(grads_per_step):
        g = [t.to(dtype) for t in grads]
        norm = torch.sqrt(sum((t * t).sum() for t in g))
        sc = torch.ones_like(norm) if bool(norm < max_norm) else max_norm / norm
        lr = torch.tensor(schedule(count), dtype=torch.float64).to(dtype)
        t1 = count + 1
        for i in range(len(p)):
            gi = g[i] * sc
            m[i] = b1 * m[i] + (1.0 - b1) * gi
            v[i] = b2 * v[i] + (1.0 - b2) * gi * gi
            upd = (m[i] / (1.0 - b1 ** t1)) / (torch.sqrt(v[i] / (1.0 - b2 ** t1)) + eps) + wd * p[i]
            p[i] = p[i] - lr * upd
        out.append([t.clone() for t in p])
    return out


# ---------------------------------------------------------------------------- grad_sumsq bound
def sumsq_tiles(shapes):
    n = 0
    for shape in shapes:
        R, C = (shape[0], shape[1]) if len(shape) == 2 else (1, int(np.prod(shape)))
        n += -(-R // SUMSQ_TILE_ROWS) * -(-C // 64)
    return n


def sumsq_allowed_units(shapes):
    """The allowed relative error of one launch's sum of squares over tensors of ``shapes``, in units
    of 2^-24 (see the module docstring)."""
    A = 8 * max(1, -(-sumsq_tiles(shapes) // SUMSQ_MAX_BLOCKS))
    return (A + 10) * (1.0 + 2.0 ** -10)
