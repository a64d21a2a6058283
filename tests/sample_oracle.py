"""Float64 numpy oracle of the sampling rule (``ops/kernels.py::sample_reference`` states it).

The uniforms come from ``random._philox_np`` with the counter layout of a draw, ``(c0 = i >> 2, c1 = lo, c2 = hi,
c3 = 0x5A3D)``, word ``i & 3``.  Per row the oracle gives the kept set's threshold ``tau`` and size ``kept``, the perturbed
scores, the winner, and two margins that say how far the row is from a decision another valid evaluation could
take differently:

* ``gap``: the best minus the second-best perturbed score over the kept set (``inf`` with one kept entry);
* ``pmargin``: ``min over distinct values v of |mass{x > v} / S - p|`` (``inf`` without top-p): how far the nearest
  tie group's boundary is from ``p``, in probability.
"""
import numpy as np

from learning_jax_sharding_amd import random as R

STREAM = 0x5A3D


def uniforms(key, V, hi, lo):
    """u_i of one draw, i = 0 .. V-1, float64."""
    i = np.arange(V, dtype=np.uint64)
    c1 = np.full(V, int(lo) & 0xFFFFFFFF, dtype=np.uint64)
    words = R._philox_np(i >> np.uint64(2), c1, key.k0, key.k1, int(hi) & 0xFFFFFFFF, STREAM)
    word = np.choose((i & np.uint64(3)).astype(np.int64), words)
    return R._u01(word)


def gumbel(u):
    return -np.log(-np.log(u))


def z_of(x, temperature):
    """z = f32(x) * f32(1 / T), the f32 product, as float64."""
    return (np.asarray(x, np.float32) * np.float32(1.0 / float(temperature))).astype(np.float64)


def kept_set(x, temperature=1.0, top_k=None, top_p=None):
    """(mask, tau, pmargin) of one row ``x`` (float64 values of the f32 / bf16 logits)."""
    x = np.asarray(x, np.float64)
    V = x.shape[0]
    tau = -np.inf
    if top_k is not None and top_k < V:
        tau = np.sort(x)[::-1][top_k - 1]
    mask = x >= tau
    pmargin = np.inf
    if top_p is not None and top_p < 1.0:
        z = z_of(x, temperature)
        w = np.where(mask, np.exp(z - z[mask].max()), 0.0)
        S = w.sum()
        vals = np.unique(x[mask])[::-1]                      # distinct kept values, descending
        mass_at = _mass_at(x, w, mask)
        above = np.concatenate([[0.0], np.cumsum(mass_at)[:-1]]) / S
        keep_v = above < top_p
        pmargin = np.abs(above - top_p).min()
        tau = vals[keep_v].min()
        mask = x >= tau
    return mask, tau, pmargin


def _mass_at(x, w, mask):
    """The mass of each distinct kept value, descending by value."""
    order = np.argsort(-x[mask], kind="stable")
    xs, ws = x[mask][order], w[mask][order]
    starts = np.flatnonzero(np.concatenate([[True], xs[1:] != xs[:-1]]))
    return np.add.reduceat(ws, starts)


def sample_row(x, key=None, hi=0, lo=0, temperature=1.0, top_k=None, top_p=None):
    """dict(token, kept, tau, gap, pmargin, score) of one row."""
    x = np.asarray(x, np.float64)
    V = x.shape[0]
    if key is None:
        return dict(token=int(np.flatnonzero(x == x.max())[0]), kept=V, tau=-np.inf, gap=np.inf, pmargin=np.inf,
                    score=float(x.max()))
    mask, tau, pmargin = kept_set(x, temperature, top_k, top_p)
    s = np.where(mask, z_of(x, temperature) + gumbel(uniforms(key, V, hi, lo)), -np.inf)
    best = s.max()
    token = int(np.flatnonzero(s == best)[0])
    rest = np.delete(s, token)
    gap = best - rest.max() if mask.sum() > 1 else np.inf
    return dict(token=token, kept=int(mask.sum()), tau=float(tau), gap=float(gap), pmargin=float(pmargin),
                score=float(best))


def sample(x2d, key=None, batch_offset=0, pos=None, **kw):
    """Row-wise :func:`sample_row` of ``[B, V]`` values with ``hi = batch_offset + b``, ``lo = pos[b]`` (0 without)."""
    return [sample_row(x2d[b], key, batch_offset + b, 0 if pos is None else int(pos[b]), **kw)
            for b in range(len(x2d))]


def margin(score, gumbel_err=0.0):
    """The gap above which another valid evaluation takes the oracle's winner: ``2^-22 |score|`` covers the f32 roundings
    of z and of the sum; an evaluation whose Gumbel value is not float64 adds ``4 x`` its measured maximum absolute error
    (the project's factor over a measured error).  ``sample_reference`` takes the Gumbel value in float64."""
    return 4.0 * gumbel_err + 2.0 ** -22 * abs(score)


# ----------------------------------------------------------------------------- inputs with room around p
# A row is six tie groups of distinct values: the head groups have the sizes HEAD in every row, the tail groups
# split the rest of the row at random.  Group g carries the probability MASS[g] at temperature T, so the mass
# above a value moves in steps of at least 0.08: a p half way between two steps is >= 0.04 from every boundary,
# far more than the 1e-3 the tests ask of ``pmargin`` (and assert).
HEAD = (1, 1, 2)
MASS = (0.30, 0.22, 0.16, 0.14, 0.10, 0.08)


def rows(B, V, temperature=1.0, seed=0, head=HEAD, bf16=False):
    """``[B, V]`` float32 logits (bf16-representable with ``bf16``), a fresh permutation and offset per row."""
    rng = np.random.default_rng(seed)
    nt = len(MASS) - len(head)
    out = np.empty((B, V), np.float32)
    for b in range(B):
        rest = V - sum(head) - nt
        cuts = np.sort(rng.integers(0, rest + 1, nt - 1))
        sizes = list(head) + [int(s) + 1 for s in np.diff(np.concatenate([[0], cuts, [rest]]))]
        vals = np.concatenate([np.full(n, temperature * np.log(q / n)) for q, n in zip(MASS, sizes)])
        out[b] = (vals + rng.uniform(-3.0, 3.0))[rng.permutation(V)]
    if bf16:
        import torch
        out = torch.from_numpy(out).bfloat16().float().numpy()
    return out


def p_between(step, groups=len(MASS)):
    """A top_p that keeps exactly the groups ``0 .. step - 1`` of the distribution over the first ``groups`` groups
    (what a top-k leaves, renormalised): half way between the mass above group ``step - 1`` and that above ``step``."""
    c = np.concatenate([[0.0], np.cumsum(MASS[:groups])]) / sum(MASS[:groups])
    return float(0.5 * (c[step - 1] + c[step]))


def modes(V, temperature):
    """(name, sampling arguments) of every filter combination the tests run on :func:`rows`."""
    t = dict(temperature=temperature)
    return [("none", dict(t)),
            ("k", dict(t, top_k=3)),                         # the third place lies inside the tie group of two
            ("k half", dict(t, top_k=max(V // 2, 4))),       # a threshold in the tail
            ("k1", dict(t, top_k=1)),
            ("p", dict(t, top_p=p_between(4))),              # three head groups and a tail group
            ("k,p", dict(t, top_k=3, top_p=p_between(2, 3)))]


# A top_p below every probability keeps exactly the maximum's tie group.  Its only boundary nearer than 1e-3 is
# the maximum's own: nothing lies above the maximum, a mass of exactly 0 in every arithmetic; the next boundary
# is MASS[0] away.  ``pmargin`` (which counts the zero) is 1e-6 here by construction, so this case states its
# own precondition instead of the 1e-3.
P_TINY = 1e-6
