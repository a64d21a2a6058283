"""Float64 oracle and per-element error bounds for the fused Adam kernels (tests/test_adam_oracle*.py):
``adam_kernel`` and every ``adam_multi_kernel`` instance of csrc/kernels/elementwise.hip.  Plain
numpy float64 on the CPU; nothing here reads the package under test and no number here comes from a
kernel run.

Oracle (the rule of ops/optim_kernels._torch_adam), in float64 from the exact f32 values the kernel
receives -- b1, b2, eps, wd, lr rounded to f32 first (the kernel arguments are ``float``), t the
integer count the kernel uses:

    m' = b1 m + (1 - b1) g        v' = b2 v + (1 - b2) g^2
    p' = p - lr ((m' / (1 - b1^t)) / (sqrt(v' / (1 - b2^t)) + eps) + wd p)

The gradient g is the f32 value the kernel's moment updates see: the f32 tensor, the bf16 values
widened, the f32 constant of a ConstGrad, ``hip.slab_reduce``'s f32 sum for a SlabGrad (the slab
sum's order is pinned bit for bit elsewhere, as in clip_oracle.py), and under a clipping scale
``f32(g * scale)`` (:func:`scaled`; the kernel rounds that product once, scaled_grad,
elementwise.hip:531-535).

Bound, rounding by rounding.  u = 2^-24: every f32 rounding to nearest multiplies by (1 + d),
|d| <= u; a multiply-add the compiler contracts into an fma loses the product's rounding, so
counting every product's rounding covers both contraction choices (the build uses hipcc's default
contraction).  Lines are those of elementwise.hip: the multi-tensor kernel's 4-wide path / its
scalar path / adam_kernel's 4-wide path / its tail.

  m' (706 / 802 / 476 / 487)      m = b1 * m + (1.f - b1) * g
      u |b1 m|                    the product b1 * m
      u |(1-b1) g|                the product (1.f - b1) * g
      |f32(1-b1) - (1-b1)| |g|    the f32 subtraction 1.f - b1 (exact for b1 >= 0.5, Sterbenz;
                                  evaluated, not assumed)
      u |m'|                      the sum
  v' (707 / 803 / 477 / 488)      v = b2 * v + (1.f - b2) * g * g   (left to right)
      u |b2 v|                    the product b2 * v
      2 u (1-b2) g^2              the products (1.f - b2) * g and (...) * g
      |f32(1-b2) - (1-b2)| g^2    the subtraction 1.f - b2
      u |v'|                      the sum
  bias corrections (579 / 462-463), per launch:
      bc = 1.f - powf(b, t):      powf is off by <= POWF_ULPS ulps, an absolute POWF_ULPS 2u b^t
                                  (an ulp of x is at most 2u |x|); the subtraction adds u bc.
                                  Relative to bc this is r_bc = POWF_ULPS 2u b^t / bc + u -- the
                                  cancellation: b2^t / (1 - b2^t) is ~ 1000 at t = 1, ~ 500 at t = 2
      inv_bc1 = 1.f / bc1         r_inv1 = r_bc1 + u  (a correctly rounded division)
      inv_sqrt_bc2 = rsqrtf(bc2)  r_is2 = r_bc2 / 2 + RSQRTF_ULPS 2u
  p' (711 / 805 / 478-479 / 489-490)
      p - lr * ((m * inv_bc1) / (sqrtf(v) * inv_sqrt_bc2 + eps) + wd * p), with mhat = m'/bc1,
      root = sqrt(v'/bc2), den = root + eps, q = mhat / den, U = q + wd p:
      E_num  = E_m / bc1 + |mhat| (r_inv1 + u)                the product m * inv_bc1
      E_s    = E_v / (2 sqrt v') + u sqrt v'                   sqrtf, correctly rounded (0 at v' = 0:
                                                               every term of v' is then exactly 0)
      E_root = E_s / sqrt(bc2) + root (r_is2 + u)              the product sqrtf(v) * inv_sqrt_bc2
      E_den  = E_root + u den                                  + eps
      E_q    = E_num / den + |q| E_den / den + u |q|           the division, correctly rounded
      E_U    = E_q + u |wd p| + u |U|                          the product wd * p and the sum
      E_p    = lr E_U + u |lr U| + u |p'|                      the product lr * (...) and the final
                                                               rounding of p'

Division and sqrtf are correctly rounded in this build (no fast-math flag in csrc/build.py).  The
HIP math documentation is not part of the ROCm install this was written against, so the ulp errors
of powf and rsqrtf are the OpenCL 3.0 full-profile limits the device library is built to meet:
pow <= 16 ulp, rsqrt <= 2 ulp.  Each bound is first order; the largest relative first-order term is
r_bc2 <= 16 * 2^-23 * b2 / (1 - b2) < 2^-9 (b2 = 0.999, t = 1), so every product of two of them is
below 2^-9 of a first-order term and the factor (1 + 2^-8) covers the second order.  2^-149 is
added for a rounding that underflows gradually.
"""
from collections import namedtuple

import numpy as np

U = 2.0 ** -24
POWF_ULPS, RSQRTF_ULPS = 16.0, 2.0
SECOND_ORDER = 1.0 + 2.0 ** -8
ETA = 2.0 ** -149

Hyper = namedtuple("Hyper", "lr b1 b2 eps wd t")


def f32(x):
    return float(np.float32(x))


def rounded(h):
    """The hyperparameters as the kernel receives them: floats rounded to f32, t an int."""
    return Hyper(f32(h.lr), f32(h.b1), f32(h.b2), f32(h.eps), f32(h.wd), int(h.t))


def a64(x):
    """A torch tensor or array as a flat float64 array (bf16 / f32 values widen exactly)."""
    if hasattr(x, "detach"):
        x = x.detach().double().cpu().numpy()
    return np.asarray(x, dtype=np.float64).reshape(-1)


def a32(x):
    if hasattr(x, "detach"):
        x = x.detach().float().cpu().numpy()
    return np.asarray(x, dtype=np.float32).reshape(-1)


def scaled(g, scale):
    """f32(g * scale): the one rounding of scaled_grad (elementwise.hip:531-535)."""
    return a32(g) * np.float32(scale)


def oracle(p, g, m, v, h):
    """(p', m', v') in float64."""
    h = rounded(h)
    p, g, m, v = a64(p), a64(g), a64(m), a64(v)
    m2 = h.b1 * m + (1.0 - h.b1) * g
    v2 = h.b2 * v + (1.0 - h.b2) * g * g
    bc1, bc2 = 1.0 - h.b1 ** h.t, 1.0 - h.b2 ** h.t
    p2 = p - h.lr * ((m2 / bc1) / (np.sqrt(v2 / bc2) + h.eps) + h.wd * p)
    return p2, m2, v2


def bound(p, g, m, v, h):
    """The allowed |kernel - oracle| of (p', m', v') per element (see the module docstring)."""
    h = rounded(h)
    p, g, m, v = a64(p), a64(g), a64(m), a64(v)
    p2, m2, v2 = oracle(p, g, m, v, h)
    omb1, omb2 = 1.0 - h.b1, 1.0 - h.b2
    e_omb1, e_omb2 = abs(f32(omb1) - omb1), abs(f32(omb2) - omb2)
    E_m = U * np.abs(h.b1 * m) + U * np.abs(omb1 * g) + e_omb1 * np.abs(g) + U * np.abs(m2) + ETA
    E_v = U * np.abs(h.b2 * v) + 2 * U * omb2 * g * g + e_omb2 * g * g + U * np.abs(v2) + ETA
    pw1, pw2 = h.b1 ** h.t, h.b2 ** h.t
    bc1, bc2 = 1.0 - pw1, 1.0 - pw2
    r_bc1 = POWF_ULPS * 2 * U * pw1 / bc1 + U
    r_bc2 = POWF_ULPS * 2 * U * pw2 / bc2 + U
    r_inv1 = r_bc1 + U
    r_is2 = r_bc2 / 2 + RSQRTF_ULPS * 2 * U
    mhat = m2 / bc1
    s = np.sqrt(v2)
    root = s / np.sqrt(bc2)
    den = root + h.eps
    q = mhat / den
    w = h.wd * p
    Uu = q + w
    E_num = E_m / bc1 + np.abs(mhat) * (r_inv1 + U)
    E_s = np.where(v2 > 0, E_v / (2 * np.where(v2 > 0, s, 1.0)) + U * s, 0.0)
    E_root = E_s / np.sqrt(bc2) + root * (r_is2 + U)
    E_den = E_root + U * den
    E_q = E_num / den + np.abs(q) * E_den / den + U * np.abs(q)
    E_U = E_q + U * np.abs(w) + U * np.abs(Uu)
    E_p = h.lr * E_U + U * np.abs(h.lr * Uu) + U * np.abs(p2) + ETA
    return E_p * SECOND_ORDER, E_m * SECOND_ORDER, E_v * SECOND_ORDER


# ---------------------------------------------------------------------------- f32 model of the kernel
FORMS = ("separate", "fma_first", "fma_second")


def _fma(a, b, c):
    """An fma: the float64 product and sum (the product of two f32 is exact) rounded once to f32."""
    return (a.astype(np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(np.float32)


def kernel_model(p, g, m, v, h, form="separate"):
    """The kernel's formula evaluated in f32, one rounding per operation: ``separate`` rounds every
    product, ``fma_first`` / ``fma_second`` contract every multiply-add, fusing the first / the
    second product of a sum of two products.  powf and rsqrtf are the float64 values rounded."""
    assert form in FORMS
    h = rounded(h)
    F = np.float32
    p, g, m, v = a32(p), a32(g), a32(m), a32(v)
    b1, b2, eps, wd, lr = F(h.b1), F(h.b2), F(h.eps), F(h.wd), F(h.lr)
    omb1, omb2 = F(1) - b1, F(1) - b2
    og = (omb2 * g)
    if form == "separate":
        m2 = b1 * m + omb1 * g
        v2 = b2 * v + og * g
    elif form == "fma_first":
        m2 = _fma(m, b1, omb1 * g)
        v2 = _fma(v, b2, og * g)
    else:
        m2 = _fma(g, omb1, b1 * m)
        v2 = _fma(og, g, b2 * v)
    t = float(h.t)
    bc1 = F(1) - F(float(b1) ** t)
    bc2 = F(1) - F(float(b2) ** t)
    inv_bc1 = F(1) / bc1
    inv_sqrt_bc2 = F(1.0 / np.sqrt(np.float64(bc2)))
    s = np.sqrt(v2)
    if form == "separate":
        num = m2 * inv_bc1
        den = s * inv_sqrt_bc2 + eps
        u = num / den + wd * p
        p2 = p - lr * u
    else:
        num = m2 * inv_bc1
        den = _fma(s, inv_sqrt_bc2, eps)
        u = _fma(p, wd, num / den)
        p2 = _fma(u, -lr, p)
    return p2, m2, v2


# ---------------------------------------------------------------------------- hyperparameter cases
LR = 1e-3


def case_names():
    return [f"{c}/wd={wd}" for c in ("fresh", "warm", "small_p", "eps", "large_count") for wd in (0, 0.1)]


def make_case(name, n, seed=0):
    """(Hyper, p, g, m, v) as f32 arrays of n elements; the last n // 8 elements are the band with
    g = m = v = 0 (the result there is p (1 - lr wd): no NaN from 0 / (0 + eps))."""
    kind, wd = name.split("/wd=")
    wd = float(wd)
    rng = np.random.default_rng([seed, sorted(("fresh", "warm", "small_p", "eps", "large_count")).index(kind), n])
    nrm = lambda s: (rng.standard_normal(n) * s).astype(np.float32)   # noqa: E731
    uni = lambda s: (rng.random(n) * s).astype(np.float32)            # noqa: E731
    if kind == "fresh":
        # t = 1 from zero moments: the bias corrections' cancellation, 1 / (1 - b2) = 1000
        h, p, g, m, v = Hyper(LR, 0.9, 0.999, 1e-8, wd, 1), nrm(1), nrm(1), nrm(0), uni(0)
    elif kind == "warm":
        # t = 3, warm moments: both terms of each moment update, b^t far from 0 and from 1
        h, p, g, m, v = Hyper(LR, 0.9, 0.999, 1e-8, wd, 3), nrm(1), nrm(1), nrm(0.1), uni(1e-3)
    elif kind == "small_p":
        # |p| ~ lr: the final rounding of p' (u |p'|) no longer hides the update's own error
        h, p, g, m, v = Hyper(LR, 0.9, 0.999, 1e-8, wd, 3), nrm(LR), nrm(1), nrm(0.1), uni(1e-3)
    elif kind == "eps":
        # sqrt(v' / bc2) ~ eps: where eps enters the denominator is visible
        h, p, g, m, v = Hyper(LR, 0.9, 0.999, 1e-3, wd, 3), nrm(LR), nrm(1e-4), nrm(1e-4), uni(1e-8)
    elif kind == "large_count":
        # t = 5000, |p| ~ lr: b1^t = 0, b2^t = 0.0067 -- the count itself, and with the powf term
        # gone the sharpest bound on the update (decay placement, a scaled update)
        h, p, g, m, v = Hyper(LR, 0.9, 0.999, 1e-8, wd, 5000), nrm(LR), nrm(1), nrm(0.1), uni(1e-3)
    else:
        raise KeyError(name)
    band = n - n // 8
    g[band:], m[band:], v[band:] = 0, 0, 0
    return h, p, g, m, v


# ---------------------------------------------------------------------------- tile plan of one launch
def launch_tiles(tensors, forced_rows=0):
    """(launch height, [per-tensor tile height], total tiles) of one adam_multi launch, from the rule
    the launcher documents: 32-row tiles, 64 when a tensor carries MX shadows (the others keep 32);
    a 4-wide tensor with C % 64 == 0 and no MX shadows whose gradient has >= 2x (>= 4x) the slabs of
    the launch's lightest slab gradient gets tiles of half (a quarter of) the height, at least 16.
    ``tensors``: dicts with R, C, vec (the 4-wide path's alignment conditions hold), mx, S (slabs, 0
    for the other sources)."""
    any_mx = any(t["mx"] for t in tensors)
    rows = forced_rows if forced_rows in (16, 32, 64) else (64 if any_mx else 32)
    slabbed = [t["S"] for t in tensors if t["S"] > 0]
    s_min = min(slabbed) if slabbed else 0
    heights, tiles = [], 0
    for t in tensors:
        short_ok = t["vec"] and t["C"] % 64 == 0 and not t["mx"]
        hgt = rows
        if short_ok and forced_rows == 0 and rows == 64:
            hgt = 32
        if hgt >= 32 and s_min > 0 and short_ok and t["S"] >= 2 * s_min:
            hgt = 16 if (t["S"] >= 4 * s_min or hgt == 32) else 32
        heights.append(hgt)
        tiles += -(-t["R"] // hgt) * -(-t["C"] // 64)
    return rows, heights, tiles


# ---------------------------------------------------------------------------- figures
class Figures:
    """Collects comparisons: every :meth:`check` prints its ``adam-figures`` line, :meth:`finish`
    fails the test afterwards if any missed, so all figures print before the failure."""

    def __init__(self):
        self.failures, self.worst = [], {}

    def check(self, name, got, want, allowed):
        """``got`` against ``want`` within ``allowed`` at every element (arrays, or lists of arrays
        taken together); returns the worst fraction of the bound."""
        cat = lambda x: np.concatenate([a64(t) for t in x]) if isinstance(x, (list, tuple)) else a64(x)  # noqa: E731
        got, want, allowed = cat(got), cat(want), cat(allowed)
        assert got.shape == want.shape == allowed.shape and got.size > 0, (name, got.shape, want.shape)
        err = np.abs(got - want)
        with np.errstate(divide="ignore", invalid="ignore"):
            frac = np.where(allowed > 0, err / allowed, np.where(err == 0, 0.0, np.inf))
        frac = np.where(np.isfinite(got), frac, np.inf)          # a NaN / inf result never passes
        i = int(np.argmax(frac))
        worst = float(frac[i])
        print(f"adam-figures {name} n={got.size} max_abs_err={float(err[i]) if np.isfinite(err[i]) else float('nan'):.3e} "
              f"worst_fraction_of_bound={worst:.3f}")
        out = name.rsplit(" ", 1)[-1]
        self.worst[out] = max(self.worst.get(out, 0.0), worst)
        if not worst < 1.0:
            self.failures.append(f"{name}: element {i} got {got[i]!r} want {want[i]!r} allowed {allowed[i]:.3e} "
                                 f"({worst:.3f} of the bound)")
        return worst

    def equal(self, name, ok, detail=""):
        """An exact (bit-for-bit) condition, reported with the figures."""
        if not ok:
            self.failures.append(f"{name}: not bit-identical {detail}")

    def finish(self):
        assert not self.failures, "\n".join(self.failures)
