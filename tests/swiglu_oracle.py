"""The float64 oracle of the SwiGLU activation and the bounds tests/test_swiglu.py and
tests/test_swiglu_gpu.py hold every implementation to.

With s = sigmoid(g) and c = sigmoid(-g) = 1 - s, all in float64 from the inputs as stored:

    h  = g s u                      (forward)
    du = dh s g                     (backward, recomputed from g, u, dh)
    dg = dh s u (1 + g c)

Bounds.  One unit is 2^-24, the relative error of one f32 rounding to nearest.  With

    w    = 1 + c |g|
    m_h  = w |h|,    m_du = w |du|,    m_dg = w |dh u s| (1 + |g| c)

an f32 output is within U * 2^-24 * m of the oracle, and a bf16 output within one bf16 ulp of the
oracle rounded to bf16 plus that allowance (the convention of tests/rope_oracle.py: |got - want| <=
2^-7 |want| + U 2^-24 m, want = bf16(oracle); the value rounded to bf16 is the f32 result, not the
oracle).  w is the conditioning of s under an error of the exponential's argument; 1 + |g| c is the
term sum of 1 + g c, which cancels near g = -1.278.

The constants, rounding by rounding through the instruction sequence of csrc/kernels/swiglu.hip
(relative errors in units; sigma, c and e = exp(-|g|) are the exact values):

  1. a = fl(-|g| L), L = fl(log2 e): L is off by 0.22 units and the product rounds once, so a is
     off by at most 1.22 units relative, which is 1.22 |g| units relative on 2^a.
  2. v_exp_f32 is a 1-ulp instruction: 2 units.        e':  E = 1.22 |g| + 2
  3. d = fl(1 + e'): 1 unit.   4. r = v_rcp_f32(d), 1 ulp: 2 units.
     With q = e / (1 + e) and p = 1 / (1 + e) (q = c, p = s for g >= 0 and the other way round
     below):                                           r':  q E + 3
  5. er = fl(e' r'): the errors of e' enter as (1 - q) = p.   er':  p E + 4
     s is r for g >= 0 and er below, c is er for g >= 0 and r below:

         err(s) <= c E + 3 + [g < 0],        err(c) <= s E + 3 + [g >= 0]

  6. h = fl(fl(g s) u) and du = fl(fl(dh s) g): two products.

         err(h), err(du) <= c (1.22 |g| + 2) + 5 + [g < 0]

     Over w this is largest at g -> 0 from below (c = 1/2, w = 1): 7 units.  It falls to 1.22 for
     large |g|, where c |g| dominates both sides.
  7. t = fma(g, c, 1) rounds once (1 unit of |t| <= 1 + |g| c) and carries |g| c err(c);
     dg = fl(fl(fl(dh s) u) t) is three products.  With f = |g| c / (1 + |g| c):

         err(dg) <= err(s) + 4 + f err(c)          relative to |dh u s| (1 + |g| c)

     Over w this is again largest at g -> 0 from below (f = 0): 5 + 4 = 9 units; at g = 1 it is
     7.3, at g = -2 5.1 (``derived_units`` evaluates both expressions on a grid).

U_H = U_DU = 7.5 and U_DG = 9.5: the suprema and a half for the second-order terms, as in
tests/rope_oracle.py.  Measured on 2.2M samples (scripts/swiglu_probe.py --figures), worst units for
h / du / dg: the host formulation (ops/kernels.py swiglu_reference: torch.exp of the exact argument
and a true division) 3.51 / 3.37 / 4.50, the kernels 3.53 / 3.71 / 4.63.  What the derivation allows the
kernel beyond the host's sequence is the argument product (step 1) and the second unit each of
v_exp_f32 and v_rcp_f32.  No rounding of the sequence is idle: the product e r for g < 0 (step 5) could
only be traded for a second v_rcp_f32, which costs more and is itself two units.
"""
import torch

U_H = 7.5
U_DU = 7.5
U_DG = 9.5
UNIT = 2.0 ** -24


def derived_units(g):
    """(sup-expression for h / du, for dg) of the docstring at the float64 points ``g``, over w."""
    g = g.double()
    s, c = torch.sigmoid(g), torch.sigmoid(-g)
    a = g.abs()
    E = 1.22 * a + 2.0
    neg = (g < 0).double()
    err_s = c * E + 3.0 + neg
    err_c = s * E + 3.0 + (1.0 - neg)
    w = 1.0 + c * a
    f = a * c / (1.0 + a * c)
    return (err_s + 2.0) / w, (err_s + 4.0 + f * err_c) / w


def _sc(g):
    g = g.detach().double().cpu()
    return g, torch.sigmoid(g), torch.sigmoid(-g)


def forward64(g, u):
    """(h, m_h) in float64 from g and u as stored."""
    g, s, c = _sc(g)
    h = g * s * u.detach().double().cpu()
    return h, (1.0 + c * g.abs()) * h.abs()


def backward64(g, u, dh):
    """(dg, m_dg, du, m_du) in float64 from g, u and dh as stored."""
    g, s, c = _sc(g)
    u, dh = u.detach().double().cpu(), dh.detach().double().cpu()
    w = 1.0 + c * g.abs()
    du = dh * s * g
    dg = dh * s * u * (1.0 + g * c)
    return dg, w * (dh * u * s).abs() * (1.0 + g.abs() * c), du, w * du.abs()


def inputs(shape, in_dtype, out_dtype, seed=0):
    """(g, u, dh) for the bounded cases: |g| <= 80 with exact zeros, a run across [-1.4, -1.1] and both
    ends +-80 (as far as the element count allows); 2^-10 <= |u|, |dh| <= 8, and values of order one
    where g is +-80, so that no result is f32-subnormal."""
    gen = torch.Generator().manual_seed(seed + 13 * shape[-1] + shape[-2])
    n = 1
    for d in shape:
        n *= d

    def mag(scale):
        t = torch.randn(n, generator=gen) * scale
        return torch.where(t < 0, -1.0, 1.0) * t.abs().clamp(2.0 ** -10, 8.0)

    g = (4.0 * torch.randn(n, generator=gen)).clamp(-80.0, 80.0)
    u, dh = mag(2.0), mag(1.0)
    k = min(16, max(1, (n - 4) // 2))
    g[:k] = torch.linspace(-1.4, -1.1, k)
    g[k], g[k + 1] = 0.0, -0.0
    g[-1], g[-2] = 80.0, -80.0
    u[-2:], dh[-2:] = torch.tensor([1.5, -0.75]), torch.tensor([-1.25, 0.875])
    return g.view(shape).to(in_dtype), u.view(shape).to(in_dtype), dh.view(shape).to(out_dtype)


def check(name, got, y64, m64, units):
    """Assert ``got`` (f32 or bf16) against the oracle under the module's bounds; prints the figures first."""
    got = got.detach().cpu()
    assert tuple(got.shape) == tuple(y64.shape), (name, got.shape, y64.shape)
    assert torch.isfinite(got).all(), name
    if got.dtype == torch.bfloat16:
        want = y64.to(torch.bfloat16).double()
        err = (got.double() - want).abs()
        allowed = 2.0 ** -7 * want.abs() + units * UNIT * m64
        frac = float((err / allowed.clamp_min(1e-300)).max()) if float(err.max()) > 0 else 0.0
        print(f"swiglu-figures {name} bf16 worst_fraction_of_bound={frac:.3f} (U = {units})")
        assert (err <= allowed).all(), (name, frac)
        return frac
    assert got.dtype == torch.float32, got.dtype
    err = (got.double() - y64).abs()
    worst = float(torch.where(err > 0, err / (UNIT * m64).clamp_min(1e-300), torch.zeros_like(err)).max())
    print(f"swiglu-figures {name} f32 worst_units_of_2^-24_m={worst:.3f} (allowed {units})")
    assert worst <= units, (name, worst)
    return worst
