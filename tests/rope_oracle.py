"""The float64 oracle of the rotary embedding and the bounds tests/test_rope.py and
tests/test_rope_gpu.py hold every implementation to.

Convention (half-split pairs): for a head vector x[0:D] at global position p, h = D / 2, i in [0, h):

    ang      = p * theta^(-2 i / D)
    y[i]     = x[i]     cos(ang) - x[i + h] sin(ang)
    y[i + h] = x[i + h] cos(ang) + x[i]     sin(ang)

and the backward is the same map with -ang.  The oracle keeps the table and the arithmetic in
float64.

Bounds.  With m = |x_a| |cos| + |x_b| |sin| per element (first half: a = i, b = i + h; second half:
a = i + h, b = i):

* an f32 output is within 3.5 * 2^-24 * m of the oracle: one rounding of the table entry, one of the
  products and one of the result, each at most 2^-24 of m; the extra half covers second-order terms;
* a bf16 output is within one bf16 ulp of the oracle rounded to bf16, in the convention of
  tests/test_norm_gpu.py: |got - want| <= 2^-7 |want| + the f32 allowance, want = bf16(oracle).  The
  f32 allowance (3.5 * 2^-24 * m here) belongs to it because the value that is rounded to bf16 is
  the f32 result, not the oracle: rounding is monotone, so the two roundings differ by at most one
  step more than the f32 results differ.  It matters only where the two products cancel (|y| below
  about 2^-15 m), where one bf16 ulp of y is smaller than the f32 error of the products.
"""
import numpy as np
import torch

F32_UNITS = 3.5
EPS_F32 = F32_UNITS * 2.0 ** -24


def table64(S, D, theta, offset):
    """(cos, sin) in float64 of positions offset .. offset + S, [S, D / 2] each."""
    inv_freq = np.power(np.float64(theta), -2.0 * np.arange(D // 2, dtype=np.float64) / D)
    ang = np.arange(offset, offset + S, dtype=np.float64)[:, None] * inv_freq[None, :]
    return torch.from_numpy(np.cos(ang)), torch.from_numpy(np.sin(ang))


def rotate64(x, offset, theta, inverse=False):
    """(y, m) in float64 for x of shape (B, S, H, D) in any dtype: the rotation (by -ang when
    ``inverse``) and the magnitude the bounds scale with."""
    B, S, H, D = x.shape
    h = D // 2
    cos, sin = table64(S, D, theta, offset)
    cos, sin = cos.view(1, S, 1, h), sin.view(1, S, 1, h)
    if inverse:
        sin = -sin
    xd = x.detach().double().cpu()
    a, b = xd[..., :h], xd[..., h:]
    y = torch.cat([a * cos - b * sin, b * cos + a * sin], dim=-1)
    m = torch.cat([a.abs() * cos.abs() + b.abs() * sin.abs(), b.abs() * cos.abs() + a.abs() * sin.abs()], dim=-1)
    return y, m


def _ordered(t):
    """bf16 values as integers in value order (sign-magnitude bits unfolded)."""
    bits = t.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
    mag = bits & 0x7FFF
    return torch.where((bits & 0x8000) != 0, -mag, mag)


def check(name, got, y64, m64):
    """Assert ``got`` (f32 or bf16) against the oracle under the module's bounds; prints the figures first."""
    got = got.detach().cpu()
    assert tuple(got.shape) == tuple(y64.shape), (name, got.shape, y64.shape)
    assert torch.isfinite(got).all(), name
    if got.dtype == torch.bfloat16:
        want = y64.to(torch.bfloat16).double()
        err = (got.double() - want).abs()
        allowed = 2.0 ** -7 * want.abs() + EPS_F32 * m64
        steps = (_ordered(got) - _ordered(y64.to(torch.bfloat16))).abs()
        frac = float((err / allowed.clamp_min(1e-300)).max()) if float(err.max()) > 0 else 0.0
        print(f"rope-figures {name} bf16 worst_fraction_of_bound={frac:.3f} max_steps={int(steps.max())} "
              f"fraction_off={float((steps > 0).double().mean()):.3e} "
              f"off_by_more_than_one_step={int((steps > 1).sum())}")
        assert (err <= allowed).all(), (name, frac)
    else:
        assert got.dtype == torch.float32, got.dtype
        units = ((got.double() - y64).abs() / (2.0 ** -24 * m64).clamp_min(1e-300))
        units = torch.where(m64 > 0, units, (got.double() - y64).abs() * float("inf")).nan_to_num(nan=0.0)
        worst = float(units.max())
        print(f"rope-figures {name} f32 worst_units_of_2^-24_m={worst:.3f} (allowed {F32_UNITS})")
        assert worst <= F32_UNITS, (name, worst)
