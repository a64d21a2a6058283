"""Integer oracle of "MX-quantise a block of 32": plain torch on bit patterns, nothing of the package.

The rule (OCP MX v1.0 with e4m3fn elements and an e8m0 scale, plus this project's no-saturation bump).  A
block is 32 finite values; ``amax`` is their largest magnitude.

* shared exponent ``X = -127`` for ``amax == 0``, else ``clamp(floor(log2 amax) - 8 + [amax > 1.75 *
  2^floor(log2 amax)], -127, 127)``; the scale byte is ``X + 127``;
* element byte: ``v * 2^-X`` rounded to nearest, ties to even, onto the e4m3fn grid (subnormal step 2^-9,
  normals 2^-6 .. 448); the sign bit is kept, so ``-0`` and negatives that round to zero give 0x80.  A block whose
  exponent clamps at -127 (``0 < amax < 2^-119``) is scaled by 2^127 like any other: nothing is flushed;
* the rule never saturates: ``|v * 2^-X| <= 448`` is asserted for every element, not clamped;
* non-finite inputs are outside the contract: every entry point raises on them.

Two input rules: ``direct`` takes bf16 or f32 values as they are; ``via_bf16`` rounds f32 to bf16 (nearest even)
first and also returns that bf16 copy.

Everything works on integers: values are f32 bit patterns held in int64 tensors (a bf16 pattern is widened by
``<< 16``), decoded into sign, an integer significand M and an exponent E with ``|v| = M * 2^E``; subnormals take
their leading bit from M.  There is no float multiply, no ``frexp`` / ``ldexp`` and no float8 cast in the rule.
``quantize_naive`` states the same rule a second time, one element at a time, in ``fractions.Fraction``
arithmetic against the enumerated e4m3 grid; tests/test_mx_oracle.py holds the two against each other.

Inputs (deterministic, no RNG):

* ``bf16_sweep()``: 49 715 blocks = 1 590 880 bf16 elements.  For each of 64 block maxima ``a = m * 2^k`` (m in
  1, 1.75, 1.7578125, 1.9921875; k in ``SWEEP_K``; all 64 are finite, so none is dropped) every finite bf16
  pattern of magnitude <= a, both signs and both zeros, 31 to a block beside one element of magnitude a whose
  sign alternates and whose slot cycles through the 32 positions; an all-zero and an all-negative-zero block
  close the stream.  bf16 denormals are part of it.
* ``f32_set()``: 319 blocks = 10 208 f32 elements: around every e4m3 rounding midpoint at X in -126, -20, 0, 100
  (the midpoint and +-1, +-2 f32 ulps, both signs), the values one f32 ulp to either side of the bf16 rounding midpoints next to
  an e4m3 midpoint (the double-rounding cases of ``via_bf16``), and block maxima ``1.75 * 2^k * (1 +- 2^-23)``.
  Building it asserts that ``direct`` and ``via_bf16`` differ somewhere on it.
"""
from fractions import Fraction

import torch

BLOCK = 32
I64 = torch.int64
SWEEP_M = (0x00, 0x60, 0x61, 0x7F)       # bf16 mantissa fields of 1, 1.75, 1.7578125, 1.9921875
SWEEP_K = (-126, -125, -122, -120, -119, -118, -117, -110, -20, -1, 0, 8, 60, 119, 126, 127)
F32_X = (-126, -20, 0, 100)
GUARD = 0xA5


# ============================================================================ the rule, vectorised
def _finite(bits):
    if bool((((bits >> 23) & 0xFF) == 0xFF).any()):
        raise ValueError("non-finite input: outside the MX quantisation contract")


def _bitlen(m):
    """Number of significant bits of 0 <= m < 2^40 (0 for 0)."""
    n = torch.zeros_like(m)
    for b in range(40):
        n = n + (m >= (1 << b)).to(I64)
    return n


def _decode(bits):
    """(sign, M, E) of f32 patterns: |v| = M * 2^E exactly."""
    sign = (bits >> 31) & 1
    ef, mf = (bits >> 23) & 0xFF, bits & 0x7FFFFF
    M = torch.where(ef > 0, mf | 0x800000, mf)
    E = torch.where(ef > 0, ef - 150, torch.full_like(ef, -149))
    return sign, M, E


def block_exponent(bits):
    """X [...] of blocks ``bits`` [..., 32] (f32 patterns)."""
    mag = (bits & 0x7FFFFFFF).amax(-1)          # magnitudes order like their patterns
    _, M, E = _decode(mag)
    bl = _bitlen(M)
    fl = bl - 1 + E                              # floor(log2 amax) (for amax > 0)
    norm = M << (24 - bl).clamp(min=0)           # leading bit at 2^23
    x = fl - 8 + (norm > 0xE00000).to(I64)       # 1.75 * 2^23
    x = x.clamp(-127, 127)
    return torch.where(M > 0, x, torch.full_like(x, -127))


def element_bytes(bits, X):
    """e4m3fn bytes of f32 patterns ``bits`` [..., 32] divided by 2^X (``X`` [...]): RNE, sign kept, no clamp."""
    sign, M, E = _decode(bits)
    sh = E - X[..., None] + 9                    # |v| 2^-X = M 2^sh in units of the subnormal step 2^-9
    p = _bitlen(M) - 1 + sh                      # leading bit of that, in units
    t = (p - 3).clamp(min=0)                     # log2 of the grid step there, in units
    up = (sh - t).clamp(0, 30)
    r = (t - sh).clamp(0, 30)                    # (M < 2^24: every shift of 25 or more gives 0, like 30)
    big = (M > 0) & (sh - t > 30)
    n = (M << up) >> r
    rem = (M << up) & ((1 << r) - 1)
    half = torch.where(r > 0, 1 << (r - 1).clamp(min=0), torch.zeros_like(r))
    n = n + ((r > 0) & ((rem > half) | ((rem == half) & ((n & 1) == 1)))).to(I64)
    w = n << t.clamp(max=30)                     # the rounded value in units of 2^-9
    if bool(big.any()) or bool((w > 448 * 512).any()):
        raise AssertionError("an element exceeds 448 after scaling: the rule promised no saturation")
    pw = _bitlen(w) - 1
    byte = torch.where(w < 8, w, ((pw - 2) << 3) | ((w >> (pw - 3).clamp(min=0)) & 7))
    return (byte | (sign << 7)).to(torch.uint8)


def round_bf16(bits):
    """bf16 patterns (int64, 16 bits) of f32 patterns, round to nearest even."""
    _finite(bits)
    b = (bits + 0x7FFF + ((bits >> 16) & 1)) >> 16
    _finite(b << 16)
    return b


def quantize(bits, rule="direct"):
    """``bits`` [..., K] f32 patterns (int64), K % 32 == 0 -> (e4m3 bytes uint8 [..., K], scale bytes uint8
    [..., K/32]) and, for ``rule="via_bf16"``, the bf16 copy's patterns (int64 [..., K]) as a third result."""
    assert rule in ("direct", "via_bf16") and bits.dtype == I64 and bits.shape[-1] % BLOCK == 0
    _finite(bits)
    xb = None
    if rule == "via_bf16":
        xb = round_bf16(bits)
        bits = xb << 16
    blk = bits.reshape(*bits.shape[:-1], bits.shape[-1] // BLOCK, BLOCK)
    X = block_exponent(blk)
    q = element_bytes(blk, X).reshape(bits.shape)
    s = (X + 127).to(torch.uint8)
    return (q, s) if xb is None else (q, s, xb)


# ============================================================================ the rule again, naively
def _frac(b):
    """The value of one f32 pattern as a Fraction."""
    ef, mf = (b >> 23) & 0xFF, b & 0x7FFFFF
    if ef == 0xFF:
        raise ValueError("non-finite input: outside the MX quantisation contract")
    mag = Fraction(mf, 1 << 149) if ef == 0 else Fraction((1 << 23) | mf, 1 << 23) * Fraction(2) ** (ef - 127)
    return -mag if b >> 31 else mag


def _e4m3_grid():
    g = []
    for byte in range(0x7F):
        e, m = byte >> 3, byte & 7
        g.append(Fraction(m, 512) if e == 0 else Fraction(8 + m, 8) * Fraction(2) ** (e - 7))
    return g


_GRID = _e4m3_grid()


def quantize_naive(block, rule="direct"):
    """One block (32 f32 patterns as Python ints) -> (32 bytes, scale byte[, 32 bf16 patterns])."""
    assert len(block) == BLOCK
    xb = None
    if rule == "via_bf16":
        xb = []
        for b in block:
            _frac(b)
            lo, hi = b & ~0xFFFF, (b & ~0xFFFF) + 0x10000       # the bf16 neighbours, by magnitude
            d = 2 * (b & 0xFFFF)
            r = lo if d < 0x10000 else hi if d > 0x10000 else (lo if not (lo >> 16) & 1 else hi)
            _frac(r)
            xb.append(r >> 16)
        block = [r << 16 for r in xb]
    vals = [_frac(b) for b in block]
    amax = max(abs(v) for v in vals)
    if amax == 0:
        X = -127
    else:
        fl = 0
        while Fraction(2) ** fl > amax:
            fl -= 1
        while Fraction(2) ** (fl + 1) <= amax:
            fl += 1
        X = max(-127, min(127, fl - 8 + (1 if amax > Fraction(7, 4) * Fraction(2) ** fl else 0)))
    scale = Fraction(2) ** X
    out = []
    for b, v in zip(block, vals):
        u = abs(v) / scale
        assert u <= 448, "an element exceeds 448 after scaling"
        lo, hi = 0, len(_GRID) - 1                  # the grid points around u
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if _GRID[mid] <= u:
                lo = mid
            else:
                hi = mid
        dl, dh = u - _GRID[lo], _GRID[hi] - u
        byte = lo if dl < dh else hi if dh < dl else (lo if lo % 2 == 0 else hi)
        out.append(byte | ((b >> 31) << 7))
    return (out, X + 127) if xb is None else (out, X + 127, xb)


def dequantize_exact(q, s):
    """Fractions ``q * 2^X`` of bytes ``q`` (list) under scale byte ``s``; the sign of a zero is dropped."""
    sc = Fraction(2) ** (s - 127)
    return [(-1 if b & 0x80 else 1) * _GRID[b & 0x7F] * sc for b in q]


def f32_bits_of(fr):
    """The f32 magnitude pattern of |fr| (a Fraction) if that is an f32 number, else None."""
    n, d = abs(fr).numerator, abs(fr).denominator
    if n == 0:
        return 0
    if d & (d - 1):
        return None
    e = max(n.bit_length() - d.bit_length(), -126)       # floor(log2), or the subnormal exponent
    m = Fraction(n, d) / Fraction(2) ** (e - 23)          # the significand in units of 2^(e - 23)
    if e > 127 or m.denominator != 1:
        return None
    m = int(m)
    return ((e + 127) << 23) | (m & 0x7FFFFF) if m >= (1 << 23) else m


# ============================================================================ inputs
def _pack_blocks(vals, amax_bits, start, sign_bit):
    """``vals`` (int64 patterns) 31 to a block beside one element ``amax_bits`` whose sign (bit ``sign_bit``)
    alternates and whose slot cycles from ``start``; the last block is filled up with zeros.  -> [nb][32]"""
    nb = -(-vals.numel() // 31)
    body = torch.zeros(nb * 31, dtype=I64)
    body[:vals.numel()] = vals
    body = body.reshape(nb, 31)
    idx = torch.arange(start, start + nb, dtype=I64)
    slot, sgn = idx % BLOCK, idx % 2
    out = torch.empty(nb, BLOCK, dtype=I64)
    col = torch.arange(BLOCK, dtype=I64)[None, :]
    src = (col - (col > slot[:, None]).to(I64)).clamp(max=30)
    out[:] = torch.gather(body, 1, src)
    out[torch.arange(nb), slot] = amax_bits | (sgn << sign_bit)
    return out


_CACHE = {}


def sweep_maxima():
    """The bf16 magnitude patterns of the sweep's block maxima, in stream order."""
    out = []
    for k in SWEEP_K:
        for m in SWEEP_M:
            a = ((k + 127) << 7) | m
            if (a >> 7) & 0xFF != 0xFF:             # (finite: all 64 are)
                out.append(a)
    return out


def sweep_blocks_for(a, start=0):
    """The sweep's blocks [nb][32] (bf16 patterns, int64) for the one block maximum ``a`` (a bf16 magnitude
    pattern): every pattern of magnitude <= a, both signs, both zeros."""
    mags = torch.arange(a + 1, dtype=I64)
    vals = torch.stack([mags, mags | 0x8000], 1).reshape(-1)
    return _pack_blocks(vals, a, start, 15)


def bf16_sweep():
    """[nb][32] bf16 patterns (int64): the exhaustive sweep of the module docstring."""
    if "sweep" not in _CACHE:
        parts, n = [], 0
        for a in sweep_maxima():
            parts.append(sweep_blocks_for(a, n))
            n += parts[-1].shape[0]
        parts.append(torch.zeros(1, BLOCK, dtype=I64))
        parts.append(torch.full((1, BLOCK), 0x8000, dtype=I64))
        _CACHE["sweep"] = torch.cat(parts)
    return _CACHE["sweep"]


def _bits_pow2(n, e):
    """The f32 pattern of n * 2^e (n a positive int of at most 24 bits), which must be an f32 number."""
    b = f32_bits_of(Fraction(n) * Fraction(2) ** e)
    assert b is not None
    return b


def f32_set():
    """[nb][32] f32 patterns (int64): the tie, double-rounding and threshold cases of the module docstring."""
    if "f32" in _CACHE:
        return _CACHE["f32"]
    units = []                                  # the non-negative e4m3 values in units of 2^-9
    for byte in range(0x7F):
        e, m = byte >> 3, byte & 7
        units.append(m if e == 0 else (8 + m) << (e - 1))
    parts, n = [], 0
    for X in F32_X:
        vals = []
        for lo, hi in zip(units, units[1:]):
            B = _bits_pow2(lo + hi, X - 10)     # the midpoint, times 2^X
            near = [B + d for d in (-2, -1, 0, 1, 2)]
            if B & 0xFFFF == 0 and B >= 0x8000:  # the bf16 rounding midpoints on either side of it
                near += [B + h + d for h in (-0x8000, 0x8000) for d in (-1, 1)]
            vals += [v | s for v in near for s in (0, 1 << 31)]
        top = _bits_pow2(448, X)                # 1.75 * 2^(X + 8): the largest maximum with exponent X
        assert max(v & 0x7FFFFFFF for v in vals) < top
        parts.append(_pack_blocks(torch.tensor(vals, dtype=I64), top, n, 31))
        n += parts[-1].shape[0]
    for k in SWEEP_K:                           # maxima one f32 ulp to either side of the 1.75 threshold
        t = ((k + 127) << 23) | 0x600000
        for a in (t - 1, t + 1):
            fill = torch.tensor([(a - 0x10000 * (i + 1)) | ((i & 1) << 31) for i in range(31)], dtype=I64)
            parts.append(_pack_blocks(fill, a, n, 31))
            n += 1
    blocks = torch.cat(parts)
    d, v = quantize(blocks, "direct"), quantize(blocks, "via_bf16")
    assert not torch.equal(d[0], v[0]) and not torch.equal(d[1], v[1]), \
        "direct and via_bf16 agree on the whole f32 set: it could not tell a kernel's input rule"
    _CACHE["f32"] = blocks
    return blocks


# ============================================================================ shapes
def pad_blocks(blocks, multiple):
    """``blocks`` [nb][32] padded with all-zero blocks to a multiple of ``multiple`` blocks."""
    nb = blocks.shape[0]
    pad = -nb % multiple
    return torch.cat([blocks, torch.zeros(pad, BLOCK, dtype=blocks.dtype)]) if pad else blocks


def as_rows(blocks, K, rows_multiple=1):
    """The block stream as a row-blocked operand [R][K] (K % 32 == 0), R a multiple of ``rows_multiple``."""
    per = K // BLOCK
    return pad_blocks(blocks, per * rows_multiple).reshape(-1, K)


def as_cols(blocks, N, k_multiple=32):
    """The block stream as a column-blocked operand [K][N]: column n's K/32 blocks are consecutive blocks of the
    stream, so ``as_cols(...).t()`` is the row-blocked [N][K] the outputs are compared in."""
    kb = k_multiple // BLOCK
    b = pad_blocks(blocks, N * kb)
    return b.reshape(N, -1).t().contiguous()


def as_cache(blocks, B, Hkv):
    """The block stream as cache rows (B, T, Hkv, 64): two blocks per head row."""
    b = pad_blocks(blocks, 2 * Hkv * B)
    return b.reshape(B, -1, Hkv, 64)


def bf16_tensor(bits):
    """A torch.bfloat16 tensor with the patterns ``bits`` (int64, 16 bits)."""
    b = bits & 0xFFFF
    return torch.where(b >= 0x8000, b - 0x10000, b).to(torch.int16).view(torch.bfloat16)


def f32_tensor(bits):
    """A torch.float32 tensor with the patterns ``bits`` (int64, 32 bits)."""
    b = bits & 0xFFFFFFFF
    return torch.where(b >= (1 << 31), b - (1 << 32), b).to(torch.int32).view(torch.float32)


def bits_of(t):
    """The patterns of a bf16 / f32 tensor as int64, a bf16 one widened to f32's."""
    if t.dtype == torch.bfloat16:
        return (t.view(torch.int16).to(I64) & 0xFFFF) << 16
    assert t.dtype == torch.float32
    return t.view(torch.int32).to(I64) & 0xFFFFFFFF


def first_difference(name, got, want, inputs):
    """None when ``got`` equals ``want`` (uint8 [nb][w]); else a message with the first differing block's input
    patterns, the expected bytes and the bytes received."""
    got, want = got.reshape(want.shape), want
    if torch.equal(got, want):
        return None
    bad = (got != want).reshape(want.shape[0], -1).any(1).nonzero()
    i = int(bad[0])
    return (f"{name}: {bad.numel()} of {want.shape[0]} blocks differ; first block {i}\n"
            f"  input bits {[hex(v) for v in inputs[i].tolist()]}\n"
            f"  expected   {[hex(v) for v in want[i].tolist()]}\n"
            f"  received   {[hex(v) for v in got[i].tolist()]}")
