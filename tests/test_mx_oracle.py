"""tests/mx_oracle.py held against itself, and the host MX quantiser held against it (CPU).

The oracle's vectorised integer form and its naive ``fractions.Fraction`` form are two independent statements
of one rule; they must agree on every finite bf16 pattern and on the f32 tie / double-rounding set.  Then
``fp8.quantize_mx_ref`` / ``kernels._mx_bytes`` -- what CPU devices run and what the cache tests compare against
-- must give the oracle's bytes on the whole sweep and the whole f32 set, and ``dequantize_mx_ref`` the exact
``q * 2^X``.  Every comparison is bit equality."""
from fractions import Fraction

import pytest
import torch

import mx_oracle as O


def _naive_all(blocks, rule):
    out = [O.quantize_naive(b, rule) for b in blocks.tolist()]
    q = torch.tensor([o[0] for o in out], dtype=torch.uint8)
    s = torch.tensor([o[1] for o in out], dtype=torch.uint8)
    xb = torch.tensor([o[2] for o in out], dtype=torch.int64) if rule == "via_bf16" else None
    return q, s, xb


def _same(name, blocks, rule):
    got = O.quantize(blocks, rule)
    q, s, xb = _naive_all(blocks, rule)
    for what, g, w in (("bytes", got[0], q), ("scales", got[1][:, None], s[:, None])):
        msg = O.first_difference(f"{name} {rule} {what}: vectorised (received) vs naive (expected)", g, w, blocks)
        assert msg is None, msg
    if xb is not None:
        assert torch.equal(got[2], xb), f"{name}: bf16 copies differ"


# (max pattern, what it covers): the largest finite bf16 -- every one of the 65 280 finite patterns, X = 120;
# 1.75 -- the threshold, X = -8; 2^-120 -- the clamp, X = -127, where bf16 denormals reach non-zero bytes
NAIVE_MAXIMA = [0x7F7F, 0x3FE0, 0x0380]


@pytest.mark.parametrize("a", NAIVE_MAXIMA, ids=[hex(a) for a in NAIVE_MAXIMA])
def test_two_formulations_agree_on_every_bf16_pattern(a):
    assert a in O.sweep_maxima()
    blocks = O.sweep_blocks_for(a)
    if a == 0x7F7F:
        seen = torch.zeros(1 << 16, dtype=torch.bool)
        seen[blocks.reshape(-1)] = True
        assert int(seen.sum()) == 65280 and not seen[0x7F80:0x8000].any() and not seen[0xFF80:].any()
    _same(hex(a), blocks << 16, "direct")


def test_two_formulations_agree_on_the_f32_set():
    f = O.f32_set()
    _same("f32_set", f, "direct")
    _same("f32_set", f, "via_bf16")
    zeros = torch.cat([torch.zeros(1, 32, dtype=torch.int64), torch.full((1, 32), 1 << 31, dtype=torch.int64)])
    _same("zeros", zeros, "direct")


def test_known_answers():
    """Bytes worked out by hand: the anchor outside both formulations."""
    def one(vals):       # f32 patterns, zero-filled to a block
        q, s = O.quantize(torch.tensor([vals + [0] * (32 - len(vals))], dtype=torch.int64))
        return q[0, :len(vals)].tolist(), int(s[0, 0])
    assert one([0x3F80 << 16]) == ([0x78], 119)                      # 1.0 -> 256 * 2^-8
    assert one([0x3FE0 << 16]) == ([0x7E], 119)                      # 1.75 -> 448 * 2^-8: no bump
    assert one([0x3FE1 << 16]) == ([0x76], 120)                      # its bf16 successor -> RNE(225) = 224 * 2^-7
    assert one([0x3FE00001]) == ([0x76], 120)                        # one f32 ulp above 1.75 bumps too
    assert one([0x0380 << 16]) == ([0x70], 0)                        # 2^-120: the clamp scales by 2^127 -> 128
    assert one([0x0001 << 16]) == ([0x08], 0)                        # the smallest bf16 denormal 2^-133 -> 2^-6
    assert one([0x8000 << 16, 0x3F80 << 16]) == ([0x80, 0x78], 119)  # -0 keeps its sign
    # ties at X = 0 (block max 256 = 0x4380): 2^-10 -> 0 (even), 3 * 2^-10 -> 2 * 2^-9 (even), sign kept
    q, s = one([0x4380 << 16, 0x3A800000, 0xBA800000, 0x3B400000, 0x3A800001])
    assert (q, s) == ([0x78, 0x00, 0x80, 0x02, 0x01], 127)
    # 17 sits between 16 (0x58) and 18 (0x59): tie to the even mantissa
    assert one([0x4380 << 16, 0x41880000, 0x41980000])[0] == [0x78, 0x58, 0x5A]


def test_sweep_layout():
    sw = O.bf16_sweep()
    assert sw.shape == (49715, 32) and sw.numel() == 1590880
    assert sw[-2].eq(0).all() and sw[-1].eq(0x8000).all()
    mag = sw & 0x7FFF
    top = mag.amax(1)
    assert set(top[:-2].tolist()) == set(O.sweep_maxima()) and len(O.sweep_maxima()) == 64
    idx = torch.arange(sw.shape[0] - 2)
    at = sw[idx, idx % 32]
    assert torch.equal(at & 0x7FFF, top[:-2]) and torch.equal(at >> 15, idx % 2)     # slot cycles, sign alternates
    seen = torch.zeros(1 << 16, dtype=torch.bool)
    seen[sw.reshape(-1)] = True
    assert int(seen.sum()) == 65280
    s = O.quantize(sw << 16)[1]
    assert int(s.min()) == 0 and int(s.max()) == 247        # both ends the rule can reach: X = -127 .. 120


def test_non_finite_inputs_raise():
    for bad in (0x7F800000, 0xFF800000, 0x7FC00000, 0x7F7FFFFF):     # the last: finite, rounds to a bf16 inf
        blk = torch.zeros(1, 32, dtype=torch.int64)
        blk[0, 5] = bad
        with pytest.raises(ValueError):
            O.quantize(blk, "via_bf16")
        with pytest.raises(ValueError):
            O.quantize_naive(blk[0].tolist(), "via_bf16")
        if bad != 0x7F7FFFFF:
            with pytest.raises(ValueError):
                O.quantize(blk)
            with pytest.raises(ValueError):
                O.quantize_naive(blk[0].tolist())


def test_shape_helpers():
    sw = O.bf16_sweep()[:100]
    r = O.as_rows(sw, 128, 8)
    assert r.shape[1] == 128 and r.shape[0] % 8 == 0 and torch.equal(r.reshape(-1, 32)[:100], sw)
    assert r.reshape(-1, 32)[100:].eq(0).all()
    c = O.as_cols(sw, 72, 64)
    assert c.shape[1] == 72 and c.shape[0] % 64 == 0
    assert torch.equal(c.t().reshape(-1, 32)[:100], sw)
    k = O.as_cache(sw, 2, 3)
    assert k.shape[0] == 2 and k.shape[2:] == (3, 64) and torch.equal(k.reshape(-1, 32)[:100], sw)


# ----------------------------------------------------------------------------- the host quantiser
def _host(x):
    from learning_jax_sharding_amd.ops.fp8 import quantize_mx_ref
    from learning_jax_sharding_amd.ops.kernels import _mx_bytes
    q, ex = quantize_mx_ref(x)
    bq, bs = _mx_bytes(x)
    assert bq.dtype == torch.uint8 and bs.dtype == torch.uint8
    assert torch.equal(q.view(torch.uint8), bq) and torch.equal((ex + 127).to(torch.uint8), bs)
    return bq, bs


def test_host_reference_matches_oracle_on_the_bf16_sweep():
    sw = O.bf16_sweep()
    x = O.bf16_tensor(sw)
    assert torch.equal(O.bits_of(x), sw << 16)
    want_q, want_s = O.quantize(sw << 16)
    q, s = _host(x)
    for what, g, w in (("bytes", q, want_q), ("scales", s, want_s)):
        msg = O.first_difference(f"quantize_mx_ref bf16 {what}", g, w, sw)
        assert msg is None, msg
    q, s = _host(x.float())                                   # the same values as f32
    assert torch.equal(q, want_q) and torch.equal(s, want_s)


def test_host_reference_matches_oracle_on_the_f32_set():
    f = O.f32_set()
    x = O.f32_tensor(f)
    assert torch.equal(O.bits_of(x), f)
    want_q, want_s = O.quantize(f, "direct")
    q, s = _host(x)
    for what, g, w in (("bytes", q, want_q), ("scales", s, want_s)):
        msg = O.first_difference(f"quantize_mx_ref f32 {what}", g, w, f)
        assert msg is None, msg
    vq, vs, xb = O.quantize(f, "via_bf16")
    xb_t = x.to(torch.bfloat16)
    assert torch.equal(O.bits_of(xb_t), xb << 16)             # torch's bf16 cast is the oracle's rounding
    q, s = _host(xb_t)
    assert torch.equal(q, vq) and torch.equal(s, vs)


def test_dequantize_reference_is_exact():
    """``dequantize_mx_ref`` of every (element byte, scale byte) the rule can produce equals ``q * 2^X`` exactly
    wherever that is an f32 number -- a zero scale byte means 2^-127, not zero."""
    from learning_jax_sharding_amd.ops.fp8 import dequantize_mx_ref
    bytes_ = [b for b in range(256) if b & 0x7F != 0x7F]      # (0x7F / 0xFF are e4m3fn's NaN: never produced)
    scales = list(range(255))                                 # (255 is e8m0's NaN: never produced)
    q = torch.tensor(bytes_ * 8, dtype=torch.uint8)[:32 * (len(bytes_) * 8 // 32)]
    n = q.numel()
    qq = q.repeat(len(scales), 1)                             # [scale][n]
    ex = torch.tensor(scales, dtype=torch.int32)[:, None].expand(-1, n // 32) - 127
    d = dequantize_mx_ref(qq.view(torch.float8_e4m3fn), ex.contiguous())
    got = O.bits_of(d)
    checked = 0
    for si, s in enumerate(scales):
        exact = O.dequantize_exact(bytes_, s)
        for bi, (b, fr) in enumerate(zip(bytes_, exact)):
            mag = O.f32_bits_of(fr)
            if mag is None:
                continue
            want = mag | ((b >> 7) << 31)
            assert int(got[si, bi]) == want, (hex(b), s, hex(int(got[si, bi])), hex(want))
            checked += 1
    assert checked > 60000
    assert int(got[0, bytes_.index(0x70)]) == 0x03800000      # 128 * 2^-127 = 2^-120
    assert int(got[0, bytes_.index(0x01)]) == 0x00002000      # 2^-9 * 2^-127 = 2^-136, an f32 denormal
