"""Every MX-fp8 quantiser of the library against the integer oracle of tests/mx_oracle.py, bit for bit, on a
real MI355X.

"Quantise a block of 32" is implemented many times over on two instruction paths (multiply + convert, and the
gfx950 scaled conversion on an integer amax).  Each test below runs ONE kernel instance on the exhaustive bf16
sweep (and, where the instance reads f32, on the f32 tie / double-rounding set), at the smallest shape that
still selects the instance and holds the sweep in one launch, and asserts

* uint8 equality of the element bytes and of the scale bytes with the oracle's (on failure: the first differing
  block's input bits, the expected and the received bytes),
* through ``hip.launch_log()`` the record of the instance that was meant to run,
* that the guard bytes (0xA5) behind every output are untouched.

Operands whose blocks run along columns get the sweep in that layout (``as_cols``); kernels with a row-blocked
and a column-blocked output run once per layout, and every output of every run is compared (the oracle is
evaluated on the operand as the output blocks it).  Nothing here has a tolerance."""

import pytest
import torch

import mx_oracle as O

pytestmark = pytest.mark.gpu

BF16, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
GUARD_BYTES = 256


def _mods():
    from learning_jax_sharding_amd.ops import fp8, hip
    return hip, fp8


# ----------------------------------------------------------------------------- inputs and the oracle, once
_MEMO = {}


def _memo(key, make):
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


def _stream(kind):
    """The block stream [nb][32] as f32 patterns: ``bf16`` the sweep, ``f32`` the f32 set followed by the sweep."""
    if kind == "bf16":
        return _memo("stream bf16", lambda: O.bf16_sweep() << 16)
    return _memo("stream f32", lambda: torch.cat([O.f32_set(), O.bf16_sweep() << 16]))


def _want(key, bits, rule="direct"):
    """The oracle on ``bits`` [R][K] (f32 patterns), memoised under ``key``: (q [nb][32], s [nb][1][, xb [R][K]])."""
    def make():
        r = O.quantize(bits, rule)
        return (r[0].reshape(-1, 32), r[1].reshape(-1, 1)) + tuple(r[2:])
    return _memo(("want", key, rule), make)


def _tensor(bits, dtype):
    """The GPU tensor with these f32 patterns (bf16: their upper halves, which must be all of them)."""
    if dtype == BF16:
        assert bool(((bits & 0xFFFF) == 0).all())
        return O.bf16_tensor(bits >> 16).cuda()
    return O.f32_tensor(bits).cuda()


def _strided(x, pad=8):
    """``x`` [R][K] as a view of rows of K + pad elements (the pad holds a large finite value no block may see)."""
    big = torch.full((x.shape[0], x.shape[1] + pad), 3.0e38, dtype=x.dtype, device=x.device)
    big[:, :x.shape[1]] = x
    v = big[:, :x.shape[1]]
    assert not v.is_contiguous() and v.data_ptr() % 16 == 0
    return v


class Guarded:
    """Output buffers with GUARD_BYTES of 0xA5 behind (and in) each, and the check that they stayed."""

    def __init__(self):
        self.bufs = []

    def new(self, shape, dtype=U8, fill=O.GUARD):
        n = 1
        for d in shape:
            n *= d
        nbytes = n * torch.empty((), dtype=dtype).element_size()
        pad = -nbytes % 16
        raw = torch.full((nbytes + pad + GUARD_BYTES,), O.GUARD, dtype=U8, device="cuda")
        if fill != O.GUARD:
            raw[:nbytes] = fill
        self.bufs.append((raw, nbytes))
        return raw[:nbytes].view(dtype).view(shape)

    def check(self, name):
        for raw, nbytes in self.bufs:
            assert bool((raw[nbytes:] == O.GUARD).all()), f"{name}: guard bytes behind an output were written"


def _same(name, got_q, got_s, want, inputs):
    """Element bytes and scale bytes against the oracle's, block by block."""
    torch.cuda.synchronize()
    want_q, want_s = want[0], want[1]
    blocks = inputs.reshape(-1, 32)
    for what, g, w in (("element bytes", got_q.cpu().reshape(-1, 32), want_q),
                       ("scale bytes", got_s.cpu().reshape(-1, 1), want_s)):
        assert g.dtype == U8 and g.shape == w.shape, (name, what, g.shape, w.shape)
        msg = O.first_difference(f"{name}: {what}", g, w, blocks)
        assert msg is None, msg


def _names(log):
    return [r["name"] for r in log]


# ----------------------------------------------------------------------------- quant_mx_rows
@pytest.mark.parametrize("strided", [False, True], ids=["contig", "ld>K"])
def test_quant_rows_bf16(strided):
    hip, F = _mods()
    K = 128
    bits = O.as_rows(_stream("bf16"), K)
    x = _tensor(bits, BF16)
    x = _strided(x) if strided else x
    G = Guarded()
    q, s = G.new(bits.shape), G.new((bits.shape[0], K // 32))
    with hip.launch_log() as log:
        F.quant_rows(x, out=(q, s))
    assert _names(log) == ["quant_mx_rows"], log
    _same("quant_mx_rows bf16", q, s, _want("rows128 bf16", bits), bits)
    G.check("quant_mx_rows bf16")


@pytest.mark.parametrize("with_xb", [False, True], ids=["noxb", "xb"])
@pytest.mark.parametrize("strided", [False, True], ids=["contig", "ld>K"])
def test_quant_rows_f32(strided, with_xb):
    """Rule ``direct`` on the f32 set and the widened sweep; ``xb`` is the oracle's bf16 rounding of the input."""
    hip, F = _mods()
    K = 128
    bits = O.as_rows(_stream("f32"), K)
    x = _tensor(bits, F32)
    x = _strided(x) if strided else x
    G = Guarded()
    q, s = G.new(bits.shape), G.new((bits.shape[0], K // 32))
    xb = G.new(bits.shape, BF16) if with_xb else None
    with hip.launch_log() as log:
        F.quant_rows(x, out=(q, s), xb=xb)
    assert _names(log) == ["quant_mx_rows"], log
    _same("quant_mx_rows f32", q, s, _want("rows128 f32", bits), bits)
    if with_xb:
        want_xb = _memo("rows128 f32 xb", lambda: O.round_bf16(bits))
        assert torch.equal(O.bits_of(xb.cpu()) >> 16, want_xb), "quant_mx_rows: xb is not the input rounded to bf16"
    G.check("quant_mx_rows f32")


# ----------------------------------------------------------------------------- quant_mx_cols
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_quant_cols_generic(dtype):
    """N = 72 is no multiple of 64 (and an f32 input never tiles): one thread per block."""
    hip, F = _mods()
    N, kind = 72, "bf16" if dtype == BF16 else "f32"
    w_bits = O.as_cols(_stream(kind), N)                      # [K][N]
    K = w_bits.shape[0]
    G = Guarded()
    q, s = G.new((N, K)), G.new((N, K // 32))
    with hip.launch_log() as log:
        F.quant_cols(_tensor(w_bits, dtype), out=(q, s))
    assert _names(log) == ["quant_mx_cols<generic>"], log
    rows = w_bits.t().contiguous()
    _same(f"quant_mx_cols<generic> {kind}", q, s, _want(f"cols72 {kind}", rows), rows)
    G.check("quant_mx_cols<generic>")


@pytest.mark.parametrize("strided", [False, True], ids=["contig", "ld>N"])
def test_quant_cols_tiled(strided):
    hip, F = _mods()
    N = 64
    w_bits = O.as_cols(_stream("bf16"), N, 128)
    K = w_bits.shape[0]
    assert K % 128 == 0
    w = _tensor(w_bits, BF16)
    w = _strided(w) if strided else w
    G = Guarded()
    q, s = G.new((N, K)), G.new((N, K // 32))
    with hip.launch_log() as log:
        F.quant_cols(w, out=(q, s))
    assert _names(log) == ["quant_mx_cols<tiled>"] and log[0]["grid"] == (1, K // 128, 1), log
    rows = w_bits.t().contiguous()
    _same("quant_mx_cols<tiled>", q, s, _want("cols64 bf16", rows), rows)
    G.check("quant_mx_cols<tiled>")


# ----------------------------------------------------------------------------- quant_mx_both
def _both(kind, layout):
    """[T][M] patterns, M = 64, T % 128 == 0, with the stream along the rows' or along the columns' blocks."""
    s = _stream(kind)
    return O.as_rows(s, 64, 128) if layout == "rows" else O.as_cols(s, 64, 128)


@pytest.mark.parametrize("layout", ["rows", "cols"])
@pytest.mark.parametrize("kind", ["bf16", "f32"])
def test_quant_both(kind, layout):
    """Both outputs of one pass, each against the oracle; the f32 instance rounds to bf16 first (``via_bf16``) and
    its ``xb`` is that copy."""
    hip, F = _mods()
    bits = _both(kind, layout)
    T, M = bits.shape
    f32 = kind == "f32"
    rule = "via_bf16" if f32 else "direct"
    x = _tensor(bits, F32 if f32 else BF16)
    G = Guarded()
    q, s, qT, sT = G.new((T, M)), G.new((T, M // 32)), G.new((M, T)), G.new((M, T // 32))
    xb = G.new((T, M), BF16) if f32 else None
    with hip.launch_log() as log:
        rc = F._lib().ljs_quant_mx_both(hip._p(x), x.stride(0), T, M, hip._p(qT), hip._p(sT), hip._p(q), hip._p(s),
                                        hip._p(xb) if f32 else None, hip._stream(x))
    assert rc == 0 and _names(log) == [f"quant_mx_both<{kind}>"], (rc, log)
    colsb = bits.t().contiguous()
    _same(f"quant_mx_both<{kind}> {layout}: row-blocked", q, s, _want(f"both {kind} {layout} r", bits, rule), bits)
    _same(f"quant_mx_both<{kind}> {layout}: transposed", qT, sT, _want(f"both {kind} {layout} c", colsb, rule), colsb)
    if f32:
        want_xb = _want(f"both {kind} {layout} r", bits, rule)[2]
        assert torch.equal(O.bits_of(xb.cpu()) >> 16, want_xb), "quant_mx_both<f32>: xb is not the bf16 rounding"
    G.check(f"quant_mx_both<{kind}>")


# ----------------------------------------------------------------------------- bcast_scalar_mx / mx2
def _scalars():
    """bf16 magnitude patterns of g: the four sweep mantissas at every fourth exponent field and at the lowest
    and the highest eight (the denormal field 0 included), mantissa-major."""
    fields = sorted(set(range(0, 255, 4)) | set(range(8)) | set(range(247, 255)))
    return [(f << 7) | m for m in O.SWEEP_M for f in fields if (f << 7) | m]


def test_bcast_scalar_mx():
    """One launch per scalar ``g`` (C = 64; C2 = 32 for ``mx2``): ``row`` is bf16(g) and every block holds the
    oracle's bytes of a block of 32 such values.  Sign, the form of g (bf16, or an f32 that is no bf16 number
    and rounds to it) and the kernel alternate from one magnitude to the next; the zeros take every combination.
    The case list (4 mantissas x 76 exponent fields, less the zero pattern) makes 303 + 8 launches."""
    hip, F = _mods()
    L = F._lib()
    cases = []
    for i, a in enumerate(_scalars()):
        cases.append((a | ((i & 1) << 15), bool((i >> 1) & 1), bool((i >> 2) & 1)))
    for z in (0x0000, 0x8000):
        cases += [(z, f32, two) for f32 in (False, True) for two in (False, True)]
    assert len(cases) == 311
    vals = torch.tensor([c[0] for c in cases], dtype=torch.int64)
    want = O.quantize((vals << 16)[:, None].expand(-1, 32).contiguous())
    C1, C2 = 64, 32
    n = len(cases)
    G = Guarded()
    row, q1, s1 = G.new((n, C1), BF16), G.new((n, C1)), G.new((n, C1 // 32))
    q2, s2 = G.new((n, C2)), G.new((n, C2 // 32))
    gs = []
    for i, (pat, f32, two) in enumerate(cases):
        if f32:     # an f32 strictly between bf16 numbers that rounds to ``pat`` (a zero stays a zero)
            g = O.f32_tensor(torch.tensor([(pat << 16) | (0x4000 if pat & 0x7FFF else 0)])).cuda()
        else:
            g = O.bf16_tensor(torch.tensor([pat])).cuda()
        gs.append(g)
        with hip.launch_log() as log:
            if two:
                rc = L.ljs_bcast_scalar_mx2(hip._p(g), int(not f32), C1, hip._p(row[i]), hip._p(q1[i]), hip._p(s1[i]),
                                            C2, hip._p(q2[i]), hip._p(s2[i]), hip._stream(g))
            else:
                rc = L.ljs_bcast_scalar_mx(hip._p(g), int(not f32), C1, hip._p(row[i]), hip._p(q1[i]), hip._p(s1[i]),
                                           hip._stream(g))
        assert rc == 0 and _names(log) == ["bcast_scalar_mx2" if two else "bcast_scalar_mx"], (rc, log, cases[i])
    torch.cuda.synchronize()
    assert torch.equal(O.bits_of(row.cpu()) >> 16, vals[:, None].expand(-1, C1)), "row is not bf16(g)"
    inputs = (vals << 16)[:, None].expand(-1, 32)
    wq, ws = want[0].reshape(-1, 32), want[1].reshape(-1, 1)
    for h in range(C1 // 32):
        _same(f"bcast_scalar_mx row block {h}", q1[:, 32 * h:32 * h + 32].contiguous(), s1[:, h].contiguous(),
              (wq, ws), inputs)
    two = torch.tensor([c[2] for c in cases])
    q2, s2 = q2.cpu(), s2.cpu()
    _same("bcast_scalar_mx2 second row", q2[two], s2[two], (wq[two], ws[two]), inputs[two])
    assert bool((q2[~two] == O.GUARD).all()) and bool((s2[~two] == O.GUARD).all())
    G.check("bcast_scalar_mx")


# ----------------------------------------------------------------------------- kv_append<copy,mx8>
@pytest.mark.parametrize("mode", ["host-base", "lens"])
def test_kv_append_copy_mx8(mode):
    """K is the sweep, V the sweep in reverse block order, two blocks per head row; the cache is pre-filled with
    0xFF and rows that are not written keep it."""
    hip, _ = _mods()
    B, Hkv = 2, 4
    sw = O.bf16_sweep()
    kb, vb = O.as_cache(sw << 16, B, Hkv), O.as_cache(sw.flip(0) << 16, B, Hkv)
    T = kb.shape[1]
    lens = [0, 0] if mode == "host-base" else [3, 1]
    cap = T + 5
    k, v = _tensor(kb, BF16), _tensor(vb, BF16)
    G = Guarded()
    kc, vc = G.new((B, cap, Hkv, 64), fill=0xFF), G.new((B, cap, Hkv, 64), fill=0xFF)
    kcs, vcs = G.new((B, cap, Hkv, 2), fill=0xFF), G.new((B, cap, Hkv, 2), fill=0xFF)
    lt = None if mode == "host-base" else torch.tensor(lens, dtype=torch.int32).cuda()
    with hip.launch_log() as log:
        assert hip.kv_append_q8(k, v, kc, vc, kcs, vcs, lt) is None
    assert _names(log) == ["kv_append<copy,mx8>"], log
    torch.cuda.synchronize()
    wk = _want("cache k", kb.reshape(-1, 64))
    wv = _want("cache v", vb.reshape(-1, 64))
    for name, c, cs, want, bits in (("k", kc, kcs, wk, kb), ("v", vc, vcs, wv, vb)):
        got_q = torch.stack([c[b, lens[b]:lens[b] + T] for b in range(B)])
        got_s = torch.stack([cs[b, lens[b]:lens[b] + T] for b in range(B)])
        _same(f"kv_append<copy,mx8> {mode} {name}", got_q, got_s, want, bits)
        for b in range(B):
            for t in (c, cs):
                assert bool((t[b, :lens[b]] == 0xFF).all()) and bool((t[b, lens[b] + T:] == 0xFF).all()), \
                    f"{name}: a row outside the appended ones was written"
    G.check("kv_append<copy,mx8>")


# ----------------------------------------------------------------------------- MX GEMM epilogue copies
def _res_operand(layout, BM, N):
    s = _stream("bf16")
    return O.as_rows(s, N, BM) if layout == "rows" else O.as_cols(s, N, BM)


@pytest.mark.parametrize("layout", ["rows", "cols"])
@pytest.mark.parametrize("tile", [1282, 2563])
def test_gemm_epilogue_copies(tile, layout):
    """QC and QT of the 4-wave (``tile=1282``: the scaled-conversion QC branch, taken for a bf16 output) and the
    8-wave-per-256-rows (``tile=2563``) kernels on CHOSEN outputs: A is all zero bytes under scale bytes 127, so
    the output is ``+0 + R`` -- R bit for bit, except that IEEE addition turns R's ``-0`` into ``+0``, which is
    asserted as such (so these copies see no negative zero).  N = 128, K = 128, M as many BM-row tiles as hold
    the sweep in one launch; ``rows`` puts the sweep along QC's blocks, ``cols`` along QT's, and both copies are
    compared in both runs."""
    hip, F = _mods()
    N, K = 128, 128
    BM = 128 if tile == 1282 else 256
    r_bits = _res_operand(layout, BM, N)
    M = r_bits.shape[0]
    flags = F.mx_flags(BF16, None, False, BF16, "add", True, True)
    plan = F.gemm_mx_plan(M, N, K, flags, tile)
    assert plan["err"] == 0 and plan["resolved_tile"] == tile and plan["BM"] == BM, plan
    qa, sa = torch.zeros((M, K), dtype=U8).cuda(), torch.full((M, K // 32), 127, dtype=U8).cuda()
    qb, sb = torch.zeros((N, K), dtype=U8).cuda(), torch.full((N, K // 32), 127, dtype=U8).cuda()
    R = _tensor(r_bits, BF16)
    G = Guarded()
    out = G.new((M, N), BF16)
    q, s, qT, sT = G.new((M, N)), G.new((M, N // 32)), G.new((N, M)), G.new((N, M // 32))
    with hip.launch_log() as log:
        F.gemm_mx(qa, sa, qb, sb, M, N, K, out, res=R, res_mode="add", qout=(q, s), qtout=(qT, sT), tile=tile)
    assert _names(log) == [plan["name"]] and log[0]["resolved_tile"] == tile and log[0]["variant"] == plan["fix"], log
    torch.cuda.synchronize()
    o_bits = torch.where(r_bits == 0x80000000, torch.zeros_like(r_bits), r_bits)
    assert torch.equal(O.bits_of(out.cpu()), o_bits), f"{plan['name']}: the output is not 0 + R"
    colsb = o_bits.t().contiguous()
    _same(f"{plan['name']} {layout}: QC", q, s, _want(f"epi {BM} {layout} r", o_bits), o_bits)
    _same(f"{plan['name']} {layout}: QT", qT, sT, _want(f"epi {BM} {layout} c", colsb), colsb)
    G.check(plan["name"])


def test_gemm_epilogue_qc_f32_output_branch():
    """The 4-wave epilogue's other QC branch (multiply + convert) is the one an f32 output takes; the plan refuses
    a residual there, so the outputs are products: A is the oracle's quantisation of the sweep, B a quantised
    identity, and C = dequantised A exactly (asserted bit for bit, f32 denormals included).  This branch
    therefore sees only e4m3 multiples of powers of two; QC is the oracle on them.  The elements that
    quantise to 256 * 2^120 = 2^128 (beside the largest finite bf16 as block maximum) have no f32 value: zero
    bytes stand in for them."""
    hip, F = _mods()
    from learning_jax_sharding_amd.ops.fp8 import dequantize_mx_ref
    N = K = 128
    a_bits = O.as_rows(_stream("bf16"), K, 128)
    M = a_bits.shape[0]
    aq, as_ = (t.clone() for t in _want("rows128x128 bf16", a_bits))
    over = (as_ == 247) & ((aq & 0x7F) == 0x78)                          # 0x78 = 256, scale byte 247 = 2^120
    assert 0 < int(over.sum()) < 20000
    aq[over] = 0
    exact = dequantize_mx_ref(aq.reshape(M, K).view(torch.float8_e4m3fn), as_.reshape(M, K // 32).int() - 127)
    assert torch.isfinite(exact).all()                                   # (exact: tests/test_mx_oracle.py)
    qa, sa = aq.reshape(M, K).cuda(), as_.reshape(M, K // 32).cuda()
    qb = (torch.eye(N, dtype=torch.int32) * 0x38).to(U8).cuda()          # 0x38 = 1.0
    sb = torch.full((N, K // 32), 127, dtype=U8).cuda()
    flags = F.mx_flags(F32, qout=True)
    plan = F.gemm_mx_plan(M, N, K, flags, 1282)
    assert plan["err"] == 0 and plan["name"] == "gemm_mx_fp8<128,2,fix=0>" and plan["out_f32"], plan
    G = Guarded()
    out, q, s = G.new((M, N), F32), G.new((M, N)), G.new((M, N // 32))
    with hip.launch_log() as log:
        F.gemm_mx(qa, sa, qb, sb, M, N, K, out, qout=(q, s), tile=1282)
    assert _names(log) == [plan["name"]] and log[0]["variant"] == 0, log
    torch.cuda.synchronize()
    c_bits = O.bits_of(exact) & 0x7FFFFFFF | torch.where(exact == 0, 0, O.bits_of(exact) & 0x80000000)
    got = O.bits_of(out.cpu())
    assert torch.equal(torch.where(got == 0x80000000, 0, got), c_bits), "C is not the dequantised A"
    w = O.quantize(c_bits, "via_bf16")
    _same("gemm_mx_fp8<128,2,fix=0> f32: QC", q, s, (w[0].reshape(-1, 32), w[1].reshape(-1, 1)), c_bits)
    G.check("gemm_mx_fp8 f32 QC")


# ----------------------------------------------------------------------------- Adam's MX shadows
@pytest.mark.parametrize("layout", ["rows", "cols"])
@pytest.mark.parametrize("rows", [0, 64], ids=["auto", "forced64"])
def test_adam_mx_shadows(rows, layout):
    """``lr = 0``, ``wd = 0``, zero gradient and moments: the parameter keeps its bits and the shadows are the
    ``direct`` quantisation of the f32 parameter -- ``QN`` along its rows, ``QT`` (transposed) along its columns.
    A tensor with MX shadows runs 64-row tiles only (``shadow.mx_eligible``): the automatic height and the
    forced 64 are the heights the launcher lets it take.  C = 64."""
    hip, F = _mods()
    from learning_jax_sharding_amd.ops import shadow
    C = 64
    st = _stream("f32")
    bits = O.as_rows(st, C, 64) if layout == "rows" else O.as_cols(st, C, 64)
    R = bits.shape[0]
    p = _tensor(bits, F32)
    g, m, v = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
    hip.set_adam_rows(rows)
    try:
        assert shadow.mx_eligible(p)
        shadow.get_mx(p, "QN")
        shadow.get_mx(p, "QT")
        e = shadow.entry(p, create=False)
        G = Guarded()       # the shadows the kernel writes: guarded, and holding 0xA5 so that it must write them
        e.bufs["QN"], e.bufs["QNs"] = G.new((R, C)), G.new((R, C // 32))
        e.bufs["QT"], e.bufs["QTs"] = G.new((C, R)), G.new((C, R // 32))
        step = torch.ones((), dtype=torch.int32, device="cuda")
        with hip.launch_log() as log:
            hip.adam_multi([(p, g, m, v)], step, 0.0, 0.9, 0.999, 1e-8, 0.0)
        assert _names(log) == ["adam_multi<64>"], log
        torch.cuda.synchronize()
    finally:
        hip.set_adam_rows(0)
    assert torch.equal(O.bits_of(p.cpu()), bits), "the parameter's bits changed"
    assert not m.any() and not v.any()
    colsb = bits.t().contiguous()
    _same(f"adam_multi<64> {layout}: QN", e.bufs["QN"], e.bufs["QNs"], _want(f"adam {layout} r", bits), bits)
    _same(f"adam_multi<64> {layout}: QT", e.bufs["QT"], e.bufs["QTs"], _want(f"adam {layout} c", colsb), colsb)
    G.check("adam_multi<64>")


# ----------------------------------------------------------------------------- the reader of a zero scale byte
def test_decode_reads_a_zero_scale_byte_as_2_pow_minus_127():
    """A block whose exponent clamps at -127 is live data with scale byte 0, and ``attn_decode<..,mx8>`` must read
    it as ``q * 2^-127`` like ``dequantize_mx_ref`` and the block-scaled MFMA, not as zeros: with one key per
    sequence the softmax weight is exactly 1 and ``o`` is that key's V row, i.e. the exact dequantisation (an
    f32 number; the bytes below 2^-6 give f32 denormals) rounded to bf16 -- except that the accumulation
    ``+0 + 1 * (-0)`` gives ``+0``, so a negative zero byte comes back as ``+0``.  V (and K) are all 727 such blocks
    of the sweep as the oracle quantises them."""
    hip, _ = _mods()
    from learning_jax_sharding_amd.ops.fp8 import dequantize_mx_ref
    sw = O.bf16_sweep() << 16
    wq, ws = _want("sweep", sw)
    live = (ws[:, 0] == 0) & ((wq & 0x7F) != 0).any(1)
    assert int(live.sum()) == 727
    B, H, cap = 46, 8, 64
    vq = O.pad_blocks(wq[live], 2 * H * B).reshape(B, 1, H, 64)
    vs = torch.zeros((B, 1, H, 2), dtype=U8)
    exact = dequantize_mx_ref(vq.view(torch.float8_e4m3fn), vs.int() - 127)        # (exact: tests/test_mx_oracle.py)
    assert bool((exact != 0).any())
    want = O.round_bf16(O.bits_of(exact)).reshape(B, 1, H, 64)
    want = torch.where(want == 0x8000, torch.zeros_like(want), want)
    assert int((want != 0).sum()) > 20000
    kc, kcs = torch.zeros((B, cap, H, 64), dtype=U8), torch.zeros((B, cap, H, 2), dtype=U8)
    kc[:, :1], kcs[:, :1] = vq, vs
    kc, kcs = kc.cuda(), kcs.cuda()
    q = torch.ones((B, 1, H, 64), dtype=BF16).cuda()
    lens = torch.zeros(B, dtype=torch.int32).cuda()
    with hip.launch_log() as log:
        o, _ = hip.attn_decode_q8(q, kc, kc.clone(), kcs, kcs.clone(), lens, 0.125, 1)
    assert "attn_decode<G1,mx8>" in _names(log), log
    torch.cuda.synchronize()
    got = O.bits_of(o.cpu()) >> 16
    bad = (got != want).nonzero()
    assert bad.numel() == 0, (f"{bad.shape[0]} of {want.numel()} outputs differ; first at {bad[0].tolist()}: V byte "
                              f"{hex(int(vq[tuple(bad[0])]))}, expected bf16 {hex(int(want[tuple(bad[0])]))}, "
                              f"received {hex(int(got[tuple(bad[0])]))}")
