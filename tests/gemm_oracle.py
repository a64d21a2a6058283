"""Exact-arithmetic oracle of the GEMM kernels: plain torch on the CPU, nothing of the package.

The inputs are chosen so that f32 arithmetic makes no rounding error in any summation order
(small integers; powers of two for alpha and the MX block scales): the f32 accumulator then equals
the float64 product, an f32 output must be bit-identical to the oracle and a bf16 output to the
oracle rounded to nearest even.  ``exactness`` is the condition that makes this legitimate.

The one case table below is shared by tests/test_gemm_oracle.py (CPU: every row's plan names the
instance the row claims, the claims cover every instantiated kernel) and
tests/test_gemm_oracle_gpu.py (every row run into a guarded C and compared bit for bit)."""
import itertools

import torch

BF16_NAN = 0x7FC1            # guard payloads: quiet NaNs no kernel produces
F32_NAN = 0x7FC00001
GUARD_ROWS = 4
BK = 64


# ============================================================================ operands
def _ints(gen, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=gen).double()


def _store(mat, kc, ld_pad=0, poison=5.0):
    """(2-D storage, ld) of logical [R][K] matrices ``mat`` [nb][R][K]: k-contiguous rows of
    ld = K + ld_pad, or m/n-contiguous ([K][R], ld = R + ld_pad); the pad columns hold ``poison``."""
    m = mat if kc else mat.transpose(1, 2)
    if ld_pad:
        m = torch.cat([m, torch.full(m.shape[:2] + (ld_pad,), poison, dtype=m.dtype)], 2)
    return m.contiguous(), m.shape[2]


def case(M, N, K, a_kc=True, b_kc=True, out=torch.bfloat16, batch=1, batch_a=True, batch_b=True, a_row=False,
         lda_pad=0, ldb_pad=0, a_off=0, b_off=0, bias=None, bias_batched=False, bias_skew=0, relu=False, alpha=1.0,
         accumulate=False, res=None, splitk=1, slabs=False, fold=False, lo=-8, hi=8, gaussian=False, seed=0):
    """One GEMM call and its exact answer.

    ``bias``: None / torch.float32 / torch.bfloat16 (``bias_batched``: one row per batch, sBias = N;
    ``bias_skew``: elements the bias pointer is moved off its 16-byte alignment, so the scalar
    loads run).  ``res``: None or (mode, dtype, broadcast_row) with mode "add" / "mask".
    ``a_row``: A is one row repeated (lda = 0).  ``batch_a`` / ``batch_b`` False: the operand is
    shared by the batches (stride 0).  ``fold``: weight-major batches side by side in C (sC = N,
    ldc = N * batch).  ``slabs``: split s of K writes its own f32 slab.  ``gaussian``: N(0, 1)
    operands (no exact answer: ``expected`` is None, ``bound`` the derived forward-error bound).

    Returns a dict: the stored tensors ``A`` ``B`` ``bias`` ``res`` ``c_init`` (logical
    [nb][M][N]), ``call`` (the launcher's arguments that do not depend on where C lies), ``oracle``
    (float64 [nb][M][N], nb = batch, or splits * batch in slab mode) and ``expected``."""
    gen = torch.Generator().manual_seed(seed)
    out_f32 = out == torch.float32
    nba, nbb = (batch if batch_a else 1), (batch if batch_b else 1)
    if gaussian:
        A = torch.randn((nba, 1 if a_row else M, K), generator=gen).bfloat16().double()
        B = torch.randn((nbb, K, N), generator=gen).bfloat16().double()
    else:
        A = _ints(gen, (nba, 1 if a_row else M, K), lo, hi).bfloat16().double()
        B = _ints(gen, (nbb, K, N), lo, hi).bfloat16().double()
        if not a_row and M > 3:
            A[:, 1, :] = 0                   # a row, a k-column and an output column that are all zero
        A[:, :, K // 2] = 0
        B[:, :, min(2, N - 1)] = 0
    Al = A.expand(nba, M, K) if a_row else A
    # ---- the operation, in float64
    Ab, Bb = Al.expand(batch, M, K) if nba == 1 else Al, B.expand(batch, K, N) if nbb == 1 else B
    alpha_abs = abs(alpha)
    nkt = -(-K // BK)
    s_eff = min(max(1, splitk), nkt)
    kps = -(-nkt // s_eff)
    s_eff = -(-nkt // kps)
    if slabs:
        parts = [(s * kps * BK, min(K, (s + 1) * kps * BK)) for s in range(s_eff)]
        prod = torch.cat([Ab[:, :, a:b] @ Bb[:, a:b, :] for a, b in parts], 0)       # [S * batch]: slab s * batch + b
        absum = torch.cat([Ab[:, :, a:b].abs() @ Bb[:, a:b, :].abs() for a, b in parts], 0)
    else:
        prod = Ab @ Bb
        absum = Ab.abs() @ Bb.abs()
    nb = prod.shape[0]
    y = alpha * prod
    mag = alpha_abs * absum
    bias_t = bias_l = None
    if bias is not None:
        rows = batch if bias_batched else 1
        bias_l = torch.randn((rows, N), generator=gen).to(bias).double() if gaussian else _ints(gen, (rows, N), lo, hi).to(bias).double()
        y = y + bias_l[:, None, :]
        mag = mag + bias_l.abs()[:, None, :]
        flat = bias_l.to(bias).reshape(-1)
        bias_t = torch.cat([torch.full((bias_skew,), 3.0, dtype=bias), flat])     # (the caller passes [bias_skew:])
    if relu:
        y = y.clamp_min(0.0)
    c_init = None
    if accumulate:
        c_init = _ints(gen, (nb, M, N), 8 * lo, 8 * hi)
        y = y + c_init
        mag = mag + c_init.abs()
    res_t, res_l, res_ld, sR, res_mode = None, None, 0, 0, "add"
    if res is not None:
        res_mode, rdt, brow = res
        shape = (1, 1, N) if brow else (batch, M, N)
        res_l = torch.randn(shape, generator=gen).to(rdt).double() if gaussian else _ints(gen, shape, lo, hi).to(rdt).double()
        res_t = res_l.to(rdt).reshape(-1, N).contiguous()
        res_ld, sR = (0, 0) if brow else (N, M * N)
        mag = mag + res_l.abs() if res_mode == "add" else mag
    # ---- the exact expected output, rounded where the kernels round
    expected = None
    if not gaussian:
        y32 = y.float()
        assert torch.equal(y32.double(), y)
        if out_f32:
            expected = y32
        elif res is None:
            expected = y32.bfloat16()
        elif res_mode == "add":
            expected = (y32.bfloat16().float() + res_l.float().bfloat16().float()).bfloat16()
        else:
            expected = torch.where(res_l > 0, y32, torch.zeros_like(y32)).bfloat16()
    oracle = y
    if res is not None:
        oracle = y + res_l if res_mode == "add" else torch.where(res_l > 0, y, torch.zeros_like(y))
    # forward-error bound of any order of f32 accumulation over exact bf16 x bf16 products plus the
    # epilogue's two roundings; a bf16 output adds its own rounding, 2^-8 |oracle| (bf16 keeps 8
    # significant bits: round-to-nearest errs by at most 2^-8 of the value).  A residual add rounds
    # twice, out = bf16(s), s = f32(bf16(v) + r) with v the f32 value of y: |s - oracle| <= e1 =
    # fwd + 2^-8 (|y| + fwd) + 2^-24 |s|, and |out - s| <= 2^-8 |s| with |s| <= |oracle| + e1.
    fwd = (K + 2) * 2.0 ** -24 * mag
    bound = fwd
    if not out_f32:
        bound = fwd + 2.0 ** -8 * oracle.abs()
        if res is not None and res_mode == "add":
            e1 = (fwd + 2.0 ** -8 * (y.abs() + fwd) + 2.0 ** -24 * oracle.abs()) / (1 - 2.0 ** -24)
            bound = e1 + 2.0 ** -8 * (oracle.abs() + e1)
    if fold:     # [batch][M][N] -> one [M][batch * N]
        assert batch_b and not batch_a and not slabs
        cat = lambda t: None if t is None else t.permute(1, 0, 2).reshape(1, M, batch * N)   # noqa: E731
        oracle, expected, bound, mag, c_init = cat(oracle), cat(expected), cat(bound), cat(mag), cat(c_init)
        nb = 1
    As, lda = _store(A.bfloat16(), a_kc, lda_pad)
    Bs, ldb = _store(B.transpose(1, 2).bfloat16(), b_kc, ldb_pad)
    sA, sB = (As[0].numel() if nba > 1 else 0), (Bs[0].numel() if nbb > 1 else 0)
    if fold:
        sB = N * ldb
    if a_row:
        assert a_kc
        lda = 0
    pad = lambda t, n: torch.cat([torch.full((n,), 7.0, dtype=t.dtype), t.reshape(-1)])     # noqa: E731
    call = dict(M=M, N=N, K=K, lda=lda, ldb=ldb, a_kc=a_kc, b_kc=b_kc, batch=batch, sA=sA, sB=sB,
                sBias=N if bias_batched else 0, relu=relu, alpha=alpha, accumulate=accumulate, splitk=splitk,
                a_off=a_off, b_off=b_off, res_ld=res_ld, res_mode=res_mode, sR=sR, slabs=slabs)
    return dict(A=pad(As, a_off), B=pad(Bs, b_off), bias=bias_t, bias_skew=bias_skew, res=res_t, c_init=c_init,
                call=call, out=out, nb=nb, fold=fold, splits=s_eff, oracle=oracle, expected=expected, bound=bound,
                mag=mag, terms=(alpha * Al, B) + tuple(t for t in (bias_l, c_init, res_l) if t is not None),
                gaussian=gaussian)


def _grain(t, start=1.0):
    """The largest power of two <= ``start`` that every element of ``t`` is a multiple of."""
    g = start
    for _ in range(60):
        if torch.equal(torch.round(t / g) * g, t):
            return g
        g /= 2
    raise AssertionError("no dyadic granularity")


def exactness(c):
    """max over the outputs of (|alpha| sum_k |a_k b_k| + |bias| + |C_in| + |res|) / g, g the
    granularity every term is a multiple of: below 2^24 every partial sum in any order (fused
    multiply-add or not) is an f32 number, so "bit-identical" is the right demand."""
    a, b = c["terms"][0], c["terms"][1]
    g = _grain(a) * _grain(b)
    for t in c["terms"][2:]:
        g = min(g, _grain(t))
    return float(c["mag"].max()) / g


# ============================================================================ guarded C
def guard_geometry(nb, M, N, pad=8):
    """C as [nb] blocks of GUARD_ROWS + M + GUARD_ROWS rows of ld = N + pad elements: (ld, sC,
    c_off, rows).  With N and pad multiples of 8 so are sC and c_off: the view stays 16-byte
    aligned and the LDS-DMA store conditions hold (other pads: the unaligned store paths)."""
    ld = N + pad
    rows = M + 2 * GUARD_ROWS
    return ld, rows * ld, GUARD_ROWS * ld, rows


class Guarded:
    def __init__(self, shape, dtype, device="cpu", pad=8):
        nb, M, N = shape if len(shape) == 3 else (1,) + tuple(shape)
        self.ld, self.sC, self.c_off, rows = guard_geometry(nb, M, N, pad)
        self.dtype, self.shape = dtype, (nb, M, N)
        self.idt, self.payload = (torch.int16, BF16_NAN) if dtype == torch.bfloat16 else (torch.int32, F32_NAN)
        self.buf = torch.full((nb, rows, self.ld), self.payload, dtype=self.idt, device=device).view(dtype)
        self.view = self.buf[:, GUARD_ROWS:GUARD_ROWS + M, :N]
        assert self.ld % 8 or self.view.data_ptr() % 16 == 0 or device == "cpu"

    def check(self, written=True):
        """Every guard element still holds the payload; no output element does (``written``), or
        every one still does (a rejected call)."""
        nb, M, N = self.shape
        bits = self.buf.view(self.idt).cpu()
        mask = torch.zeros(bits.shape, dtype=torch.bool)
        mask[:, GUARD_ROWS:GUARD_ROWS + M, :N] = True
        hit = (bits != self.payload) & ~mask
        assert not hit.any(), f"{int(hit.sum())} guard elements overwritten, first (block, row, col) " \
                              f"{[tuple(i) for i in hit.nonzero()[:8].tolist()]} (output rows start at {GUARD_ROWS})"
        inside = bits[:, GUARD_ROWS:GUARD_ROWS + M, :N] == self.payload
        if written:
            assert not inside.any(), f"{int(inside.sum())} output elements never written, first " \
                                     f"{[tuple(i) for i in inside.nonzero()[:8].tolist()]}"
        else:
            assert inside.all(), "a rejected call wrote to C"


def guarded(shape, dtype, device="cpu", pad=8):
    """(C view inside a larger NaN-payload buffer, its Guarded with .check())."""
    g = Guarded(shape, dtype, device, pad)
    return g.view, g


# ============================================================================ mismatch report
def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 1: torch.uint8}[t.element_size()])


def mismatch_report(got, want, bm=None, bn=None, first=8):
    """'' when ``got`` and ``want`` ([nb][M][N], same dtype) agree bit for bit, else the count and
    the first few (batch, row, col, got, want) with row % BM, col % BN of the launched tile."""
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    bad = _bits(got) != _bits(want)
    if not bad.any():
        return ""
    idx = bad.nonzero()
    rows, cols = sorted(set(idx[:, -2].tolist())), sorted(set(idx[:, -1].tolist()))
    lines = [f"{len(idx)} of {bad.numel()} elements differ, in {len(rows)} rows {rows[0]}..{rows[-1]} and "
             f"{len(cols)} columns {cols[0]}..{cols[-1]}"]
    for i in idx[:first].tolist():
        b, r, c = ([0] * (3 - len(i)) + i)
        where = f" row % {bm} = {r % bm}, col % {bn} = {c % bn}" if bm else ""
        lines.append(f"  (batch {b}, row {r}, col {c}): got {float(got[tuple(i)])!r} want {float(want[tuple(i)])!r}{where}")
    return "\n".join(lines)


def assert_bits_equal(got, want, bm=None, bn=None):
    if not torch.equal(_bits(got.cpu()), _bits(want.cpu())):
        raise AssertionError(mismatch_report(got, want, bm, bn))


# ============================================================================ MX-fp8 operands
def mx_operand(gen, R, K, lo=-8, hi=8):
    """One MX operand with independently known scales: (payload bytes uint8 [R][K], scale bytes
    uint8 [R][K / 32] = 127 + e with e in {-1, 0, 1} drawn per (row, 32-block), its float64 value)."""
    v = torch.randint(lo, hi + 1, (R, K), generator=gen).float()
    q8 = v.to(torch.float8_e4m3fn)
    assert torch.equal(q8.float(), v)                  # small integers round-trip e4m3 exactly
    e = torch.randint(-1, 2, (R, K // 32), generator=gen)
    deq = v.double().reshape(R, K // 32, 32) * torch.ldexp(torch.ones(()), e).double()[..., None]
    return q8.view(torch.uint8), (127 + e).to(torch.uint8), deq.reshape(R, K)


def mx_case(M, N, K, lo=-8, hi=8, a_bcast=False, b_bcast=False, bias=False, relu=False, out=torch.float32,
            res=None, nsplit=1, seed=0):
    """One ``gemm_mx`` call on constructed operands and its exact answer.  ``bias``: False, True (an
    f32 bias) or its dtype.  ``res``: None or
    (mode, kind) with kind "bf16" or "e4m3" (the uint8 mask).  ``nsplit`` > 1: f32 slabs."""
    gen = torch.Generator().manual_seed(seed)
    qa, sa, A = mx_operand(gen, 1 if a_bcast else M, K, lo, hi)
    qb, sb, B = mx_operand(gen, 1 if b_bcast else N, K, lo, hi)
    A, B = A.expand(M, K), B.expand(N, K)
    nkt = K // 128
    kps = -(-nkt // nsplit)
    parts = [(s * kps * 128, min(K, (s + 1) * kps * 128)) for s in range(nsplit)]
    y = torch.stack([A[:, a:b] @ B[:, a:b].t() for a, b in parts])
    mag = torch.stack([A[:, a:b].abs() @ B[:, a:b].abs().t() for a, b in parts])
    bias_t = None
    if bias:
        bias_t = _ints(gen, (N,), lo, hi).to(bias if isinstance(bias, torch.dtype) else torch.float32)   # (exact in bf16)
        y, mag = y + bias_t.double(), mag + bias_t.abs().double()
    if relu:
        y = y.clamp_min(0.0)
    res_t, res_mode, res_l = None, "add", None
    if res is not None:
        res_mode, kind = res
        res_l = _ints(gen, (M, N), lo, hi)
        res_t = res_l.bfloat16() if kind == "bf16" else res_l.float().to(torch.float8_e4m3fn).view(torch.uint8)
    y32 = y.float()
    assert torch.equal(y32.double(), y)
    if out == torch.float32:
        expected = y32
    elif res is None:
        expected = y32.bfloat16()
    elif res_mode == "add":
        expected = (y32.bfloat16().float() + res_l.float()).bfloat16()
        mag = mag + res_l.abs()
    else:
        expected = torch.where(res_l > 0, y32, torch.zeros_like(y32)).bfloat16()
    return dict(qa=qa, sa=sa, qb=qb, sb=sb, bias=bias_t, res=res_t, res_mode=res_mode, oracle=y, expected=expected,
                mag=mag, terms=(A, B) + ((bias_t.double(),) if bias else ()) + ((res_l,) if res is not None else ()),
                deq=(A, B))


# ============================================================================ the case table
# The LDS-DMA tile table of csrc/kernels/gemm.hip (LJS_GEMM_TILES), restated as data:
#   code: (BM, BN, WM, WN, NST, KK, KKF, MIX, MN, LEAN)
TILES = {
    643: (64, 64, 2, 2, 3, 1, 1, 1, 1, 0),
    644: (64, 64, 2, 2, 4, 3, 1, 1, 1, 2),
    1282: (128, 128, 2, 2, 2, 5, 1, 1, 2, 2),
    1284: (128, 128, 2, 2, 4, 5, 1, 1, 1, 2),
    1602: (128, 160, 4, 1, 2, 5, 0, 0, 0, 1),
    2561: (256, 128, 4, 2, 3, 5, 1, 0, 0, 2),
    2562: (256, 192, 4, 2, 2, 3, 0, 0, 0, 2),
    2563: (256, 128, 4, 2, 3, 0, 0, 0, 1, 0),
    12856: (128, 256, 2, 4, 3, 0, 0, 0, 1, 0),
    12883: (128, 128, 2, 4, 3, 5, 1, 0, 2, 2),
    12884: (128, 128, 2, 4, 4, 5, 1, 0, 2, 2),
}
_MIX = [(0, 0, 0), (1, 0, 0), (1, 0, 1), (0, 1, 0), (0, 1, 1)]     # (a_kc, b_kc, out_f32)
_REG_LAYOUTS = list(itertools.product((1, 0), (1, 0), (0, 1)))


def _kc(b):
    return "kc" if b else "mn"


def dma_name(code, a_kc, b_kc, out_f32, group2=False):
    bm, bn, wm, wn, nst = TILES[code][:5]
    return f"{'gemm_dma_group2' if group2 else 'gemm_dma'}<{bm},{bn},{wm},{wn},{nst},{_kc(a_kc)},{_kc(b_kc)}," \
           f"{'f32' if out_f32 else 'bf16'}>"


def lean_name(code):
    return "gemm_lean<%d,%d,%d,%d,%d>" % TILES[code][:5]


def reg_name(t, a_kc, b_kc, out_f32):
    return f"gemm_bf16<{t},{t},{_kc(a_kc)},{_kc(b_kc)},{'f32' if out_f32 else 'bf16'}>"


def instantiated():
    """Every (kernel instance name, epilogue variant) the library instantiates, from TILES' columns
    (the register-staged 8 layouts x 2 tiles have no variant)."""
    inst = set()
    for code, (bm, bn, wm, wn, nst, kk, kkf, mix, mn, lean) in TILES.items():
        if kk:
            inst |= {(dma_name(code, 1, 1, 0), v) for v in (range(5) if kk > 1 else (0,))}
        if kkf:
            inst.add((dma_name(code, 1, 1, 1), 0))
        if mix:
            inst |= {(dma_name(code, *l), 0) for l in _MIX}
        if mn:
            inst.add((dma_name(code, 0, 0, 1), 0))
        if mn == 2:
            inst |= {(dma_name(code, 0, 0, 1), 3), (dma_name(code, 0, 0, 1, True), 3)}
        if lean:
            inst |= {(lean_name(code), v) for v in range(5)}
    for t in (64, 128):
        inst |= {(reg_name(t, *l), None) for l in _REG_LAYOUTS}
    return inst


# instantiated, but no call reaches them: a call with an epilogue operand (RES 1 / 2) demotes the
# KK = 3 tiles 644 (to the register-staged 64x64) and 2562 (to 1282) in the plan
UNREACHABLE = {(n, v) for code in (644, 2562) for n in (dma_name(code, 1, 1, 0), lean_name(code)) for v in (1, 2)}

# what reaches each epilogue variant of the k-contiguous bf16 kernels; the features rotate over the
# tiles so each is seen on general and lean kernels, 4 and 8 waves
_VARIANT_CALLS = {
    0: [dict(alpha=0.5), dict(bias=torch.bfloat16, relu=True), dict(alpha=2.0, bias=torch.float32, relu=True),
        dict(bias=torch.bfloat16, bias_skew=4, alpha=0.5)],
    1: [dict(res=("add", torch.bfloat16, False)), dict(res=("mask", torch.bfloat16, False), bias=torch.float32),
        dict(res=("add", torch.bfloat16, True), alpha=0.5)],
    2: [dict(res=("mask", torch.float32, False)), dict(res=("add", torch.float32, False), relu=True),
        dict(res=("add", torch.float32, True))],
    3: [dict()],
    4: [dict(bias=torch.float32)],
}


def _shape(bm, bn, i):
    """One ragged block in each direction; every other case a single N block whose second wave
    column is partly full (the (264, 136) / (136, 72) / (72, 40) families)."""
    return bm + 8, (bn + 8 if i % 2 == 0 else bn // 2 + 8)


def _row(id, tile, claim, resolved, call, kind="gemm", splitk=1, **more):
    return dict(id=id, tile=tile, claim=claim, resolved=resolved, call=call, kind=kind, splitk=splitk, **more)


def build_table():
    rows, n = [], 0

    def add(*a, **k):
        nonlocal n
        n += 1
        k.setdefault("call", {})
        k["call"].setdefault("seed", n)
        rows.append(_row(*a, **k))

    for code, (bm, bn, wm, wn, nst, kk, kkf, mix, mn, lean) in TILES.items():
        deep = BK * (nst + 1)                          # the ring refills and wraps
        for fam in ("dma", "lean"):
            if (fam == "dma" and not kk) or (fam == "lean" and not lean):
                continue
            name = dma_name(code, 1, 1, 0) if fam == "dma" else lean_name(code)
            # forcing: + 200000 the general kernel, + 100000 the lean one (a tile's default: LEAN == 2)
            req = code + (200000 if lean == 2 else 0) if fam == "dma" else code + (0 if lean == 2 else 100000)
            for v in (range(5) if kk > 1 else (0,)):
                if (name, v) in UNREACHABLE:
                    continue
                opts = _VARIANT_CALLS[v] if kk > 1 else [dict()]      # (KK = 1: RES 0 whatever the call)
                feat = opts[(code + (fam == "lean")) % len(opts)]
                M, N = _shape(bm, bn, v + (fam == "lean"))
                K = deep if v in (1, 3) else BK
                add(f"{fam}-{code}-v{v}", req, (name, v), code, call=dict(M=M, N=N, K=K, **feat))
        if kkf:
            M, N = _shape(bm, bn, 0)
            add(f"kkf-{code}", code, (dma_name(code, 1, 1, 1), 0), code,
                call=dict(M=M, N=N, K=deep, out=torch.float32, alpha=0.5, bias=torch.float32))
        if mix:
            for i, (ak, bk, of) in enumerate(_MIX):
                M, N = _shape(bm, bn, i)
                feat = [dict(), dict(relu=True, bias=torch.float32), dict(alpha=2.0)][i % 3]
                add(f"mix-{code}-{_kc(ak)}-{_kc(bk)}-{'f32' if of else 'bf16'}", code, (dma_name(code, ak, bk, of), 0), code,
                    call=dict(M=M, N=N, K=deep if i % 2 else BK, a_kc=bool(ak), b_kc=bool(bk),
                              out=torch.float32 if of else torch.bfloat16, **feat))
        if mn:
            M, N = _shape(bm, bn, 0)
            add(f"mn-{code}", code, (dma_name(code, 0, 0, 1), 0), code,
                call=dict(M=M, N=N, K=deep, a_kc=False, b_kc=False, out=torch.float32, alpha=0.5))
        if mn == 2:
            # slab mode, uneven splits: 7 K-tiles over 3 splits (3 + 3 + 1), the last runs past K
            add(f"slab-{code}", code, (dma_name(code, 0, 0, 1), 3), code, splitk=3,
                call=dict(M=136, N=72, K=448, a_kc=False, b_kc=False, out=torch.float32, splitk=3, slabs=True))
            add(f"group2-{code}", code, (dma_name(code, 0, 0, 1, True), 3), code, kind="group2", splitk=3, splitk1=2,
                call=dict(M=136, N=72, K=448, a_kc=False, b_kc=False, out=torch.float32, splitk=3, slabs=True),
                call1=dict(M=72, N=200, K=448, a_kc=False, b_kc=False, out=torch.float32, splitk=2, slabs=True,
                           seed=1000 + code))
    # ---- register-staged: 8 layouts x 2 tiles, asked for by code and reached by demotion (K = 40)
    feats = [dict(), dict(alpha=0.5, bias=torch.float32), dict(relu=True, bias=torch.bfloat16), dict(alpha=2.0)]
    for t, (i, (ak, bk, of)) in itertools.product((64, 128), enumerate(_REG_LAYOUTS)):
        feat = dict(feats[i % 4])
        if not of and i % 3 == 0:
            feat["res"] = [("add", torch.bfloat16, False), ("mask", torch.float32, False)][(i // 3) % 2]
        if of and i % 4 == 1:
            feat["accumulate"] = True
        req = t if i % 2 == 0 else (644 if t == 64 else 1282)
        add(f"reg-{t}-{_kc(ak)}-{_kc(bk)}-{'f32' if of else 'bf16'}", req, (reg_name(t, ak, bk, of), None), t,
            call=dict(M=136, N=72, K=40, a_kc=bool(ak), b_kc=bool(bk), out=torch.float32 if of else torch.bfloat16, **feat))
    # ---- arguments today's suite never checks against the operation
    f32, bf16 = torch.float32, torch.bfloat16
    G, L = 201282, 1282                              # one general and one lean instance
    gname, lname = dma_name(1282, 1, 1, 0), lean_name(1282)
    add("acc-kkf", 1284, (dma_name(1284, 1, 1, 1), 0), 1284, call=dict(M=136, N=136, K=128, out=f32, accumulate=True))
    add("acc-kkf-tail", 1284, (dma_name(1284, 1, 1, 1), 0), 1284,
        call=dict(M=136, N=134, K=128, out=f32, accumulate=True, alpha=0.5), pad=10)    # N % 4: the scalar tail
    add("acc-splitk-mn", 1282, (dma_name(1282, 0, 0, 1), 0), 1282, splitk=2,
        call=dict(M=136, N=72, K=256, a_kc=False, b_kc=False, out=f32, accumulate=True, splitk=2))
    add("acc-splitk-reg", 128, (reg_name(128, 0, 0, 1), None), 128, splitk=2,
        call=dict(M=136, N=72, K=128, a_kc=False, b_kc=False, out=f32, accumulate=True, splitk=2))
    for tag, req, claim in (("g", G, (gname, None)), ("l", L, (lname, None))):
        nm = claim[0]
        add(f"offsets-{tag}", req, (nm, 3), 1282, call=dict(M=136, N=72, K=128, a_off=8, b_off=24))
        add(f"ldpad-{tag}", req, (nm, 3), 1282, call=dict(M=136, N=72, K=128, lda_pad=8, ldb_pad=16))
        add(f"lda0-{tag}", req, (nm, 3), 1282, call=dict(M=136, N=72, K=128, a_row=True))
        add(f"batch-sA0-{tag}", req, (nm, 3), 1282, call=dict(M=136, N=72, K=64, batch=3, batch_a=False))
        add(f"batch-sA-{tag}", req, (nm, 0), 1282, call=dict(M=136, N=72, K=64, batch=3, batch_b=False, alpha=0.5))
        add(f"batch-bias-{tag}", req, (nm, 4), 1282,
            call=dict(M=136, N=72, K=64, batch=3, bias=f32, bias_batched=True))
        add(f"bias-bf16-n72-{tag}", req, (nm, 0), 1282, call=dict(M=136, N=72, K=64, bias=bf16))
        add(f"bias-bf16-skew-{tag}", req, (nm, 0), 1282, call=dict(M=136, N=72, K=64, bias=bf16, bias_skew=3, relu=True))
        # fused output sums: operands in [-2, 2] and K = 64, so every per-wave partial is exact
        add(f"psum-{tag}", req, (nm, 0), 1282, call=dict(M=136, N=136, K=64, lo=-2, hi=2), psum=True)
    add("lda0-reg", 128, (reg_name(128, 1, 0, 1), None), 128,
        call=dict(M=136, N=72, K=40, a_row=True, b_kc=False, out=f32))
    add("offsets-reg", 64, (reg_name(64, 0, 1, 0), None), 64,
        call=dict(M=136, N=72, K=40, a_kc=False, a_off=16, b_off=8))
    add("odd-n-reg", 128, (reg_name(128, 1, 1, 0), None), 128, call=dict(M=130, N=67, K=40, bias=f32), pad=0)
    # the fused projection's weight-major 3-batch: folded into one GEMM by 2562, else a real batch on 2561
    add("fold-2562", 2562, (lean_name(2562), 3), 2562, call=dict(M=264, N=72, K=128, batch=3, batch_a=False, fold=True),
        launched=(216, 1))
    add("fold-2562-general", 202562, (dma_name(2562, 1, 1, 0), 0), 2562,
        call=dict(M=264, N=72, K=128, batch=3, batch_a=False, fold=True, alpha=0.5), launched=(216, 1))
    add("unfold-2561", 2562, (lean_name(2561), 4), 2561,
        call=dict(M=264, N=72, K=128, batch=3, batch_a=False, fold=True, bias=f32, bias_batched=True), launched=(72, 3))
    # ---- Gaussian inputs, a non-dyadic alpha: one per kernel family, against the derived bound
    ga = dict(gaussian=True, alpha=0.37)
    add("gauss-reg", 128, (reg_name(128, 1, 1, 0), None), 128, kind="gauss",
        call=dict(M=136, N=72, K=40, bias=f32, **ga))
    add("gauss-reg-f32", 64, (reg_name(64, 0, 0, 1), None), 64, kind="gauss",
        call=dict(M=136, N=72, K=40, a_kc=False, b_kc=False, out=f32, **ga))
    add("gauss-general", 201284, (dma_name(1284, 1, 1, 0), 0), 1284, kind="gauss",
        call=dict(M=136, N=136, K=640, bias=bf16, relu=True, **ga))
    add("gauss-general-f32", 2561, (dma_name(2561, 1, 1, 1), 0), 2561, kind="gauss",
        call=dict(M=264, N=136, K=640, out=f32, bias=f32, **ga))
    add("gauss-lean", 12883, (lean_name(12883), 0), 12883, kind="gauss", call=dict(M=136, N=136, K=640, **ga))
    add("gauss-lean-res", 2561, (lean_name(2561), 1), 2561, kind="gauss",
        call=dict(M=264, N=136, K=320, res=("add", bf16, False), **ga))
    add("gauss-slab", 1282, (dma_name(1282, 0, 0, 1), 3), 1282, kind="gauss", splitk=3,
        call=dict(M=136, N=72, K=448, a_kc=False, b_kc=False, out=f32, splitk=3, slabs=True, gaussian=True))
    # ---- the shared bf16 epilogue's other combinations, general and lean (last, so the rows above
    # keep their seeds): a misaligned f32 bias (RES 4's scalar loads), the fused sum behind the f32
    # bias (RES 4, the out-projection's call) and behind a residual add (RES 1); then the operand
    # instances RES 1 (bf16 R) and RES 2 (f32 R) with an aligned bias, a misaligned one and the fused
    # sum.  With RES 0's rows above (bias-bf16-n72, bias-bf16-skew, psum) every instance that has the
    # code runs it: RES 3 is the plain store loop, which a bias or a fused sum never reaches (the
    # plan gives such a call RES 0 or 4), and RES 4's bias is f32 by definition.
    for tag, req, nm in (("g", G, gname), ("l", L, lname)):
        add(f"res1-bias-{tag}", req, (nm, 1), 1282,
            call=dict(M=136, N=72, K=64, bias=bf16, res=("add", bf16, False)))
        add(f"res1-bias-skew-{tag}", req, (nm, 1), 1282,
            call=dict(M=136, N=72, K=64, bias=f32, bias_skew=1, res=("mask", bf16, False)))
        add(f"res2-bias-{tag}", req, (nm, 2), 1282,
            call=dict(M=136, N=72, K=64, bias=f32, res=("add", f32, False)))
        add(f"res2-bias-skew-{tag}", req, (nm, 2), 1282,
            call=dict(M=136, N=72, K=64, bias=bf16, bias_skew=5, relu=True, res=("mask", f32, False)))
        add(f"psum-res2-{tag}", req, (nm, 2), 1282,
            call=dict(M=136, N=136, K=64, lo=-2, hi=2, bias=f32, res=("add", f32, False)), psum=True)
        add(f"bias-f32-skew-{tag}", req, (nm, 4), 1282, call=dict(M=136, N=72, K=64, bias=f32, bias_skew=1))
        add(f"psum-bias-{tag}", req, (nm, 4), 1282, call=dict(M=136, N=136, K=64, lo=-2, hi=2, bias=f32), psum=True)
        add(f"psum-res-{tag}", req, (nm, 1), 1282,
            call=dict(M=136, N=136, K=64, lo=-2, hi=2, res=("add", bf16, False)), psum=True)
    return rows


TABLE = build_table()


def plan_args(row, c=None):
    """hip.gemm_plan's arguments for a table row (C in its guarded geometry)."""
    c = c or case(**row["call"])
    k = c["call"]
    if c["fold"]:
        ld, sC = k["N"] * k["batch"], k["N"]
    else:
        ld, sC, _, _ = guard_geometry(c["nb"], k["M"], k["N"], row.get("pad", 8))
    res_dtype = row["call"]["res"][1] if row["call"].get("res") else None
    return dict(M=k["M"], N=k["N"], K=k["K"], lda=k["lda"], ldb=k["ldb"], ldc=ld, a_kc=k["a_kc"], b_kc=k["b_kc"],
                out_f32=c["out"] == torch.float32, batch=k["batch"], sA=k["sA"], sB=k["sB"], sC=sC,
                bias_dtype=row["call"].get("bias"), relu=k["relu"], alpha=k["alpha"], accumulate=k["accumulate"],
                splitk=k["splitk"], tile=row["tile"], res_dtype=res_dtype, res_ld=k["res_ld"], res_mode=k["res_mode"],
                sR=k["sR"], slabs=k["slabs"], psum=bool(row.get("psum")))


def persistent_rows(slots_of):
    """A grid smaller than the item count: items = 2 x the resident slots, ragged M and N, K = 128,
    on one 4-wave and one 8-wave tile, general and lean.  ``slots_of(plan kwargs)``: the plan's grid
    of a call of more than ``slots`` whole rounds (the caller's CU count)."""
    rows = []
    for req, code, name in ((1282, 1282, lean_name(1282)), (201282, 1282, dma_name(1282, 1, 1, 0)),
                            (2561, 2561, lean_name(2561)), (202561, 2561, dma_name(2561, 1, 1, 0))):
        bm, bn = TILES[code][:2]
        M, N = bm + 8, bn + 8                                  # 4 items per batch
        probe = dict(M=M, N=N, K=128, lda=128, ldb=128, ldc=N + 8, a_kc=True, b_kc=True, out_f32=False, batch=4096,
                     sA=M * 128, sB=0, sC=(M + 2 * GUARD_ROWS) * (N + 8), tile=req)
        slots = slots_of(probe)
        assert slots % 2 == 0 and slots <= 1024, slots       # (whole rounds of the resident slots)
        rows.append(_row(f"persistent-{req}", req, (name, 3), code, kind="persistent", slots=slots,
                         call=dict(M=M, N=N, K=128, batch=slots // 2, batch_b=False, seed=req)))
    return rows
