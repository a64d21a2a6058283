"""The MX-fp8 GEMM kernels of csrc/kernels/fp8.hip against the exact-arithmetic oracle of
tests/gemm_oracle.py (run on a real MI355X: -m gpu).  The operands are constructed, not quantized:
payload bytes from integers in [-8, 8] and a scale byte 127 + e with e drawn independently per
(row, 32-block) from {-1, 0, 1}, so every block scale is known and a mis-indexed scale operand of
the block-scaled MFMA changes the answer.  Every partial sum is a multiple of 2^-2 far below 2^20:
f32 outputs must equal the float64 product bit for bit, bf16 outputs its round-to-nearest-even, in
guarded buffers.  Every call runs under hip.launch_log(): the launch record must be the one
fp8.gemm_mx_plan gives for the same call, and over the whole file the records must name every GEMM
instance fp8.hip instantiates (tests/test_fp8_picks.py INSTANCES)."""
import pytest
import torch

import gemm_oracle as O
import test_fp8_picks as P

pytestmark = pytest.mark.gpu

dev = torch.device("cuda", 0)

_W4 = [t for t, row in P.MX_TILES.items() if row[0] == "4-wave"]
_W8 = [t for t, row in P.MX_TILES.items() if row[0] == "8-wave"]
_RAN = set()            # the instance names recorded so far (test_every_instance_ran, last in the file)


def _bm_bn(tile):
    return P.MX_TILES[tile][1:3]


@pytest.fixture(scope="module")
def F():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from learning_jax_sharding_amd.ops import fp8, hip
    hip.lib()
    return fp8


def _run(F, c, M, N, K, out_dtype, tile, nsplit=1, **kw):
    """One gemm_mx call into a guarded output (``out_dtype`` None: no output, the MX copies only);
    its launch record must be the plan's."""
    from learning_jax_sharding_amd.ops import hip
    g = None if out_dtype is None else O.Guarded((nsplit, M, N), out_dtype, dev)
    ops = [c[n].to(dev) for n in ("qa", "sa", "qb", "sb")]
    bias = None if c["bias"] is None else c["bias"].to(dev)
    res = None if c["res"] is None else c["res"].to(dev)
    out = None if g is None else (g.view if nsplit > 1 else g.view[0])
    with hip.launch_log() as log:
        F.gemm_mx(*ops, M, N, K, out, bias=bias, res=res, res_mode=c["res_mode"], tile=tile, nsplit=nsplit, **kw)
    torch.cuda.synchronize()
    flags = F.mx_flags(out_dtype, None if bias is None else bias.dtype, kw.get("relu", False),
                       None if res is None else res.dtype, c["res_mode"], "qout" in kw, "qtout" in kw, "colsum" in kw)
    plan = F.gemm_mx_plan(M, N, K, flags, tile=tile, nsplit=nsplit, C=0 if g is None else 4096)
    assert plan["err"] == 0 and len(log) == 1 == log.total, (plan, log)
    rec = log[0]
    assert rec["requested_tile"] == tile, rec
    assert {k: rec[k] for k in ("name", "resolved_tile", "splitk", "grid", "block", "variant")} == \
        {k: plan[k] for k in ("name", "resolved_tile", "splitk", "grid", "block", "variant")}, (rec, plan)
    _RAN.add(rec["name"])
    return g


@pytest.mark.parametrize("K", [128, 384])
@pytest.mark.parametrize("mode", ["f32", "bf16_bias_relu", "bf16_bias16_relu"])
@pytest.mark.parametrize("tile", _W4 + _W8)
def test_mx_gemm_tile_is_exact(F, tile, mode, K):
    """Every tile code at one ragged block in each direction, one and three 128-wide K-tiles
    (bias16: the bias is bf16, else f32)."""
    bm, bn = _bm_bn(tile)
    M, N = bm + 8, bn + 8
    f32 = mode == "f32"
    bias = False if f32 else (torch.bfloat16 if "bias16" in mode else True)
    c = O.mx_case(M, N, K, bias=bias, relu=not f32, out=torch.float32 if f32 else torch.bfloat16, seed=tile % 977 + K)
    assert O.exactness(c) < 2 ** 20
    g = _run(F, c, M, N, K, c["expected"].dtype, tile, relu=not f32)
    O.assert_bits_equal(g.view, c["expected"], bm, bn)
    g.check()


_TWO = [1282, 256160]          # one 4-wave tile and one 8-wave tile


@pytest.mark.parametrize("tile", _TWO)
def test_mx_gemm_split_slabs_sum_exactly(F, tile):
    bm, bn = _bm_bn(tile)
    M, N, K = bm + 8, bn + 8, 384                       # 3 K-tiles over 2 splits: 2 + 1
    c = O.mx_case(M, N, K, nsplit=2, seed=tile % 977)
    g = _run(F, c, M, N, K, torch.float32, tile, nsplit=2)
    O.assert_bits_equal(g.view, c["expected"], bm, bn)
    g.check()
    whole = O.mx_case(M, N, K, seed=tile % 977)
    assert torch.equal(g.view.sum(0).cpu(), whole["expected"][0])


@pytest.mark.parametrize("which", ["a_bcast", "b_bcast"])
@pytest.mark.parametrize("tile", _TWO)
def test_mx_gemm_broadcast_operand_is_exact(F, tile, which):
    bm, bn = _bm_bn(tile)
    M, N, K = bm + 8, bn + 8, 384
    c = O.mx_case(M, N, K, seed=tile % 977 + 1, **{which: True})
    g = _run(F, c, M, N, K, torch.float32, tile, **{which: True})
    O.assert_bits_equal(g.view, c["expected"], bm, bn)
    g.check()


@pytest.mark.parametrize("res", [("add", "bf16"), ("mask", "bf16"), ("mask", "e4m3")])
@pytest.mark.parametrize("tile", _TWO)
def test_mx_gemm_residual_and_masks_are_exact(F, tile, res):
    """bf16(bf16(y) + res); keep y where res > 0 and write +0 elsewhere, from a bf16 operand and from
    e4m3 bytes."""
    bm, bn = _bm_bn(tile)
    M, N, K = bm + 8, bn + 8, 128
    c = O.mx_case(M, N, K, bias=True, out=torch.bfloat16, res=res, seed=tile % 977 + 2)
    g = _run(F, c, M, N, K, torch.bfloat16, tile)
    O.assert_bits_equal(g.view, c["expected"], bm, bn)
    g.check()


@pytest.mark.parametrize("tile", _TWO)
def test_mx_gemm_quantized_copies_are_exact(F, tile):
    """qout / qtout: the MX copies of the bf16 output, rows and transposed.  The expected output is
    known exactly, so its quantization (quantize_mx_ref) is fully determined."""
    bm, bn = _bm_bn(tile)
    M, N, K = bm + 32, bn + 32, 128
    c = O.mx_case(M, N, K, bias=True, relu=True, out=torch.bfloat16, seed=tile % 977 + 3)
    want = c["expected"][0]
    outs = [torch.full(s, 0xAB, dtype=torch.uint8, device=dev) for s in ((M, N), (M, N // 32), (N, M), (N, M // 32))]
    g = _run(F, c, M, N, K, torch.bfloat16, tile, relu=True, qout=(outs[0], outs[1]), qtout=(outs[2], outs[3]))
    O.assert_bits_equal(g.view, c["expected"], bm, bn)
    g.check()
    _assert_mx_copies(F, want, outs[:2], outs[2:], bm, bn)


def _assert_mx_copies(F, want, rows, transposed, bm, bn):
    """(q, s) pairs against the quantization of the exactly known bf16 output ``want`` [M][N]."""
    for (q, s), ref, tag in ((rows, want, "rows"), (transposed, want.t().contiguous(), "transposed")):
        q_ref, ex = F.quantize_mx_ref(ref)
        assert (ex > -127).all()                                   # (no all-zero block: its scale byte is not pinned)
        O.assert_bits_equal(s.cpu()[None], (ex + 127).to(torch.uint8)[None])
        O.assert_bits_equal(q.cpu()[None], q_ref.view(torch.uint8)[None], bm if tag == "rows" else bn,
                            bn if tag == "rows" else bm)


@pytest.mark.parametrize("K", [128, 384])
@pytest.mark.parametrize("fix", [1, 2])
def test_mx_gemm_fixed_epilogue_copies_are_exact(F, fix, K):
    """The FF block's two compile-time epilogues (tile 1282, no bf16 output, both MX copies): FIX 1 =
    ReLU, FIX 2 = the ReLU mask read from e4m3 bytes.  M = N = 160: a full block and a ragged one in
    each direction, the smallest size with whole 32-blocks along both.  The copies are contiguous,
    so each sits between two guard runs of its fill byte and every byte of it is compared."""
    M = N = 160
    guard = 4096
    c = O.mx_case(M, N, K, relu=fix == 1, out=torch.bfloat16, res=("mask", "e4m3") if fix == 2 else None, seed=fix + K)
    assert O.exactness(c) < 2 ** 20
    bufs = [torch.full((r * k + 2 * guard,), 0xAB, dtype=torch.uint8, device=dev)
            for r, k in ((M, N), (M, N // 32), (N, M), (N, M // 32))]
    outs = [b[guard:-guard].view(shape) for b, shape in zip(bufs, ((M, N), (M, N // 32), (N, M), (N, M // 32)))]
    _run(F, c, M, N, K, None, 1282, relu=fix == 1, qout=(outs[0], outs[1]), qtout=(outs[2], outs[3]))
    assert P.mx_name(1282, fix=fix) in _RAN
    _assert_mx_copies(F, c["expected"][0], outs[:2], outs[2:], 128, 128)
    for b in bufs:
        assert (b[:guard] == 0xAB).all() and (b[-guard:] == 0xAB).all()


@pytest.mark.parametrize("K,N,path", [(128, 64, "tiled"), (32, 8, "generic")])
def test_quant_cols_path_is_recorded_and_matches_reference(F, K, N, path):
    """ljs_quant_mx_cols picks the LDS-tiled kernel from the shape and the alignment: the record
    names the one that ran, and either equals the reference quantizer bit for bit."""
    from learning_jax_sharding_amd.ops import hip
    w = (torch.randn(K, N, generator=torch.Generator().manual_seed(K + N)) * 3).bfloat16()
    with hip.launch_log() as log:
        q, s = F.quant_cols(w.to(dev))
    torch.cuda.synchronize()
    assert [r["name"] for r in log] == [f"quant_mx_cols<{path}>"], log
    assert log[0]["grid"] == ((1, 1, 1) if path == "tiled" else (1, K // 32, 1)) and log[0]["block"] == (256 if path == "tiled" else 64)
    q_ref, ex = F.quantize_mx_ref(w.t().contiguous())
    O.assert_bits_equal(q.cpu()[None], q_ref.view(torch.uint8)[None])
    O.assert_bits_equal(s.cpu()[None], (ex + 127).to(torch.uint8)[None])


def test_mx_gemm_fused_column_sums_are_exact(F):
    """colsum (8-wave tiles): per row tile, the column sums of the bf16 values stored -- operands in
    [-2, 2], so the sums are exact in any order."""
    tile = 256160
    bm, bn = _bm_bn(tile)
    M, N, K = bm + 8, bn + 8, 128
    c = O.mx_case(M, N, K, lo=-2, hi=2, out=torch.bfloat16, seed=7)
    cs = torch.full((-(-M // bm), N), float("nan"), device=dev)
    g = _run(F, c, M, N, K, torch.bfloat16, tile, colsum=cs)
    O.assert_bits_equal(g.view, c["expected"], bm, bn)
    g.check()
    want = torch.stack([c["expected"][0, r:r + bm].double().sum(0) for r in range(0, M, bm)])
    assert float(want.abs().max()) * 4 < 2 ** 24
    O.assert_bits_equal(cs.cpu()[None], want.float()[None])


@pytest.mark.parametrize("tile", _TWO)
def test_mx_gemm_gaussian_inside_derived_bound(F, tile):
    """N(0, 1) data quantized on the CPU (quantize_mx_ref), against the float64 product of the
    dequantized operands: |got - oracle| <= (K + 2) 2^-24 sum_k |a_k b_k|, every element."""
    bm, bn = _bm_bn(tile)
    M, N, K = bm + 8, bn + 8, 384
    gen = torch.Generator().manual_seed(tile % 977)
    c = dict(bias=None, res=None, res_mode="add")
    deq = []
    for n, R in (("a", M), ("b", N)):
        q, ex = F.quantize_mx_ref(torch.randn(R, K, generator=gen))
        c["q" + n], c["s" + n] = q.view(torch.uint8), (ex + 127).to(torch.uint8)
        deq.append(F.dequantize_mx_ref(q, ex).double())
    oracle = deq[0] @ deq[1].t()
    bound = (K + 2) * 2.0 ** -24 * (deq[0].abs() @ deq[1].abs().t())
    g = _run(F, c, M, N, K, torch.float32, tile)
    err = (g.view[0].double().cpu() - oracle).abs()
    print(f"gemm-figures mx-gauss-{tile:<7d} M,N,K {M},{N},{K} max|err| {err.max().item():.3e} "
          f"max err/bound {(err / bound).max().item():.3f}")
    assert (err <= bound).all()
    g.check()


def test_every_instance_ran():
    """Last in the file: the records of the cases above name every instance fp8.hip instantiates."""
    assert _RAN == P.INSTANCES - set(P.UNREACHABLE), sorted(_RAN ^ P.INSTANCES)
