"""The MX-fp8 GEMM launcher's instance choice, pinned on the CPU: ljs_gemm_mx_plan (fp8.gemm_mx_plan)
is the plan step ljs_gemm_mx_fp8 itself runs -- checks, tile, kernel instance, split, grid, block -- as
a pure function, so the built library answers it without a GPU.  The tile table, the instance names
and the case lists here are the ones tests/test_fp8_gemm_oracle_gpu.py uses, imported and not copied."""
import itertools
import os

import pytest

from learning_jax_sharding_amd.ops import fp8 as F
from learning_jax_sharding_amd.ops import hip

# LJS_MX_TILES (csrc/kernels/fp8.hip) restated as data: code: (family, BM, BN, WM, NST)
MX_TILES = {
    1282: ("4-wave", 128, 128, 2, 2), 1283: ("4-wave", 128, 128, 2, 3),
    2562: ("4-wave", 256, 128, 4, 2), 2563: ("4-wave", 256, 128, 4, 3),
    256256: ("8-wave", 256, 256, 2, 2), 256128: ("8-wave", 256, 128, 2, 2), 256160: ("8-wave", 256, 160, 4, 2),
    128320: ("8-wave", 128, 320, 2, 2), 128256: ("8-wave", 128, 256, 2, 2), 128128: ("8-wave", 128, 128, 2, 2),
    128160: ("8-wave", 128, 160, 4, 2), 3128128: ("8-wave", 128, 128, 2, 3), 3128160: ("8-wave", 128, 160, 4, 3),
    3128256: ("8-wave", 128, 256, 2, 3), 3256128: ("8-wave", 256, 128, 2, 3),
}
RELU, BIAS, BIAS_F32, OUT_F32 = F.MX_RELU, F.MX_BIAS, F.MX_BIAS_F32, F.MX_OUT_F32
RES_ADD, RES_MASK, QC, QT, E4M3, COLSUM = F.MX_RES_ADD, F.MX_RES_MASK, F.MX_QC, F.MX_QT, F.MX_RES_E4M3, F.MX_COLSUM
FIX1, FIX2, FIX3 = RELU | QC | QT, RES_MASK | E4M3 | QC | QT, OUT_F32


def mx_name(code, out_f32=False, fix=0):
    fam, bm, bn, wm, nst = MX_TILES[code]
    if fam == "4-wave":
        return f"gemm_mx_fp8<{bm},{nst},fix={fix}>"
    return f"gemm_mx8<{bm},{bn},{wm},{'f32' if out_f32 else 'bf16'},{nst}>"


# the 29 instances fp8.hip instantiates: 4 + 3 of the 4-wave kernel, 11 8-wave tiles x {bf16, f32}
INSTANCES = ({mx_name(c) for c, t in MX_TILES.items() if t[0] == "4-wave"}
             | {mx_name(1282, fix=f) for f in (1, 2, 3)}
             | {mx_name(c, of) for c, t in MX_TILES.items() if t[0] == "8-wave" for of in (False, True)})
UNREACHABLE = {}     # name: reason -- every instance is reachable through gemm_mx


@pytest.fixture(scope="module")
def planned():
    if not os.path.exists(hip._LIBPATH):
        from learning_jax_sharding_amd.csrc import build
        build.build_all()
    hip.lib()


def _cdiv(a, b):
    return -(-a // b)


def tile_cases():
    """(tile, flags, M, N, K, nsplit, addr): every code at one ragged block in each direction, both
    output types, one and two splits (a bf16 output has no split: those are rejections)."""
    for code, (_, bm, bn, _, _) in MX_TILES.items():
        for flags, nsplit in itertools.product((OUT_F32, 0), (1, 2)):
            yield code, flags, bm + 8, bn + 8, 384, nsplit, {}


def fix_cases():
    """(tile, flags, M, N, K, nsplit, addr, fix): the four FIX conditions and their near misses."""
    s = (160, 160, 128)
    no_c = dict(C=0)
    for tile in (0, 1282):
        yield (tile, FIX1, *s, 1, no_c, 1)
        yield (tile, FIX2, *s, 1, no_c, 2)
        yield (tile, FIX3, *s, 1, {}, 3)
    yield (1282, FIX3, 160, 160, 384, 2, {}, 3)                  # any split count
    yield (1282, FIX1, *s, 1, {}, 0)                             # a bf16 output as well
    yield (1282, FIX2, *s, 1, {}, 0)
    yield (1282, FIX1, *s, 1, dict(C=0, bias=4096), 0)           # a bias pointer (even unused)
    yield (1282, FIX2, *s, 1, dict(C=0, bias=4096), 0)
    yield (1282, FIX3, *s, 1, dict(bias=4096), 0)
    yield (1282, FIX1 | BIAS, *s, 1, no_c, 0)                    # one more flag
    yield (1282, FIX1 | RES_MASK, *s, 1, no_c, 0)
    yield (1282, FIX1 & ~QT, *s, 1, no_c, 0)                     # ... or one fewer
    yield (1282, FIX2 | RELU, *s, 1, no_c, 0)
    yield (1282, FIX2 & ~E4M3, *s, 1, no_c, 0)                   # (a bf16 mask)
    yield (1282, FIX3 | RELU, *s, 1, {}, 0)
    yield (1282, FIX3 | BIAS | BIAS_F32, *s, 1, {}, 0)
    yield (1282, FIX3 | QC, *s, 1, {}, 0)
    for tile in (1283, 2562, 2563):                              # the FIX instances exist at 1282 only
        yield (tile, FIX1, 288, 160, 128, 1, no_c, 0)
        yield (tile, FIX2, 288, 160, 128, 1, no_c, 0)
        yield (tile, FIX3, 288, 160, 128, 1, {}, 0)


def parent_launch(tile, flags, c_null, bias_null, nsplit, M, N):
    """(instance, grid, block) by the launcher this plan replaced -- its tile-code arithmetic, its
    launch_mx8 / launch_f8 conditions and its two grid computations, transcribed from that source
    (with its bare flag numbers), not from the plan under test."""
    if tile == 0:
        tile = 1282
    if tile >= 10000:
        t6 = tile % 1000000
        bm, bn = t6 // 1000, t6 % 1000
        wm, nst = (4 if bn == 160 else 2), (3 if tile >= 1000000 else 2)       # its switch's template arguments
        return (f"gemm_mx8<{bm},{bn},{wm},{'f32' if flags & 32 else 'bf16'},{nst}>",
                _cdiv(M, bm) * _cdiv(N, bn) * nsplit, 512)
    bm = 256 if tile // 10 >= 256 else 128
    grid = _cdiv(M, bm) * _cdiv(N, 128) * nsplit
    BM, NST = {1283: (128, 3), 2562: (256, 2), 2563: (256, 3)}.get(tile, (128, 2))
    fix = 0
    if (BM, NST) == (128, 2) and c_null and bias_null and nsplit == 1 and flags in (1 | 256 | 512, 128 | 1024 | 256 | 512):
        fix = 1 if flags == (1 | 256 | 512) else 2
    elif (BM, NST) == (128, 2) and flags == 32 and bias_null:
        fix = 3
    return f"gemm_mx_fp8<{BM},{NST},fix={fix}>", grid, BM * 2


def _plan(tile, flags, M, N, K, nsplit, addr):
    return F.gemm_mx_plan(M, N, K, flags, tile=tile, nsplit=nsplit, **addr)


# ============================================================================ the tile table
def test_every_tile_code_plans_its_own_instance(planned):
    assert len(MX_TILES) == 15 and len(INSTANCES) == 29
    for code, flags, M, N, K, nsplit, addr in tile_cases():
        plan = _plan(code, flags, M, N, K, nsplit, addr)
        if nsplit > 1 and not flags & OUT_F32:
            assert plan["err"] != 0 and plan["name"] == "", plan        # only f32 slabs are split
            continue
        fam, bm, bn, wm, nst = MX_TILES[code]
        fix = (3 if code == 1282 and flags == OUT_F32 else 0) if fam == "4-wave" else None
        assert plan["err"] == 0 and plan["name"] == mx_name(code, bool(flags & OUT_F32), fix or 0), plan
        assert (plan["family"], plan["BM"], plan["BN"], plan["WM"], plan["NST"]) == (fam, bm, bn, wm, nst), plan
        assert plan["resolved_tile"] == code and plan["fix"] == fix == plan["variant"], plan
        assert plan["block"] == (bm * 2 if fam == "4-wave" else 512), plan
        assert plan["blocks"] == _cdiv(M, bm) * _cdiv(N, bn) * nsplit == 4 * nsplit, plan
        assert plan["grid"] == (4 * nsplit, 1, 1) and plan["out_f32"] == bool(flags & OUT_F32)
        assert (plan["nsplit"], plan["splitk"], plan["kps"]) == (nsplit, nsplit, 3 if nsplit == 1 else 2), plan


def test_tile_zero_is_1282(planned):
    for flags in (0, OUT_F32, RELU | BIAS):
        zero, named = (F.gemm_mx_plan(136, 136, 384, flags, tile=t) for t in (0, 1282))
        assert zero == named and zero["resolved_tile"] == 1282 and zero["err"] == 0


# ============================================================================ the FIX instances
def test_fix_conditions_and_their_near_misses(planned):
    seen = set()
    for tile, flags, M, N, K, nsplit, addr, fix in fix_cases():
        plan = _plan(tile, flags, M, N, K, nsplit, addr)
        code = tile or 1282
        assert plan["err"] == 0 and plan["fix"] == fix and plan["name"] == mx_name(code, fix=fix), (tile, flags, addr, plan)
        assert plan["resolved_tile"] == code and plan["nsplit"] == nsplit
        seen.add(fix)
    assert seen == {0, 1, 2, 3}
    # a second split turns the two copy-only calls into errors (only f32 slabs are split)
    for flags in (FIX1, FIX2):
        assert F.gemm_mx_plan(160, 160, 384, flags, tile=1282, nsplit=2, C=0)["err"] != 0


# ============================================================================ rejections
def _err(M=160, N=160, K=128, flags=0, tile=1282, nsplit=1, **kw):
    return F.gemm_mx_plan(M, N, K, flags, tile=tile, nsplit=nsplit, **kw)["err"]


def test_rejections_the_launcher_always_had(planned):
    assert _err() == 0
    assert _err(K=64) and _err(N=164) and _err(ldc=164)
    assert _err(M=1 << 24) and _err(N=1 << 24)                    # M K, N K >= 2^31
    for res in (RES_ADD, RES_MASK):
        assert _err(flags=res) == 0
        assert _err(flags=res, R=0) and _err(flags=res, ldr=164) and _err(flags=res, R=4104)
        assert _err(flags=res | OUT_F32)
    assert _err(flags=E4M3) and _err(flags=E4M3 | RES_MASK) == 0
    assert _err(flags=QC) == 0 and _err(flags=QC, QC=0) and _err(flags=QC, SC=0) and _err(flags=QC, N=168)
    assert _err(flags=QT) == 0 and _err(flags=QT, QT=0) and _err(flags=QT, ST=0) and _err(flags=QT, M=168)
    assert _err(flags=QT, ldqt=128) and _err(flags=QT, ldqt=176) and _err(flags=QT | OUT_F32) and _err(flags=QT, QT=4104)
    # split-K: f32 slabs with nothing else, and a slab count that is exact
    assert _err(K=384, flags=OUT_F32, nsplit=2) == 0 == _err(K=384, flags=OUT_F32, nsplit=3)
    assert _err(K=384, nsplit=2) and _err(K=384, flags=OUT_F32 | BIAS, nsplit=2) and _err(K=384, flags=OUT_F32 | QC, nsplit=2)
    assert _err(K=384, flags=RES_ADD, nsplit=2) and _err(K=384, flags=QT, nsplit=2)
    assert _err(K=512, flags=OUT_F32, nsplit=3)                   # 4 K-tiles in 3 splits of 2: only 2 slabs
    assert _err(K=384, flags=OUT_F32, nsplit=0) == 0              # (no split)
    # fused column sums: an 8-wave tile's bf16 epilogue
    assert _err(flags=COLSUM, tile=256160) == 0 == _err(flags=COLSUM, tile=256160, C=0)
    assert _err(flags=COLSUM, tile=256160, csum=0) and _err(flags=COLSUM | OUT_F32, tile=256160)
    assert _err(flags=COLSUM, tile=1282) and _err(flags=COLSUM, tile=0)
    assert _err(tile=256192) and _err(tile=2128128) and _err(tile=10000)      # no such 8-wave tile


def test_rejections_of_what_no_instance_honours(planned):
    """Calls the launcher used to accept and a kernel then ran differently from what was asked."""
    for tile in (1284, 2561, 1602, 643, 7, 9999, -1):              # ran as <128, 2>: 1284 is a bf16 tile code
        assert _err(tile=tile), tile
    # the 8-wave f32 instance returns after its f32 stores; the 4-wave kernel writes the copy
    for tile, (fam, *_rest) in MX_TILES.items():
        assert bool(_err(flags=OUT_F32 | QC, tile=tile)) == (fam == "8-wave"), tile
    assert F.gemm_mx_plan(160, 160, 128, OUT_F32 | QC, tile=1282)["fix"] == 0
    assert _err(flags=RES_ADD | RES_MASK) and _err(flags=RES_ADD | RES_MASK | E4M3)     # the epilogues take one
    assert _err(flags=BIAS_F32) and _err(flags=BIAS | BIAS_F32) == 0                    # read only under BIAS
    assert _err(flags=8) and _err(flags=16) and _err(flags=4096) and _err(flags=1 << 30)      # bits no kernel reads
    assert _err(K=384, flags=OUT_F32 | RELU, nsplit=2) and _err(K=384, flags=OUT_F32 | RELU) == 0   # a ReLU per partial
    assert _err(flags=BIAS, bias=0) and _err(flags=OUT_F32, C=0)                        # an operand that is not there
    assert _err(C=0) == 0                                                               # (a bf16 call may want copies only)


# ============================================================================ coverage, preserved behaviour
def _all_cases():
    return [c + (None,) for c in tile_cases()] + list(fix_cases())


def test_the_cases_reach_exactly_the_instantiated_instances(planned):
    names = {p["name"] for p in (_plan(*c[:7]) for c in _all_cases()) if p["err"] == 0}
    assert names == INSTANCES - set(UNREACHABLE) and not UNREACHABLE, sorted(names ^ INSTANCES)


def test_plan_launches_what_the_previous_launcher_did(planned):
    n = 0
    for tile, flags, M, N, K, nsplit, addr, _ in _all_cases():
        plan = _plan(tile, flags, M, N, K, nsplit, addr)
        if plan["err"]:
            continue
        want = parent_launch(tile, flags, addr.get("C", 4096) == 0, addr.get("bias", 4096 if flags & BIAS else 0) == 0,
                             nsplit, M, N)
        assert (plan["name"], plan["blocks"], plan["block"]) == want, (tile, flags, addr, nsplit, plan, want)
        n += 1
    assert n == 15 * 3 + len(list(fix_cases()))


# ============================================================================ the automatic tile
def test_auto_tile_at_the_ff_block_shapes():
    assert F._auto_tile(16384, 640, 2560, 0, 1) == 256160 == F._auto_tile(16384, 640, 2560, RES_ADD, 1)
    assert F._auto_tile(16384, 640, 2560, QC, 1) == 0 == F._auto_tile(16384, 640, 2560, QT, 1)
    assert F._auto_tile(16384, 640, 2560, RELU | QC | QT, 1) == 0
    assert F._auto_tile(16384, 640, 2560, 0, 2) == 0
    assert F._auto_tile(2048, 640, 2560, 0, 1) == 0 == F._auto_tile(2048, 640, 2560, RES_ADD, 1)
    assert F._auto_tile(16384, 2560, 640, 0, 1) == 0              # the up projection's shape
    assert (RELU, BIAS, BIAS_F32, OUT_F32, RES_ADD, RES_MASK, QC, QT, E4M3, COLSUM) == (1, 2, 4, 32, 64, 128, 256, 512, 1024, 2048)


def test_mx_flags_states_a_call():
    import torch
    assert F.mx_flags(torch.float32) == OUT_F32 and F.mx_flags(torch.bfloat16) == 0 == F.mx_flags(None)
    assert F.mx_flags(torch.bfloat16, torch.float32, True) == RELU | BIAS | BIAS_F32
    assert F.mx_flags(torch.bfloat16, torch.bfloat16) == BIAS
    assert F.mx_flags(None, relu=True, qout=True, qtout=True) == FIX1
    assert F.mx_flags(None, res_dtype=torch.uint8, res_mode="mask", qout=True, qtout=True) == FIX2
    assert F.mx_flags(torch.bfloat16, res_dtype=torch.bfloat16) == RES_ADD
    assert F.mx_flags(torch.bfloat16, res_dtype=torch.bfloat16, res_mode="mask", colsum=True) == RES_MASK | COLSUM
