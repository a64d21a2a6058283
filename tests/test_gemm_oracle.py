"""The GEMM oracle's case table on the CPU (tests/gemm_oracle.py; the GPU half is
tests/test_gemm_oracle_gpu.py): every row's plan names the instance the row claims, the claims are
the whole of what the tile table instantiates, the exactness condition holds for every row, and
the oracle itself is checked against scalar arithmetic.  Needs the built library, not a GPU."""
import os

import pytest
import torch

import gemm_oracle as O
from learning_jax_sharding_amd.ops import hip


@pytest.fixture(scope="module")
def planned():
    if not os.path.exists(hip._LIBPATH):
        from learning_jax_sharding_amd.csrc import build
        build.build_all()
    hip.lib()


def _slots_256(probe):
    return hip.gemm_plan(**probe, cus=256)["grid"][0]


def _all_rows():
    return O.TABLE + O.persistent_rows(_slots_256)


def test_every_row_plans_the_instance_it_claims(planned):
    for row in _all_rows():
        c = O.case(**row["call"])
        plan = hip.gemm_plan(**O.plan_args(row, c))
        name, variant = row["claim"]
        assert plan["err"] == 0, (row["id"], plan)
        if row["kind"] == "group2":
            # the grouped pair runs the plain slab instance's grouped kernel: both GEMMs groupable
            # slab plans of one instance
            p1 = hip.gemm_plan(**O.plan_args(dict(row, call=row["call1"])))
            assert plan["family"] == p1["family"] == "slab" and plan["name"] == p1["name"], (row["id"], plan, p1)
            assert name == plan["name"].replace("gemm_dma<", "gemm_dma_group2<") and p1["splitk"] == row["splitk1"]
        else:
            assert plan["name"] == name, (row["id"], plan["name"], name)
        assert plan["variant"] == variant and plan["resolved_tile"] == row["resolved"], (row["id"], plan)
        assert plan["splitk"] == row["splitk"] == c["splits"], (row["id"], plan)
        if "launched" in row:
            assert (plan["N"], plan["batch"]) == row["launched"], (row["id"], plan)
        if row.get("psum"):
            assert plan["psum_count"] == plan["blocks"] * plan["WM"] * plan["WN"] > 0, (row["id"], plan)
        if row["kind"] == "persistent":
            items = 4 * row["call"]["batch"]
            assert plan["grid"][0] == row["slots"] and items == 2 * row["slots"], (row["id"], plan)


def test_claims_cover_every_instantiated_kernel():
    inst = O.instantiated()
    assert len(inst) == 122 + 16                      # LDS-DMA / lean / grouped instances + register-staged
    claims = {row["claim"] for row in O.TABLE}
    assert O.UNREACHABLE <= inst and not (claims & O.UNREACHABLE)
    assert claims == inst - O.UNREACHABLE, (sorted(inst - O.UNREACHABLE - claims, key=str), sorted(claims - inst, key=str))
    assert len({row["id"] for row in O.TABLE}) == len(O.TABLE)


def test_unreachable_instances_are_demoted_by_the_plan(planned):
    """The short list is a fact about the plan, not a convenience: a call with an epilogue operand
    on the KK = 3 tiles runs another tile, general or lean kernel asked for."""
    for code, to in ((644, 64), (2562, 1282)):
        for force in (0, 100000, 200000):
            for rd in (torch.bfloat16, torch.float32):
                plan = hip.gemm_plan(264, 200, 128, 128, 128, 200, True, True, False, tile=code + force, res_dtype=rd,
                                     res_ld=200)
                assert plan["err"] == 0 and plan["resolved_tile"] == to, plan


def test_exactness_holds_for_every_row():
    worst = 0.0
    for row in _all_rows():
        c = O.case(**row["call"])
        if c["gaussian"]:
            continue
        worst = max(worst, O.exactness(c))
        assert O.exactness(c) < 2 ** 24, row["id"]
        if row["kind"] == "group2":
            assert O.exactness(O.case(**row["call1"])) < 2 ** 24
    assert worst < 2 ** 16                             # room to spare
    # ... and the rounding is under test: a good share of the bf16 outputs are not bf16 numbers
    c = O.case(136, 136, 640)
    rounded = (c["expected"].double() != c["oracle"]).double().mean().item()
    assert float(c["oracle"].abs().max()) > 1024 and rounded > 0.3, rounded


def test_mx_exactness():
    for K in (128, 384, 512):
        for lo, hi in ((-8, 8), (-2, 2)):
            c = O.mx_case(136, 72, K, lo, hi, bias=True, res=("add", "bf16"), out=torch.bfloat16)
            assert O.exactness(c) < 2 ** 20
            assert O._grain(c["oracle"]) >= 0.25
    c = O.mx_case(136, 72, 256, out=torch.bfloat16)
    assert (c["expected"].double() != c["oracle"]).double().mean().item() > 0.5
    sa = O.mx_operand(torch.Generator().manual_seed(1), 64, 256)[1]
    assert set(sa.unique().tolist()) == {126, 127, 128}


# ============================================================================ the oracle's own checks
def test_oracle_identity_and_one_hot():
    c = O.case(8, 8, 8)
    # put an identity / a one-hot selection through the same storage + product path
    eye = torch.eye(8, dtype=torch.float64)
    B = c["B"].double().reshape(8, 8).t()              # stored [N][K] -> logical [K][N]
    assert torch.equal(eye @ B, B)
    A = c["A"].double().reshape(8, 8)
    assert torch.equal(c["oracle"][0], A @ B)
    pick = torch.zeros(3, 8, dtype=torch.float64)
    pick[0, 5] = pick[1, 0] = pick[2, 7] = 1
    assert torch.equal(pick @ B, B[[5, 0, 7]])
    # m/n-contiguous storage holds the transposes
    d = O.case(8, 16, 8, a_kc=False, b_kc=False, seed=c["call"]["M"])
    A2, B2 = d["A"].double().reshape(8, 8).t(), d["B"].double().reshape(8, 16)
    assert torch.equal(d["oracle"][0], A2 @ B2)


def _bf16(x):
    return float(torch.tensor(x, dtype=torch.float32).bfloat16())


@pytest.mark.parametrize("kw", [
    dict(alpha=0.5, bias=torch.float32, relu=True), dict(alpha=2.0, bias=torch.bfloat16),
    dict(res=("add", torch.bfloat16, False), alpha=0.5), dict(res=("mask", torch.float32, False), bias=torch.float32),
    dict(res=("add", torch.float32, True)), dict(out=torch.float32, accumulate=True, alpha=0.5),
    dict(out=torch.float32, bias=torch.float32, relu=True)])
def test_epilogue_formulas_against_a_scalar_loop(kw):
    M = N = K = 3
    c = O.case(M, N, K, seed=11, lo=-300, hi=300, **kw)      # (large enough that bf16 rounds)
    A, B = c["A"].reshape(M, K).tolist(), c["B"].reshape(N, K).tolist()
    bias = c["bias"].tolist() if c["bias"] is not None else [0.0] * N
    res, alpha = kw.get("res"), kw.get("alpha", 1.0)
    for i in range(M):
        for j in range(N):
            y = alpha * sum(A[i][k] * B[j][k] for k in range(K)) + bias[j]
            if kw.get("relu"):
                y = max(y, 0.0)
            if kw.get("accumulate"):
                y += float(c["c_init"][0, i, j])
            if kw.get("out") == torch.float32:
                want = y
            elif res is None:
                want = _bf16(y)
            else:
                r = float(c["res"][0 if res[2] else i, j])
                want = _bf16(_bf16(y) + _bf16(r)) if res[0] == "add" else (_bf16(y) if r > 0 else 0.0)
            got = float(c["expected"][0, i, j])
            assert got == want and (want != 0 or str(got) == "0.0"), (i, j, got, want)     # (masked: +0)


# ============================================================================ the comparison itself
def test_guarded_and_report_catch_mutations():
    """The mutation check: a flipped bit, a zeroed 16-row band and a truncating store each fail the
    comparison, and the report points at the place; a stray write fails the guard check."""
    c = O.case(136, 72, 640)
    want = c["expected"]
    O.assert_bits_equal(want.clone(), want, 128, 128)
    # one bit of one element
    got = want.clone()
    got.view(torch.int16)[0, 129, 70] ^= 1
    with pytest.raises(AssertionError, match=r"1 of 9792 elements differ.*\n.*row 129, col 70.*row % 128 = 1, col % 128 = 70"):
        O.assert_bits_equal(got, want, 128, 128)
    # a 16-row band
    got = want.clone()
    got[0, 32:48] = 0
    rep = O.mismatch_report(got, want, 128, 128)
    bad = (got.view(torch.int16) != want.view(torch.int16))
    assert set(bad.nonzero()[:, 1].tolist()) <= set(range(32, 48)) and "in 16 rows 32..47 and" in rep and "row 32," in rep
    with pytest.raises(AssertionError):
        O.assert_bits_equal(got, want, 128, 128)
    # truncation instead of round-to-nearest-even
    trunc = (c["oracle"].float().view(torch.int32) & -65536).view(torch.float32).bfloat16()
    assert O.mismatch_report(trunc, want, 128, 128).startswith(f"{int((trunc != want).sum())} of 9792")
    assert (trunc != want).float().mean().item() > 0.15
    # guards
    view, g = O.guarded((2, 5, 8), torch.bfloat16)
    assert view.shape == (2, 5, 8) and g.ld == 16 and g.sC == 13 * 16 and g.c_off == 4 * 16
    g.check(written=False)
    with pytest.raises(AssertionError, match="never written"):
        g.check()
    view.copy_(torch.ones(2, 5, 8))
    g.check()
    g.buf[1, 3, 2] = 1.0                                # the row before the view
    with pytest.raises(AssertionError, match=r"1 guard elements overwritten.*\(1, 3, 2\)"):
        g.check()
    view32, g32 = O.guarded((5, 8), torch.float32)
    assert g32.buf.view(torch.int32)[0, 0, 0].item() == 0x7FC00001 and g.buf.view(torch.int16)[0, 0, 0].item() == 0x7FC1
    view32.zero_()
    g32.buf[0, 4, 8] = 0.0                              # the column after the view
    with pytest.raises(AssertionError, match=r"\(0, 4, 8\)"):
        g32.check()
