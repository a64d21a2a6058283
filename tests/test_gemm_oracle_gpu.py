"""Every GEMM kernel instance of csrc/kernels/gemm.hip against the exact-arithmetic oracle of
tests/gemm_oracle.py (run on a real MI355X: -m gpu).  Each row of the oracle's case table runs
into a C that lies inside a larger NaN-payload buffer, under the launch log: the record must name
the instance the row claims, the output must equal the expected bits (integer views, no
tolerance anywhere) and every guard element must be untouched.  The Gaussian rows are held to the
derived forward-error bound and print one ``gemm-figures`` line each (profiles/gemm/figures.txt)."""
import pytest
import torch

import gemm_oracle as O

pytestmark = pytest.mark.gpu

dev = torch.device("cuda", 0)


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from learning_jax_sharding_amd.ops import hip as H
    H.lib()
    return H


def _rows(kind):
    return [pytest.param(r, id=r["id"]) for r in O.TABLE if r["kind"] == kind]


def _guarded_for(row, c):
    k = c["call"]
    if c["fold"]:    # weight-major batches side by side: ldc = N * batch leaves no room for guard columns
        return O.Guarded((1, k["M"], k["N"] * k["batch"]), c["out"], dev, pad=0)
    return O.Guarded((c["nb"], k["M"], k["N"]), c["out"], dev, pad=row.get("pad", 8))


def _launch(hip, row, c, g, psum=None):
    """The row's call with C = the guarded view (through c_off, inside the whole buffer)."""
    k = c["call"]
    bias = None if c["bias"] is None else c["bias"].to(dev)[c["bias_skew"]:]
    res = None if c["res"] is None else c["res"].to(dev)
    ldc, sC = (k["N"] * k["batch"], k["N"]) if c["fold"] else (g.ld, g.sC)
    if c["c_init"] is not None:
        g.view.copy_(c["c_init"].to(c["out"]))
    keep = (c["A"].to(dev), c["B"].to(dev), bias, res)
    cnt = hip.gemm(keep[0], keep[1], g.buf, k["M"], k["N"], k["K"], k["lda"], k["ldb"], ldc, k["a_kc"], k["b_kc"],
                   batch=k["batch"], sA=k["sA"], sB=k["sB"], sC=sC, bias=bias, sBias=k["sBias"], relu=k["relu"],
                   alpha=k["alpha"], accumulate=k["accumulate"], splitk=k["splitk"], tile=row["tile"], a_off=k["a_off"],
                   b_off=k["b_off"], c_off=g.c_off, psum=psum, res=res, res_ld=k["res_ld"], res_mode=k["res_mode"],
                   sR=k["sR"], slabs=k["slabs"])
    return cnt, keep


def _check_record(rec, row):
    name, variant = row["claim"]
    assert rec["name"] == name and rec["variant"] == variant, (row["id"], rec)
    assert rec["requested_tile"] == row["tile"] and rec["resolved_tile"] == row["resolved"], (row["id"], rec)
    assert rec["splitk"] == row["splitk"], (row["id"], rec)


def _tile_of(row):
    if row["resolved"] in O.TILES:
        return O.TILES[row["resolved"]][:2]
    return row["resolved"], row["resolved"]


def _run(hip, row, psum=None):
    c = O.case(**row["call"])
    g = _guarded_for(row, c)
    with hip.launch_log() as log:
        cnt, keep = _launch(hip, row, c, g, psum)
    torch.cuda.synchronize()
    assert log.total == 1
    _check_record(log[0], row)
    return c, g, log[0], cnt


@pytest.mark.parametrize("row", _rows("gemm"))
def test_gemm_instance_is_exact(hip, row):
    psum = None
    if row.get("psum"):
        k = row["call"]
        psum = torch.full((hip.psum_slots(k["M"], k["N"], 1),), float("nan"), device=dev)
    c, g, rec, cnt = _run(hip, row, psum)
    O.assert_bits_equal(g.view, c["expected"], *_tile_of(row))
    g.check()
    if row.get("psum"):
        # the fused output sums: one exact partial per (item, wave), of the bf16 values stored
        plan = hip.gemm_plan(**O.plan_args(row, c), cus=hip._cus())
        assert cnt == plan["psum_count"] == rec["blocks"] * plan["WM"] * plan["WN"] > 0
        assert psum[:cnt].double().sum().item() == g.view.double().sum().item() == c["expected"].double().sum().item()
        assert torch.isnan(psum[cnt:]).all()
    if c["call"]["slabs"]:
        # slab_reduce of the exact slabs is the whole product
        k = c["call"]
        slabs = g.view.contiguous()
        out = torch.full((1, k["M"], k["N"]), float("nan"), device=dev)
        hip.slab_reduce(slabs, out, k["N"], k["M"] * k["N"])
        torch.cuda.synchronize()
        O.assert_bits_equal(out, c["oracle"].sum(0, keepdim=True).float())


@pytest.mark.parametrize("row", _rows("group2"))
def test_gemm_grouped_pair_is_exact(hip, row):
    """A closed group of two slab GEMMs: one launch of the grouped kernel, every slab of both exact."""
    cs = [O.case(**row["call"]), O.case(**row["call1"])]
    gs = [_guarded_for(row, c) for c in cs]
    with hip.launch_log() as log:
        hip.gemm_group_begin()
        keep = [_launch(hip, row, c, g) for c, g in zip(cs, gs)]
        hip.gemm_group_end(gs[0].buf)
    torch.cuda.synchronize()
    assert log.total == 1 and keep
    _check_record(log[0], row)
    assert log[0]["splitk1"] == row["splitk1"]
    bm, bn = _tile_of(row)
    assert log[0]["blocks"] == sum(-(-c["call"]["M"] // bm) * -(-c["call"]["N"] // bn) * c["splits"] for c in cs)
    for c, g in zip(cs, gs):
        O.assert_bits_equal(g.view, c["expected"], bm, bn)
        g.check()


@pytest.mark.parametrize("req", [1282, 201282, 2561, 202561])
def test_gemm_persistent_walk_is_exact(hip, req):
    """A grid smaller than the item count: every block walks two items, the second item's first
    K-tiles in flight under the first one's epilogue, the accumulators cleared in between."""
    rows = O.persistent_rows(lambda probe: hip.gemm_plan(**probe, cus=hip._cus())["grid"][0])
    row = next(r for r in rows if r["tile"] == req)
    c, g, rec, _ = _run(hip, row)
    items = 4 * row["call"]["batch"]
    assert rec["grid"][0] == row["slots"] < items == 2 * row["slots"], (rec, row["slots"])
    assert g.buf.numel() * g.buf.element_size() < 32 << 20
    O.assert_bits_equal(g.view, c["expected"], *_tile_of(row))
    g.check()


@pytest.mark.parametrize("row", _rows("gauss"))
def test_gemm_gaussian_inside_derived_bound(hip, row):
    """N(0, 1) operands and alpha = 0.37: the low mantissa bits integers never exercise.  Bound
    (tests/gemm_oracle.py case): (K + 2) 2^-24 (|alpha| sum_k |a_k b_k| + |bias|), plus 2^-8 |oracle|
    for a bf16 output; a residual add rounds twice and its bound carries both roundings (derived in
    tests/gemm_oracle.py case) -- every element checked; the printed figure is a record."""
    c, g, rec, _ = _run(hip, row)
    err = (g.view.double().cpu() - c["oracle"]).abs()
    frac = (err / c["bound"]).max().item()
    k = c["call"]
    print(f"gemm-figures {row['id']:18s} {rec['name']:40s} variant {rec['variant']} M,N,K {k['M']},{k['N']},{k['K']} "
          f"max|err| {err.max().item():.3e} max err/bound {frac:.3f}")
    assert torch.isfinite(err).all() and (err <= c["bound"]).all(), frac
    g.check()


@pytest.mark.parametrize("bad", ["relu", "bias"])
@pytest.mark.parametrize("slabs", [False, True])
def test_split_call_with_bias_or_relu_raises_and_writes_nothing(hip, monkeypatch, bad, slabs):
    row = dict(tile=1282, pad=8)
    c = O.case(136, 72, 256, a_kc=False, b_kc=False, out=torch.float32, splitk=2, slabs=slabs, accumulate=not slabs)
    g = _guarded_for(row, c)
    k = c["call"]
    A, B = c["A"].to(dev), c["B"].to(dev)
    bias = torch.ones(72, device=dev) if bad == "bias" else None
    kw = dict(sC=g.sC, splitk=2, tile=1282, c_off=g.c_off, slabs=slabs)
    n = hip.lib().ljs_launch_count()
    with pytest.raises(AssertionError, match="no bias and no ReLU"):
        hip.gemm(A, B, g.buf, 136, 72, 256, k["lda"], k["ldb"], g.ld, False, False, relu=bad == "relu", bias=bias, **kw)
    # the launcher itself: the same flags past the wrapper's assertion
    flags = hip._gemm_flags
    monkeypatch.setattr(hip, "_gemm_flags", lambda *a: flags(*a) | (1 if bad == "relu" else 2 | 4))
    with pytest.raises(RuntimeError, match="hipError 1"):
        hip.gemm(A, B, g.buf, 136, 72, 256, k["lda"], k["ldb"], g.ld, False, False, zero_c=not slabs, **kw)
    torch.cuda.synchronize()
    assert hip.lib().ljs_launch_count() == n
    g.check(written=False)


def test_gemm_f32_is_exact(hip):
    gen = torch.Generator().manual_seed(5)
    A = torch.randint(-8, 9, (3, 20, 36), generator=gen).float()
    B = torch.randint(-8, 9, (3, 36, 12), generator=gen).float()
    view, g = O.guarded((3, 20, 12), torch.float32, dev)
    Ad, Bd = A.to(dev), B.to(dev)
    with hip.launch_log() as log:
        hip._gemm_f32(Ad, Bd, view, 20, 12, 36, 36, 1, 12, 1, g.ld, 20 * 36, 36 * 12, g.sC, 3)
    torch.cuda.synchronize()
    assert log.total == 1 and log[0]["name"] == "gemm_f32" and log[0]["grid"] == (1, 1, 3)
    O.assert_bits_equal(view, (A.double() @ B.double()).float(), 32, 32)
    g.check()
