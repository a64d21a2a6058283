"""The skinny GEMM kernel (csrc/kernels/skinny.hip) on a real MI355X against the exact-arithmetic oracle of
tests/gemm_oracle.py: integer operands whose every partial sum is an f32 number, so the output must be
bit-identical to ``expected`` under the plan's wave count and under every forced one (waves with empty
slices included), into a C that lies inside a NaN-payload buffer whose guards must stay untouched.

Every run is poisoned: x is the first M rows of a buffer whose following rows are NaN, Wt the first N rows
of a buffer whose following rows are NaN (N = 24 and N = 648 end in a clamped half group), the rows of both
are padded with ``case``'s poison columns, and a residual sits in a wider NaN-padded buffer.  Gaussian
operands are held to the oracle's own derived bound, run twice for equal bits."""
import functools

import pytest
import torch

import gemm_oracle as O

pytestmark = pytest.mark.gpu

dev = torch.device("cuda", 0)
BF16, F32 = torch.bfloat16, torch.float32
SHAPES = [(1, 16, 32), (2, 24, 96), (7, 648, 640), (8, 512, 640), (16, 640, 1792), (8, 4104, 128)]
EPI_SHAPES = [(8, 512, 640), (7, 648, 640)]
EPILOGUES = {
    "bias-f32": dict(bias=F32),
    "bias-bf16-relu": dict(bias=BF16, relu=True),
    "relu": dict(relu=True),
    "res-bf16": dict(res=("add", BF16, False)),
    "res-f32": dict(res=("add", F32, False)),
    "bias-relu-res": dict(bias=F32, relu=True, res=("add", BF16, False)),
}
NAN_ROWS = 16


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from learning_jax_sharding_amd.ops import hip as H
    H.lib()
    yield H
    H.set_skinny_waves(None)


def _freeze(kw):
    return tuple(sorted((k, v) for k, v in kw.items()))


@functools.lru_cache(maxsize=None)
def _case(M, N, K, out, frozen=()):
    """The oracle's case (computed once per test module) and its operands on the device, poisoned."""
    c = O.case(M, N, K, out=out, lda_pad=8, ldb_pad=16, seed=M + N + K, **dict(frozen))
    k = c["call"]
    nan = lambda cols: torch.full((NAN_ROWS, cols), float("nan"), dtype=BF16)     # noqa: E731
    x = torch.cat([c["A"].view(M, k["lda"]), nan(k["lda"])]).to(dev)
    wt = torch.cat([c["B"].view(N, k["ldb"]), nan(k["ldb"])]).to(dev)
    bias = None if c["bias"] is None else c["bias"].to(dev)
    res = None
    if c["res"] is not None:
        res = torch.full((M + 1, N + 8), float("nan"), dtype=c["res"].dtype)
        res[:M, :N] = c["res"]
        res = res.to(dev)
    return c, (x, wt, bias, res)


def _launch(hip, c, ops, g, raw=False, **over):
    k = c["call"]
    x, wt, bias, res = ops
    a = dict(x=x, wt=wt, out=g.view[0], M=k["M"], N=k["N"], K=k["K"], lda=k["lda"], ldc=g.ld, bias=bias,
             relu=k["relu"], res=res, res_ld=0 if res is None else res.stride(0), ldb=k["ldb"])
    a.update(over)
    return (hip.skinny_raw if raw else hip.skinny)(**a)


def _check_record(hip, log, c, waves):
    k = c["call"]
    assert log.total == 1, log
    rec = log[0]
    if waves is None:
        waves = hip.skinny_plan(k["M"], k["N"], k["K"], torch.cuda.get_device_properties(dev).multi_processor_count)[0]
    parts = [str(waves), "f32" if c["out"] == F32 else "bf16"] + (["bias"] if c["bias"] is not None else []) + \
        (["relu"] if k["relu"] else []) + (["res"] if c["res"] is not None else [])
    assert rec["name"] == "skinny<" + ",".join(parts) + ">", rec
    assert rec["blocks"] == -(-k["N"] // 16) and rec["block"] == 64 * waves, rec


def _exact(hip, M, N, K, out, **kw):
    c, ops = _case(M, N, K, out, _freeze(kw))
    assert O.exactness(c) < 2 ** 24
    for waves in (None,) + tuple(hip.SKINNY_WAVES):
        hip.set_skinny_waves(waves)
        g = O.Guarded((1, M, N), out, dev)
        with hip.launch_log() as log:
            _launch(hip, c, ops, g)
        torch.cuda.synchronize()
        _check_record(hip, log, c, waves)
        g.check()
        try:
            O.assert_bits_equal(g.view, c["expected"], 16, 16)
        except AssertionError as e:
            raise AssertionError(f"M={M} N={N} K={K} out={out} waves={waves} {kw}:\n{e}") from None
    hip.set_skinny_waves(None)


@pytest.mark.parametrize("out", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_skinny_is_exact(hip, M, N, K, out):
    _exact(hip, M, N, K, out)


@pytest.mark.parametrize("epi", list(EPILOGUES))
@pytest.mark.parametrize("M,N,K", EPI_SHAPES)
def test_skinny_epilogues_are_exact(hip, M, N, K, epi):
    kw = EPILOGUES[epi]
    _exact(hip, M, N, K, BF16, **kw)
    if "res" not in kw:
        _exact(hip, M, N, K, F32, **kw)


@pytest.mark.parametrize("M,N,K", [(8, 512, 640), (16, 640, 1792)])
def test_skinny_gaussian_within_derived_bound(hip, M, N, K):
    for out in (BF16, F32):
        c, ops = _case(M, N, K, out, _freeze(dict(gaussian=True)))
        first = None
        for waves in (None, None) + tuple(hip.SKINNY_WAVES):
            hip.set_skinny_waves(waves)
            g = O.Guarded((1, M, N), out, dev)
            _launch(hip, c, ops, g)
            torch.cuda.synchronize()
            g.check()
            got = g.view.cpu()
            err = (got.double() - c["oracle"]).abs()
            worst = float((err / c["bound"]).max())
            print(f"skinny-figures gaussian M={M} N={N} K={K} out={out} waves={waves} max err/bound={worst:.3f} "
                  f"max err={float(err.max()):.3e}")
            assert torch.isfinite(got).all() and (err <= c["bound"]).all(), (M, N, K, out, waves, worst)
            if first is None:
                first = got
            elif waves is None:
                O.assert_bits_equal(got, first)             # two runs of the plan: the same bits
        hip.set_skinny_waves(None)


def test_stacked_pair_equals_single_calls(hip):
    """A fused projection's stacked [2 N][K] operand writing [M][2 N] against the two single calls into the
    column blocks of an equal buffer."""
    M, N, K = 8, 512, 640
    c1, (x, w1, _, _) = _case(M, N, K, BF16, _freeze(dict(gaussian=True)))
    ldb = c1["call"]["ldb"]
    gen = torch.Generator().manual_seed(11)
    w2 = torch.randn((N, ldb), generator=gen).bfloat16().to(dev)
    stacked = torch.cat([w1[:N], w2, torch.full((NAN_ROWS, ldb), float("nan"), dtype=BF16, device=dev)])
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    assert hip.skinny_plan(M, N, K, cus)[0] == hip.skinny_plan(M, 2 * N, K, cus)[0]
    for out in (BF16, F32):
        fused = torch.empty((M, 2 * N), dtype=out, device=dev)
        single = torch.empty((M, 2 * N), dtype=out, device=dev)
        hip.skinny(x, stacked, fused, M, 2 * N, K, c1["call"]["lda"], 2 * N, ldb=ldb)
        hip.skinny(x, w1, single[:, :N], M, N, K, c1["call"]["lda"], 2 * N, ldb=ldb)
        hip.skinny(x, w2, single[:, N:], M, N, K, c1["call"]["lda"], 2 * N, ldb=ldb)
        torch.cuda.synchronize()
        assert torch.isfinite(fused).all()
        O.assert_bits_equal(fused[None], single[None], 16, 16)


def test_launcher_refuses_and_records_nothing(hip):
    M, N, K = 8, 512, 640
    c, ops = _case(M, N, K, BF16)
    x, wt, _, _ = ops
    g = O.Guarded((1, M, N), BF16, dev)
    skewed = g.buf.view(-1)[g.c_off + 1:]                  # C two bytes off its alignment
    bad = {
        "M=17": dict(M=17),
        "M=0": dict(M=0),
        "K=40": dict(K=40),
        "N=20": dict(N=20),
        "misaligned C": dict(out=skewed),
        "null Wt": dict(wt=None),
        "odd lda": dict(lda=c["call"]["lda"] + 1),
        "ldc below N": dict(ldc=N - 8),
    }
    for name, over in bad.items():
        with hip.launch_log() as log:
            rc = _launch(hip, c, ops, g, raw=True, **over)
        torch.cuda.synchronize()
        assert rc != 0 and log.total == 0, (name, rc, list(log))
        g.check(written=False)
    with pytest.raises(NotImplementedError):
        hip.skinny(x, wt, g.view[0], 17, N, K, c["call"]["lda"], g.ld, ldb=c["call"]["ldb"])
    # the same call, accepted
    with hip.launch_log() as log:
        assert _launch(hip, c, ops, g, raw=True) == 0
    torch.cuda.synchronize()
    assert log.total == 1 and log[0]["name"].startswith("skinny<")
    g.check()
    O.assert_bits_equal(g.view, c["expected"], 16, 16)
