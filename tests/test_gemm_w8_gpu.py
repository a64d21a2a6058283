"""The W8A16 tile GEMM (csrc/kernels/gemm_w8.hip) on a real MI355X.  Exact: tests/test_skinny_mx_gpu.py's method -- x
integers in [-8, 8], codes the e4m3 encodings of integers in [-15, 15], scale bytes in [125, 129] per (row, 32-block),
every partial sum a multiple of 2^-2 below 2^22 (at K = 1280 at most 8 * 15 * 4 * 1280 = 614400; asserted in the
builder), so float64 rounded once is the expected bits -- with NaN behind and beside x, 0x7F codes and 0xFF scales
behind row N - 1 and in the pad columns, C inside NaN guards.  Then normal data against the bf16 tile GEMM on the
dequantised weight, bit for bit (the lean kernel's k order), and the launcher's refusals."""
import functools

import pytest
import torch

import gemm_oracle as O

pytestmark = pytest.mark.gpu

dev = torch.device("cuda", 0)
BF16, F32 = torch.bfloat16, torch.float32
# M = 1, 17: a fraction of a tile; 64, 65: the 64-row tile's edge; 130: two 128-row tiles and a 2-row tail.  N = 8, 24: a
# fraction of a column tile; 136, 264: whole tiles plus 8 columns.  K = 128: the prologue and one ring step; 384: the
# ring wraps, an odd count of 128-code lines; 1280: a long K.
CASES = {
    "M1-N8-K128-bf16": (1, 8, 128, BF16, {}),
    "M17-N24-K128-f32-bias": (17, 24, 128, F32, dict(bias=BF16)),
    "M64-N128-K384-bf16-relu-res": (64, 128, 384, BF16, dict(relu=True, res=BF16)),
    "M65-N136-K384-f32-bias-relu": (65, 136, 384, F32, dict(bias=F32, relu=True)),
    "M130-N264-K1280-bf16-bias-res": (130, 264, 1280, BF16, dict(bias=F32, res=F32)),
}
POISON_ROWS = 16


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from learning_jax_sharding_amd.ops import hip as H
    H.lib()
    yield H
    H.set_gemm_w8_rows(None)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(operands on the device, expected [1][M][N] in the output type): built and checked once on the CPU."""
    M, N, K, out, epi = CASES[name]
    gen = torch.Generator().manual_seed(M + N + K)
    ints = lambda shape, lo, hi: torch.randint(lo, hi + 1, shape, generator=gen)      # noqa: E731
    xv = ints((M, K), -8, 8).double()
    codes = ints((N, K), -15, 15).float().to(torch.float8_e4m3fn)
    sb = ints((N, K // 32), 125, 129)
    w = codes.float().double() * torch.ldexp(torch.ones(()), sb - 127).double().repeat_interleave(32, dim=1)
    assert float((xv.abs() @ w.abs().t()).max()) < 2.0 ** 22       # multiples of 2^-2 below 2^22: exact in f32
    y = xv @ w.t()
    bias = res = None
    if "bias" in epi:
        bias = ints((N,), -64, 64).to(epi["bias"])
        y = y + bias.double()
    if epi.get("relu"):
        y = y.clamp_min(0.0)
    y = y.to(out)
    if "res" in epi:
        r = ints((M, N), -64, 64).to(epi["res"])
        y = (y.double() + r.double()).to(BF16)
        res = torch.full((M + 1, N + 8), float("nan"), dtype=epi["res"])
        res[:M, :N] = r
    x = torch.full((M + POISON_ROWS, K + 8), float("nan"), dtype=BF16)
    x[:M, :K] = xv.to(BF16)
    q = torch.full((N + POISON_ROWS, K + 16), 0x7F, dtype=torch.uint8)
    q[:N, :K] = codes.view(torch.uint8)
    s = torch.full((N + POISON_ROWS, K // 32 + 4), 0xFF, dtype=torch.uint8)
    s[:N, :K // 32] = sb.to(torch.uint8)
    to = lambda t: None if t is None else t.to(dev)      # noqa: E731
    return (to(x), to(q), to(s), to(bias), to(res)), y[None]


def _launch(hip, name, g, raw=False, **over):
    M, N, K, out, epi = CASES[name]
    (x, q, s, bias, res), _ = _case(name)
    a = dict(x=x, q=q, s=s, out=g.view[0], M=M, N=N, K=K, lda=x.stride(0), ldc=g.ld, bias=bias,
             relu=bool(epi.get("relu")), res=res, res_ld=0 if res is None else res.stride(0), ldq=q.stride(0),
             lds=s.stride(0))
    a.update(over)
    return (hip.gemm_w8_raw if raw else hip.gemm_w8)(**a)


@pytest.mark.parametrize("rows", [64, 128])
@pytest.mark.parametrize("name", list(CASES))
def test_gemm_w8_is_exact(hip, name, rows):
    M, N, K, out, epi = CASES[name]
    _, expected = _case(name)
    hip.set_gemm_w8_rows(rows)
    g = O.Guarded((1, M, N), out, dev)
    with hip.launch_log() as log:
        _launch(hip, name, g)
    torch.cuda.synchronize()
    hip.set_gemm_w8_rows(None)
    parts = [f"R{rows}", "f32" if out == F32 else "bf16"] + [p for p in ("bias", "relu", "res") if epi.get(p)]
    assert log.total == 1 and log[0]["name"] == "gemm_w8<" + ",".join(parts) + ">", list(log)
    assert log[0]["blocks"] == -(-M // rows) * -(-N // 128) and log[0]["block"] == 256, log[0]
    g.check()
    O.assert_bits_equal(g.view, expected, rows, 128)


@pytest.mark.parametrize("rows", [64, 128])
@pytest.mark.parametrize("shape", [(65, 136, 384), (130, 264, 1280)])
def test_same_bits_as_the_bf16_tile_gemm(hip, shape, rows):
    """Normal data: the kernel equals hip.gemm at tile 1282 on the dequantised weight, whose record must be of the lean or
    LDS-DMA family (their fragment-to-k mapping and k order are the ones meant)."""
    from learning_jax_sharding_amd.ops import fp8
    M, N, K = shape
    plan = hip.gemm_plan(M, N, K, K, K, N, True, True, False, tile=1282)       # on the CPU first: 1282 does not demote
    assert plan["err"] == 0 and plan["resolved_tile"] == 1282, plan
    gen = torch.Generator().manual_seed(N)
    x = torch.randn((M, K), generator=gen).to(BF16).to(dev)
    qv, ex = fp8.quantize_mx_ref(torch.randn((N, K), generator=gen).to(BF16))
    w_hat = fp8.dequantize_mx_ref(qv, ex).to(BF16).to(dev)
    q, s = qv.view(torch.uint8).to(dev), (ex + 127).to(torch.uint8).to(dev)
    want, got = torch.empty((M, N), dtype=BF16, device=dev), torch.empty((M, N), dtype=BF16, device=dev)
    with hip.launch_log() as log:
        hip.gemm(x, w_hat, want, M, N, K, K, K, N, True, True, tile=1282)
    assert log.total == 1 and log[0]["name"].startswith(("gemm_lean<128,128,", "gemm_dma<128,128,")), list(log)
    hip.set_gemm_w8_rows(rows)
    hip.gemm_w8(x, q, s, got, M, N, K, K, N)
    hip.set_gemm_w8_rows(None)
    torch.cuda.synchronize()
    O.assert_bits_equal(got[None], want[None], rows, 128)


def test_launcher_refuses_and_records_nothing(hip):
    name = "M64-N128-K384-bf16-relu-res"
    M, N, K, out, _ = CASES[name]
    (x, q, s, _, res), expected = _case(name)
    g = O.Guarded((1, M, N), out, dev)
    bad = {
        "M=0": dict(M=0), "K=192": dict(K=192), "N=20": dict(N=20),
        "null codes": dict(q=None), "null scales": dict(s=None), "null x": dict(x=None),
        "misaligned C": dict(out=g.buf.view(-1)[g.c_off + 1:]), "misaligned codes": dict(q=q.view(-1)[8:]),
        "misaligned scales": dict(s=s.view(-1)[2:]), "lds below K / 32": dict(lds=K // 32 - 4),
        "res with f32 out": dict(out=torch.empty((M, N), dtype=F32, device=dev), ldc=N),
    }
    for what, over in bad.items():
        with hip.launch_log() as log:
            rc = _launch(hip, name, g, raw=True, **over)
        torch.cuda.synchronize()
        assert rc != 0 and log.total == 0, (what, rc, list(log))
        g.check(written=False)
    with pytest.raises(NotImplementedError):
        _launch(hip, name, g, K=192)
    with hip.launch_log() as log:          # the same call, accepted
        assert _launch(hip, name, g, raw=True) == 0
    torch.cuda.synchronize()
    assert log.total == 1 and log[0]["name"].startswith("gemm_w8<")
    g.check()
    O.assert_bits_equal(g.view, expected, 64, 128)
