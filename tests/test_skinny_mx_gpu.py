"""The MX-fp8 skinny GEMM kernel (csrc/kernels/skinny_mx.hip) on a real MI355X, bit for bit against float64 on exact
inputs: x integers in [-8, 8], codes the e4m3 encodings of integers in [-15, 15], scale bytes in [125, 129] drawn
independently per (row, 32-block), so a wrong lane -> block or row -> scale map shows.  Every partial sum is a multiple
of 2^-2 below 2^22 (checked in the builder): f32 accumulation is exact in any order and the float64 product, rounded
once, is the expected bits.  Every run is poisoned: NaN behind and beside x, 0x7F codes and 0xFF scales behind row
N - 1 and in the pad columns, a residual inside a NaN buffer, C inside NaN guards that must stay untouched."""
import functools

import pytest
import torch

import gemm_oracle as O

pytestmark = pytest.mark.gpu

dev = torch.device("cuda", 0)
BF16, F32 = torch.bfloat16, torch.float32
# M in {1, 5, 16}; N = 8 half a group, 24 a clamped tail group, 48 three blocks; K = 128 one line (forced W > 1:
# empty waves), 384 an uneven wave split, 1280 more lines than a wave keeps in flight, with a partial last round
CASES = {
    "M1-N8-K128-bf16": (1, 8, 128, BF16, {}),
    "M16-N8-K128-f32-bias": (16, 8, 128, F32, dict(bias=BF16)),
    "M5-N24-K384-f32-bias-relu": (5, 24, 384, F32, dict(bias=F32, relu=True)),
    "M16-N24-K384-bf16-relu-res": (16, 24, 384, BF16, dict(relu=True, res=BF16)),
    "M5-N48-K1280-f32": (5, 48, 1280, F32, {}),
    "M16-N48-K1280-bf16-bias-res": (16, 48, 1280, BF16, dict(bias=F32, res=F32)),
    "M1-N24-K1280-bf16-res": (1, 24, 1280, BF16, dict(res=BF16)),
}
POISON_ROWS = 16


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from learning_jax_sharding_amd.ops import hip as H
    H.lib()
    yield H
    H.set_skinny_waves(None)


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
    return (hip.skinny_mx_raw if raw else hip.skinny_mx)(**a)


@pytest.mark.parametrize("name", list(CASES))
def test_skinny_mx_is_exact(hip, name):
    M, N, K, out, epi = CASES[name]
    _, expected = _case(name)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    for waves in (None,) + tuple(hip.SKINNY_WAVES):
        hip.set_skinny_waves(waves)
        g = O.Guarded((1, M, N), out, dev)
        with hip.launch_log() as log:
            _launch(hip, name, g)
        torch.cuda.synchronize()
        W = waves or hip.skinny_mx_plan(M, N, K, cus)[0]
        parts = [str(W), "f32" if out == F32 else "bf16"] + [p for p in ("bias", "relu", "res") if epi.get(p)]
        assert log.total == 1 and log[0]["name"] == "skinny_mx<" + ",".join(parts) + ">", list(log)
        assert log[0]["blocks"] == -(-N // 16) and log[0]["block"] == 64 * W, log[0]
        g.check()
        try:
            O.assert_bits_equal(g.view, expected, 16, 16)
        except AssertionError as e:
            raise AssertionError(f"{name} waves={waves}:\n{e}") from None
    hip.set_skinny_waves(None)


def test_launcher_refuses_and_records_nothing(hip):
    name = "M16-N24-K384-bf16-relu-res"
    M, N, K, out, _ = CASES[name]
    (x, q, s, _, res), expected = _case(name)
    g = O.Guarded((1, M, N), out, dev)
    bad = {
        "M=17": dict(M=17), "M=0": dict(M=0), "K=352": dict(K=352), "N=20": dict(N=20),
        "null codes": dict(q=None), "null scales": dict(s=None), "null x": dict(x=None),
        "misaligned C": dict(out=g.buf.view(-1)[g.c_off + 1:]), "misaligned codes": dict(q=q.view(-1)[8:]),
        "misaligned scales": dict(s=s.view(-1)[2:]), "odd lda": dict(lda=x.stride(0) + 1),
        "ldq no multiple of 16": dict(ldq=q.stride(0) + 8), "lds no multiple of 4": dict(lds=s.stride(0) + 2),
        "lds below K / 32": dict(lds=K // 32 - 4), "ldc below N": dict(ldc=N - 8),
        "res with f32 out": dict(out=torch.empty((M, N), dtype=F32, device=dev), ldc=N),
    }
    for what, over in bad.items():
        with hip.launch_log() as log:
            rc = _launch(hip, name, g, raw=True, **over)
        torch.cuda.synchronize()
        assert rc != 0 and log.total == 0, (what, rc, list(log))
        g.check(written=False)
    with pytest.raises(NotImplementedError):
        _launch(hip, name, g, M=17)
    with hip.launch_log() as log:          # the same call, accepted
        assert _launch(hip, name, g, raw=True) == 0
    torch.cuda.synchronize()
    assert log.total == 1 and log[0]["name"].startswith("skinny_mx<")
    g.check()
    O.assert_bits_equal(g.view, expected, 16, 16)
