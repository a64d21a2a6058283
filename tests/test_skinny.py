"""The skinny GEMM's host side (csrc/kernels/skinny.hip through ops/hip.py and ops/linear.py), without a GPU:

* ``skinny_plan`` over a grid of shapes and CU counts: the wave count is a block size the kernel takes and
  never exceeds the K-steps, the blocks are ``ceil(N / 16)``, the plan is pure, monotone, and ``M`` does not
  enter it; shapes outside ``1 <= M <= 16, K % 32 == 0, N % 8 == 0`` are refused;
* ``skinny_supported`` on descriptions of aligned and misaligned operands, a column block (``ldc > N``) and
  an odd ``lda``;
* the routing predicate of ``ops.linear.linear``: false with grad enabled, above 16 rows, for a host tensor
  and with ``LJS_SKINNY_GEMM=0``.
"""
import itertools

import pytest
import torch

BF16, F32 = torch.bfloat16, torch.float32
MS, NS, KS, CUS = (1, 8, 16), (16, 24, 256, 512, 640, 3584, 32768), (32, 96, 512, 640, 1792), (64, 256)


@pytest.fixture(scope="module")
def hip():
    from learning_jax_sharding_amd.ops import hip as H
    H.lib()
    return H


def test_plan_properties(hip):
    seen = {}
    for M, N, K, cus in itertools.product(MS, NS, KS, CUS):
        waves, blocks = hip.skinny_plan(M, N, K, cus)
        assert waves in hip.SKINNY_WAVES and 1 <= waves <= K // 32, (M, N, K, cus, waves)
        assert blocks == -(-N // 16), (M, N, K, cus, blocks)
        seen[(M, N, K, cus)] = (waves, blocks)
    # pure: a forced wave count and a second pass change nothing; M does not enter
    hip.set_skinny_waves(4)
    try:
        for args, want in seen.items():
            assert hip.skinny_plan(*args) == want, args
    finally:
        hip.set_skinny_waves(None)
    for (M, N, K, cus), want in seen.items():
        assert want == seen[(1, N, K, cus)], (M, N, K, cus)
    # monotone: more columns never get more waves; a longer K or more CUs never fewer
    for K, cus in itertools.product(KS, CUS):
        ws = [seen[(1, N, K, cus)][0] for N in NS]
        assert ws == sorted(ws, reverse=True), (K, cus, ws)
    for N, cus in itertools.product(NS, CUS):
        ws = [seen[(1, N, K, cus)][0] for K in KS]
        assert ws == sorted(ws), (N, cus, ws)
    for N, K in itertools.product(NS, KS):
        assert seen[(1, N, K, 64)][0] <= seen[(1, N, K, 256)][0], (N, K)
    # short K: one wave; a short-N projection gets more waves than the vocabulary head
    assert hip.skinny_plan(8, 512, 32)[0] == 1
    assert hip.skinny_plan(8, 512, 640)[0] > hip.skinny_plan(8, 32768, 640)[0]


@pytest.mark.parametrize("M,N,K", [(0, 64, 64), (17, 64, 64), (8, 64, 40), (8, 64, 48), (8, 20, 64), (8, 0, 64),
                                   (8, 64, 0)])
def test_plan_refuses(hip, M, N, K):
    with pytest.raises(ValueError):
        hip.skinny_plan(M, N, K)
    assert not hip.skinny_supported(M, N, K, max(K, 8), max(K, 8), max(N, 8), BF16)


def test_set_waves_refuses_other_sizes(hip):
    for n in (3, 5, 32):
        with pytest.raises(ValueError):
            hip.set_skinny_waves(n)
    hip.set_skinny_waves(0)


def _describe(hip, x, wt, out, M, N, K, bias=None, res=None):
    """skinny_supported of host tensors standing for the operands (their strides and addresses)."""
    return hip.skinny_supported(M, N, K, x.stride(0), wt.stride(0), out.stride(0), out.dtype, x.data_ptr(),
                                wt.data_ptr(), out.data_ptr(), None if bias is None else bias.dtype,
                                0 if bias is None else bias.data_ptr(), None if res is None else res.dtype,
                                0 if res is None else res.stride(0), 0 if res is None else res.data_ptr(),
                                x.dtype, wt.dtype)


def _aligned(rows, cols, dtype, skew=0):
    """[rows][cols] inside a buffer whose base is 64-byte aligned, moved ``skew`` elements off it."""
    raw = torch.zeros(rows * cols + 64 + skew, dtype=dtype)
    off = (-raw.data_ptr() % 64) // raw.element_size()
    return raw[off + skew:off + skew + rows * cols].view(rows, cols)


def test_supported_predicate(hip):
    M, N, K = 8, 24, 64
    x, wt = _aligned(M, K, BF16), _aligned(N, K, BF16)
    out, out32 = _aligned(M, N, BF16), _aligned(M, N, F32)
    assert _describe(hip, x, wt, out, M, N, K) and _describe(hip, x, wt, out32, M, N, K)
    assert _describe(hip, x, wt, out, M, N, K, bias=_aligned(1, N, F32)[0], res=_aligned(M, N, F32))
    assert _describe(hip, x, wt, out, M, N, K, bias=_aligned(1, N, BF16)[0], res=_aligned(M, N, BF16))
    # a column block of a wider output, padded operand rows and a wider residual
    wide = _aligned(M, 3 * N, BF16)
    assert _describe(hip, x, wt, wide[:, N:2 * N], M, N, K)
    assert _describe(hip, _aligned(M, K + 8, BF16)[:, :K], _aligned(N, K + 16, BF16)[:, :K], out, M, N, K,
                     res=_aligned(M, N + 8, BF16)[:, :N])
    # misaligned bases: x and Wt need 16 bytes, a bf16 C / residual 8, an f32 C / residual 16
    assert not _describe(hip, _aligned(M, K, BF16, skew=4), wt, out, M, N, K)
    assert not _describe(hip, x, _aligned(N, K, BF16, skew=4), out, M, N, K)
    assert _describe(hip, x, wt, _aligned(M, N, BF16, skew=4), M, N, K)
    assert not _describe(hip, x, wt, _aligned(M, N, BF16, skew=2), M, N, K)
    assert not _describe(hip, x, wt, _aligned(M, N, F32, skew=2), M, N, K)
    assert not _describe(hip, x, wt, out, M, N, K, res=_aligned(M, N, BF16, skew=1))
    assert not _describe(hip, x, wt, out, M, N, K, res=_aligned(M, N, F32, skew=1))
    # leading dimensions: an odd lda, an ldb that is no multiple of 8, an ldc that is no multiple of 4 or
    # below N, a residual row shorter than N
    assert not _describe(hip, _aligned(M, K + 1, BF16)[:, :K], wt, out, M, N, K)
    assert not _describe(hip, x, _aligned(N, K + 4, BF16)[:, :K], out, M, N, K)
    assert not _describe(hip, x, wt, _aligned(M, N + 2, BF16)[:, :N], M, N, K)
    assert not hip.skinny_supported(M, N, K, K, K, N - 8, BF16)
    assert not hip.skinny_supported(M, N, K, K, K, N, BF16, res_dtype=BF16, res_ld=N - 8)
    # dtypes: f32 operands, a residual with an f32 output, other output types
    assert not _describe(hip, _aligned(M, K, F32), wt, out, M, N, K)
    assert not _describe(hip, x, _aligned(N, K, F32), out, M, N, K)
    assert not _describe(hip, x, wt, out32, M, N, K, res=_aligned(M, N, BF16))
    assert not _describe(hip, x, wt, _aligned(M, N, torch.float16), M, N, K)
    # the raw call refuses what the predicate refuses, on any device
    with pytest.raises(NotImplementedError):
        hip.skinny(x, wt, out, M, N, K, K, N)


def test_linear_routing_predicate(hip, monkeypatch):
    from learning_jax_sharding_amd.ops import linear as L
    monkeypatch.delenv("LJS_SKINNY_GEMM", raising=False)
    w = torch.zeros(64, 32)

    class OnGpu:
        """A description of a contiguous GPU activation: what the predicate reads of x."""
        is_cuda, dtype = True, BF16

        def __init__(self, *shape):
            self.shape = shape

        def numel(self):
            n = 1
            for s in self.shape:
                n *= s
            return n

        def dim(self):
            return len(self.shape)

    monkeypatch.setattr(L, "_row_order", lambda x: (tuple(range(x.dim())), False))
    with torch.no_grad():
        assert L.skinny_route(OnGpu(8, 1, 64), [w], None)
        assert L.skinny_route(OnGpu(3, 1, 64), [w, w], None)
        assert not L.skinny_route(OnGpu(24, 1, 64), [w], None)              # above 16 rows
        assert not L.skinny_route(OnGpu(8, 1, 72), [torch.zeros(72, 32)], None)     # K % 32
        assert not L.skinny_route(OnGpu(8, 1, 64), [w.bfloat16()], None)    # weights the fused path refuses
        assert not L.skinny_route(OnGpu(8, 1, 64), [w, w], torch.zeros(32))
        assert not L.skinny_route(torch.zeros(8, 1, 64), [w], None)         # a host tensor
        monkeypatch.setenv("LJS_SKINNY_GEMM", "0")
        assert not L.skinny_route(OnGpu(8, 1, 64), [w], None)
        monkeypatch.setenv("LJS_SKINNY_GEMM", "1")
        assert L.skinny_route(OnGpu(8, 1, 64), [w], None)
        # another row order (a seq-major activation, or the token_outer swap) stays on the tile path
        monkeypatch.setattr(L, "_row_order", lambda x: ((1, 0, 2), False))
        assert L.skinny_route(OnGpu(8, 1, 64), [w], None)        # (a size-1 dim moves no row)
        assert not L.skinny_route(OnGpu(8, 2, 64), [w], None)
        monkeypatch.setattr(L, "_row_order", lambda x: ((1, 0, 2), True))
        assert not L.skinny_route(OnGpu(8, 2, 64), [w], None)
    monkeypatch.setattr(L, "_row_order", lambda x: (tuple(range(x.dim())), False))
    with torch.enable_grad():
        assert not L.skinny_route(OnGpu(8, 1, 64), [w], None)
    # a host tensor keeps its path through ops.linear's caller whatever the switches say
    with torch.no_grad():
        assert not L.skinny_route(torch.zeros(2, 64), [w], None)
