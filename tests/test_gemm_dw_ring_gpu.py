"""The half-tile LDS ring of the 4-wave 128x128 weight-gradient GEMM (tile code 1282, m/n-contiguous
operands, f32 split-K slabs): five half-K-tile slots at two blocks per CU, counted waits that keep
halves in flight across every barrier and across a persistent block's item change.

Oracle 1 is the same call on tile code 1284 (four whole stages, one block per CU, a K-loop this
ring does not touch): it runs the same MFMA sequence per output element, so the slabs are equal
bit for bit.  Oracle 2 is the fp32 product with the tolerances of test_gemm_weight_grad_slab_tiles.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

dev = torch.device("cuda", 0)
RING_NAME = "gemm_dma<128,128,2,2,2,mn,mn,f32>"
GROUP_NAME = "gemm_dma_group2<128,128,2,2,2,mn,mn,f32>"


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from learning_jax_sharding_amd.ops import hip as H
    H.lib()
    return H


def _rand(*shape, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g).to(torch.bfloat16).to(dev)


def _slab_gemm(hip, A, B, M, N, T, S, tile, lda=None, ldb=None):
    """NaN-filled slabs written by one weight-gradient slab GEMM; returns (slabs, launch record)."""
    Se = hip.slab_count(-(-T // 64), S)
    sl = torch.full((Se, M, N), float("nan"), device=dev)
    hip.gemm(A, B, sl, M, N, T, lda or M, ldb or N, N, False, False, sC=M * N, splitk=Se, tile=tile, slabs=True)
    rec = hip.last_launch()
    torch.cuda.synchronize()
    return sl, rec


def _check(hip, A, B, M, N, T, S, lda=None, ldb=None, ref=None):
    got, rec = _slab_gemm(hip, A, B, M, N, T, S, 1282, lda, ldb)
    assert rec["name"] == RING_NAME and rec["resolved_tile"] == 1282, rec
    want, rec4 = _slab_gemm(hip, A, B, M, N, T, S, 1284, lda, ldb)
    assert rec4["name"] == "gemm_dma<128,128,2,2,4,mn,mn,f32>", rec4
    assert not torch.isnan(got).any()
    assert torch.equal(got, want)
    if ref is None:
        ref = A[:, :M].float().t() @ B[:, :N].float()
    torch.testing.assert_close(got.sum(0), ref, rtol=2e-3, atol=2e-3 * ref.abs().max().item())
    return got, rec


# (T, S): K-tiles per split 1, 2, 3, 4, 5, 6 and 11 with every split full (fewer than, as many as and
# more than the five half-tile slots hold, odd and even), then two whose last split runs past K
# (7 K-tiles in splits of 4; 5 K-tiles in splits of 2)
_KT = [(128, 2), (256, 2), (384, 2), (512, 2), (640, 2), (768, 2), (1408, 2), (448, 2), (320, 3)]


@pytest.mark.parametrize("T,S", _KT)
@pytest.mark.parametrize("M,N", [(136, 72), (264, 200)])
def test_ring_edges(hip, M, N, T, S):
    A = _rand(T, M, seed=41)
    B = _rand(T, N, seed=42)
    nkt = T // 64
    kps = -(-nkt // S)
    assert hip.slab_count(nkt, S) * kps >= nkt
    _check(hip, A, B, M, N, T, S)


# (M, N, T, S): 600 items of 3 K-tiles (one block per item unless the device holds fewer), then 1024
# items -- whole rounds of the 512 resident blocks of a 256-CU device, which the launcher turns into
# a persistent grid -- of 3, 1 and 2 K-tiles (with 1, every K-tile is followed by an epilogue)
@pytest.mark.parametrize("M,N,T,S", [(1280, 1280, 1152, 6), (1024, 2048, 1536, 8), (1024, 2048, 512, 8),
                                     (1024, 2048, 1024, 8)])
def test_ring_persistent_walk(hip, M, N, T, S):
    """More items than resident blocks: a persistent block changes items with halves in flight, and
    the epilogue's stores share the wait counter with them."""
    A = _rand(T, M, seed=43)
    B = _rand(T, N, seed=44)
    items = -(-M // 128) * -(-N // 128) * S
    slots = 2 * torch.cuda.get_device_properties(0).multi_processor_count
    got, rec = _check(hip, A, B, M, N, T, S)
    assert got.shape[0] == S
    if items > slots and items % slots == 0:
        assert rec["blocks"] == slots, rec   # the persistent grid: items / slots items per block
    else:
        assert rec["blocks"] == items, rec


def test_ring_grouped_launch(hip):
    """Two slab GEMMs of different shapes and split counts (the first in the dW_qkv form: a batch of
    three over one A and separate B tensors) as one grouped grid equal the two launched one by one."""
    T = 1024
    x = _rand(T, 264, seed=45)
    dq = [_rand(T, 200, seed=46 + i) for i in range(3)]
    h = _rand(T, 136, seed=49)
    dy = _rand(T, 328, seed=50)
    nkt = T // 64
    s0, s1 = hip.slab_count(nkt, 3), hip.slab_count(nkt, 5)   # 6 and 4 K-tiles per split

    def run(group, tile):
        sl0 = torch.full((s0, 3, 264, 200), float("nan"), device=dev)
        sl1 = torch.full((s1, 136, 328), float("nan"), device=dev)
        if group:
            hip.gemm_group_begin()
        hip.gemm(x, dq[0], sl0, 264, 200, T, 264, 200, 200, False, False, batch=3, sA=0, sC=264 * 200,
                 splitk=s0, tile=tile, slabs=True, b_list=dq)
        hip.gemm(h, dy, sl1, 136, 328, T, 136, 328, 328, False, False, sC=136 * 328, splitk=s1, tile=tile,
                 slabs=True)
        if group:
            hip.gemm_group_end(sl0)
        rec = hip.last_launch()
        torch.cuda.synchronize()
        return sl0, sl1, rec

    r0, r1, _ = run(False, 1282)
    g0, g1, rec = run(True, 1282)
    assert rec["name"] == GROUP_NAME and rec["resolved_tile"] == 1282, rec
    assert rec["splitk"] == s0 and rec["splitk1"] == s1, rec
    o0, o1, _ = run(False, 1284)
    assert not torch.isnan(g0).any() and not torch.isnan(g1).any()
    assert torch.equal(g0, r0) and torch.equal(g1, r1)
    assert torch.equal(g0, o0) and torch.equal(g1, o1)
    for b in range(3):
        ref = x.float().t() @ dq[b].float()
        torch.testing.assert_close(g0[:, b].sum(0), ref, rtol=2e-3, atol=2e-3 * ref.abs().max().item())
    ref = h.float().t() @ dy.float()
    torch.testing.assert_close(g1.sum(0), ref, rtol=2e-3, atol=2e-3 * ref.abs().max().item())


def test_ring_strided_operands(hip):
    """Operands that are column slices of wider tensors (ld larger than the width)."""
    M, N, T, S = 264, 200, 704, 2
    Aw = _rand(T, 384, seed=51)
    Bw = _rand(T, 320, seed=52)
    _check(hip, Aw, Bw, M, N, T, S, lda=384, ldb=320)


def test_ring_back_to_back(hip):
    """The same launch twice in a row into fresh NaN-filled slabs: both equal the oracles."""
    M, N, T, S = 264, 200, 1408, 2
    A = _rand(T, M, seed=53)
    B = _rand(T, N, seed=54)
    Se = hip.slab_count(T // 64, S)
    a = torch.full((Se, M, N), float("nan"), device=dev)
    b = torch.full((Se, M, N), float("nan"), device=dev)
    for sl in (a, b):
        hip.gemm(A, B, sl, M, N, T, M, N, N, False, False, sC=M * N, splitk=Se, tile=1282, slabs=True)
    torch.cuda.synchronize()
    want, _ = _check(hip, A, B, M, N, T, S)
    assert torch.equal(a, want) and torch.equal(b, want)
