"""Which kernel instance ran: the HIP launchers rewrite what they are asked for (a GEMM tile code is
demoted, 8 attention waves become 4, the fused projection's block takes one item or many), so every
test here reads the library's launch record (ops/hip.py last_launch / launch_log) next to its
comparison with an fp32 / fp64 reference (run on a real MI355X: -m gpu)."""
import math
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

dev = torch.device("cuda", 0)


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from learning_jax_sharding_amd.ops import hip as H
    H.lib()
    return H


def _rand(*shape, dtype=torch.bfloat16, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g).to(dtype).to(dev)


def _stored(mat, kc_rowmajor: bool):
    """(storage tensor, ld) of a logical [R][K] matrix, k-contiguous or m/n-contiguous."""
    if kc_rowmajor:
        return mat.contiguous(), mat.shape[1]
    return mat.t().contiguous(), mat.shape[0]


# ============================================================================ GEMM tile codes
def resolved_tile(tile, a_kc, b_kc, out_f32, M, N, K, lda=None, ldb=None, ldc=None, batch=1, splitk=1, sA=0, sB=0,
                  sC=0, res=False, bias=False, slabs=False, c_aligned=True):
    """The tile code ljs_gemm_bf16 launches for a requested one: its demotion rules in the order the
    launcher applies them, stated here independently of csrc/kernels/gemm.hip's tile table (whose
    plan step tests/test_gemm_picks.py checks against this function).  Pure Python;
    ``res``: an epilogue operand (residual add / mask) is passed, ``bias``: a bias is passed."""
    a_kc, b_kc, out_f32 = bool(a_kc), bool(b_kc), bool(out_f32)
    lda = (K if a_kc else M) if lda is None else lda
    ldb = (K if b_kc else N) if ldb is None else ldb
    ldc = N if ldc is None else ldc
    tile %= 100000                                    # the + 100000 / + 200000 forcing codes
    nkt = -(-K // 64)                                 # the launched split count: ceil-sized splits
    splitk = min(max(1, splitk), nkt)
    kps = -(-nkt // splitk)
    splitk = -(-nkt // kps)
    k_ext = splitk * kps * 64 if slabs else K         # K-rows the splits address
    dma_ok = (K % 64 == 0 and (slabs or (K // 64) % splitk == 0)  # whole K-tiles, 32-bit offsets
              and (M * lda if a_kc else k_ext * lda) < (1 << 30)
              and (N * ldb if b_kc else k_ext * ldb) < (1 << 30))
    dma_store_ok = out_f32 or (N % 8 == 0 and ldc % 8 == 0 and (sC % 8 == 0 or batch == 1) and c_aligned)  # 16-byte stores
    if tile > 1000 and not (dma_ok and dma_store_ok):                          # LDS-DMA conditions unmet
        tile = 128
    if res and tile > 1000 and not (a_kc and b_kc):                            # epilogue operand: k-contiguous
        tile = 128
    if res and tile in (643, 644):                                             # ... and none at 64x64
        tile = 64
    if tile in (643, 644) and not (dma_ok and dma_store_ok):                   # LDS-DMA conditions unmet
        tile = 64
    if tile in (2563, 12856) and not (not a_kc and not b_kc and out_f32):      # weight-gradient tiles only
        tile = 1282
    if tile == 2561 and not (a_kc and b_kc):                                   # k-contiguous only
        tile = 1284
    if tile == 2562 and not (a_kc and b_kc and not out_f32 and not res):       # ... bf16, no epilogue operand
        tile = 1282
    if tile == 2562 and batch > 1:                                             # a batch: folded, or 256x128
        if not (sA == 0 and sB == N * ldb and sC == N and ldc == N * batch and not bias
                and N * batch * ldb < (1 << 30)):
            tile = 2561
    if tile == 1602 and not (a_kc and b_kc and not out_f32 and splitk == 1):   # ... bf16, unsplit
        tile = 1282
    if tile in (12883, 12884) and not ((not a_kc and not b_kc and out_f32) or (a_kc and b_kc)):   # no mixed layouts
        tile = 1282
    return tile


def _kc(b):
    return "kc" if b else "mn"


def _tile_of(name):
    """(BM, BN, WM, WN) of an LDS-DMA / lean instance name."""
    return tuple(int(t) for t in re.match(r"\w+<(\d+),(\d+),(\d+),(\d+),", name).groups())


def _gemm_case(hip, tile, a_kc, b_kc, out_f32, M, N, K):
    """One test_gemm_layouts-style call, compared with the fp32 product: the launch's record."""
    A = _rand(M, K, seed=1)
    B = _rand(K, N, seed=2)
    ref = A.float() @ B.float()
    As, lda = _stored(A, a_kc)
    Bs, ldb = _stored(B.t(), b_kc)
    C = torch.full((M, N), float("nan"), dtype=torch.float32 if out_f32 else torch.bfloat16, device=dev)
    hip.gemm(As, Bs, C, M, N, K, lda, ldb, N, bool(a_kc), bool(b_kc), tile=tile)
    rec = hip.last_launch()
    torch.cuda.synchronize()
    tol = 2e-2 if not out_f32 else 1e-3            # test_gemm_layouts' tolerance
    torch.testing.assert_close(C.float(), ref, rtol=tol, atol=tol * math.sqrt(K))
    return rec


# (requested code, M, N, K, kernel instance): the k-contiguous bf16-output tiles at one ragged block
# each (K one 64-tile, or two where the 3- / 4-stage ring needs a refill), default = lean K-loop
_LEAN = [(2561, 264, 136, 128, "gemm_lean<256,128,4,2,3>"), (2562, 264, 200, 128, "gemm_lean<256,192,4,2,2>"),
         (1282, 136, 72, 64, "gemm_lean<128,128,2,2,2>"), (1284, 136, 72, 128, "gemm_lean<128,128,2,2,4>"),
         (12883, 136, 72, 128, "gemm_lean<128,128,2,4,3>"), (12884, 136, 72, 128, "gemm_lean<128,128,2,4,4>"),
         (644, 72, 40, 128, "gemm_lean<64,64,2,2,4>"),
         # 128x160 runs the general kernel unless the lean one is forced (+ 100000)
         (101602, 136, 168, 64, "gemm_lean<128,160,4,1,2>")]


@pytest.mark.parametrize("tile,M,N,K,name", _LEAN)
def test_gemm_lean_instance(hip, tile, M, N, K, name):
    rec = _gemm_case(hip, tile, 1, 1, 0, M, N, K)
    bm, bn, wm, wn = _tile_of(name)
    assert rec["name"] == name and rec["block"] == 64 * wm * wn and rec["blocks"] == -(-M // bm) * -(-N // bn)
    assert rec["requested_tile"] == tile and rec["resolved_tile"] == tile % 100000
    assert rec["splitk"] == 1 and rec["variant"] == 3          # the plain epilogue instance


# launch_dma_kk: the general LDS-DMA kernel in its k-contiguous bf16 instances (+ 200000 forces it
# where the lean kernel would run; 1602 and 643 have no lean default)
_DMA_KK = [(202561, 264, 136, 128, "gemm_dma<256,128,4,2,3,kc,kc,bf16>"),
           (202562, 264, 200, 128, "gemm_dma<256,192,4,2,2,kc,kc,bf16>"),
           (1602, 136, 168, 64, "gemm_dma<128,160,4,1,2,kc,kc,bf16>"),
           (201282, 136, 72, 64, "gemm_dma<128,128,2,2,2,kc,kc,bf16>"),
           (212883, 136, 72, 128, "gemm_dma<128,128,2,4,3,kc,kc,bf16>"),
           (212884, 136, 72, 128, "gemm_dma<128,128,2,4,4,kc,kc,bf16>"),
           (200644, 72, 40, 128, "gemm_dma<64,64,2,2,4,kc,kc,bf16>")]


@pytest.mark.parametrize("tile,M,N,K,name", _DMA_KK)
def test_gemm_dma_kk_instance(hip, tile, M, N, K, name):
    rec = _gemm_case(hip, tile, 1, 1, 0, M, N, K)
    assert rec["name"] == name
    assert rec["requested_tile"] == tile and rec["resolved_tile"] == tile % 100000
    bm, bn, wm, wn = _tile_of(name)
    assert rec["variant"] == 3 and rec["block"] == 64 * wm * wn and rec["blocks"] == -(-M // bm) * -(-N // bn)


@pytest.mark.parametrize("a_kc,b_kc", [(1, 1), (0, 0), (1, 0), (0, 1)])
@pytest.mark.parametrize("out_f32", [0, 1])
@pytest.mark.parametrize("tile,M,N,K", [(643, 72, 40, 128), (1284, 136, 72, 128)])
def test_gemm_dma_layout_instances(hip, a_kc, b_kc, out_f32, tile, M, N, K):
    """launch_dma's 8 layout / output instances at the 64x64 (3-stage) and 128x128 (4-stage) tiles."""
    forced = 200000 if (tile == 1284 and a_kc and b_kc and not out_f32) else 0   # (else the lean kernel)
    rec = _gemm_case(hip, tile + forced, a_kc, b_kc, out_f32, M, N, K)
    shape = "64,64,2,2,3" if tile == 643 else "128,128,2,2,4"
    assert rec["name"] == f"gemm_dma<{shape},{_kc(a_kc)},{_kc(b_kc)},{'f32' if out_f32 else 'bf16'}>"
    bm = 64 if tile == 643 else 128
    assert rec["resolved_tile"] == tile and rec["grid"] == (-(-M // bm) * -(-N // bm), 1, 1)


@pytest.mark.parametrize("tile", [64, 128])
@pytest.mark.parametrize("a_kc,b_kc,out_f32", [(1, 1, 0), (0, 0, 1), (1, 0, 0), (0, 1, 1)])
def test_gemm_register_staged_instances(hip, tile, a_kc, b_kc, out_f32):
    """The register-staged tiles, asked for by code and reached by demotion (K = 40 is no multiple
    of the LDS-DMA kernels' 64-wide K-tile)."""
    M, N, K = 136, 72, 40
    name = f"gemm_bf16<{tile},{tile},{_kc(a_kc)},{_kc(b_kc)},{'f32' if out_f32 else 'bf16'}>"
    for req in (tile, 644 if tile == 64 else 1282):
        rec = _gemm_case(hip, req, a_kc, b_kc, out_f32, M, N, K)
        assert rec["name"] == name and rec["requested_tile"] == req and rec["resolved_tile"] == tile
        assert rec["grid"] == (-(-M // tile) * -(-N // tile), 1, 1) and rec["block"] == 256


def _slab_operands(T, K, N, seed):
    return _rand(T, K, seed=seed), _rand(T, N, seed=seed + 1)


@pytest.mark.parametrize("tile,shape", [(1282, "128,128,2,2,2"), (12883, "128,128,2,4,3"), (12884, "128,128,2,4,4")])
def test_gemm_slab_instance(hip, tile, shape):
    """launch_slab: the weight-gradient layout's plain split-K slab instance, uneven splits."""
    T, K, N, S = 448, 136, 72, 3                   # 7 K-tiles over 3 splits: 3 + 3 + 1
    assert hip.slab_count(T // 64, S) == S
    x, dy = _slab_operands(T, K, N, 70)
    slabs = torch.full((S, K, N), float("nan"), dtype=torch.float32, device=dev)
    hip.gemm(x, dy, slabs, K, N, T, K, N, N, False, False, sC=K * N, splitk=S, tile=tile, slabs=True)
    rec = hip.last_launch()
    ref = x.float().t() @ dy.float()
    torch.testing.assert_close(slabs.sum(0), ref, rtol=2e-3, atol=2e-3 * ref.abs().max().item())
    assert rec["name"] == f"gemm_dma<{shape},mn,mn,f32>" and rec["variant"] == 3
    assert rec["requested_tile"] == tile and rec["resolved_tile"] == tile and rec["splitk"] == S
    assert rec["blocks"] == 2 * 1 * S


def test_gemm_grouped_pair_instance(hip):
    """Two slab GEMMs of one instance closed as a group: ONE record, the grouped kernel, both split
    counts, a grid of both GEMMs' items."""
    T = 448
    x0, dy0 = _slab_operands(T, 136, 72, 80)
    x1, dy1 = _slab_operands(T, 72, 200, 82)
    s0, s1 = 3, 2                                   # 7 K-tiles: 3 + 3 + 1 and 4 + 3
    assert hip.slab_count(T // 64, s0) == s0 and hip.slab_count(T // 64, s1) == s1
    sl0 = torch.full((s0, 136, 72), float("nan"), device=dev)
    sl1 = torch.full((s1, 72, 200), float("nan"), device=dev)
    with hip.launch_log() as log:
        n_before = hip.lib().ljs_launch_count()
        hip.gemm_group_begin()
        hip.gemm(x0, dy0, sl0, 136, 72, T, 136, 72, 72, False, False, sC=136 * 72, splitk=s0, tile=1282, slabs=True)
        hip.gemm(x1, dy1, sl1, 72, 200, T, 72, 200, 200, False, False, sC=72 * 200, splitk=s1, tile=1282, slabs=True)
        n_open = hip.lib().ljs_launch_count()     # (nothing is launched before the group closes)
        hip.gemm_group_end(sl0)
        n_closed = hip.lib().ljs_launch_count()
    assert n_open == n_before and n_closed == n_open + 1 and log.total == 1 and len(log) == 1
    rec = log[0]
    assert rec["name"] == "gemm_dma_group2<128,128,2,2,2,mn,mn,f32>"
    assert (rec["splitk"], rec["splitk1"]) == (s0, s1) and rec["resolved_tile"] == 1282
    assert rec["blocks"] == 2 * 1 * s0 + 1 * 2 * s1 and rec["block"] == 256
    for sl, x, dy in ((sl0, x0, dy0), (sl1, x1, dy1)):
        ref = x.float().t() @ dy.float()
        torch.testing.assert_close(sl.sum(0), ref, rtol=2e-3, atol=2e-3 * ref.abs().max().item())


def test_gemm_f32_record(hip):
    A = torch.randn(3, 20, 36, device=dev)
    B = torch.randn(3, 36, 12, device=dev)
    C = torch.empty(3, 20, 12, device=dev)
    hip._gemm_f32(A, B, C, 20, 12, 36, 36, 1, 12, 1, 12, 20 * 36, 36 * 12, 20 * 12, 3)
    rec = hip.last_launch()
    torch.testing.assert_close(C, A.double().matmul(B.double()).float(), rtol=1e-5, atol=1e-4)
    assert rec["name"] == "gemm_f32" and rec["grid"] == (1, 1, 3) and rec["requested_tile"] is None


def _block_step(B):
    """One eager value_and_grad step of the case6 attention block (tests/test_gpu_e2e.py _run_block,
    1 x 1 mesh, S = 256) under launch_log: (loss, records)."""
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd import nn
    from learning_jax_sharding_amd.mesh import Mesh, create_device_mesh
    from learning_jax_sharding_amd.models import MultiHeadAttention
    from learning_jax_sharding_amd.ops import hip as H
    from learning_jax_sharding_amd.sharding import NamedSharding, PartitionSpec as P
    mesh = Mesh(create_device_mesh((1, 1)), ("data", "model"))
    rules = (("batch", "data"), ("embed", "model"), ("hidden", "model"))
    model = MultiHeadAttention(640, heads=8, dim_head=64)
    x = ljs.random.normal(ljs.random.PRNGKey(0), (B, 256, 640))
    params = model.init(ljs.random.PRNGKey(1), x)["params"]
    params = ljs.device_put(params, nn.logical_to_mesh_sharding(nn.get_partition_spec(params), mesh, rules))
    x = ljs.device_put(x, NamedSharding(mesh, P("data", "model")))

    def loss(p):
        return model.apply({"params": p}, x).sum()

    with mesh, nn.axis_rules(rules), H.launch_log() as log:
        val, g = ljs.value_and_grad(loss)(params)
        g = ljs.tree_map(lambda a: np.asarray(a), nn.unbox(g))    # (forces the deferred weight-gradient combines)
    return float(np.asarray(val)), g, log


def test_production_picks_run_as_picked(gpu_devices):
    """The attention block's step below and past the fused projection's gate (2 B H >= CUs,
    ops/linear.py _fuse_attention_ok): every GEMM runs the tile the Python picker asked for, the
    fused projection + forward runs only past the gate, and the attention backward is the split
    pair below B H = 128 and the fused kernel from there (attention.hip ljs_attn_bwd)."""
    gpu_devices(1)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    heads = 8
    b_gate = -(-cus // (2 * heads))                 # the first batch past the gate (16 on 256 CUs)
    assert 2 * 8 * heads < cus, "an 8-batch step is meant to sit below the gate"
    for B in (8, b_gate):
        val, g, log = _block_step(B)
        assert math.isfinite(val) and log.total == len(log) > 0, (log.total, len(log))
        names = [r["name"] for r in log]
        gemms = [r for r in log if r["requested_tile"] is not None]
        # the projection (unless fused), the out-projection, its dX, the weight gradients (one grouped launch)
        assert len(gemms) >= (3 if "qkv_attn_fwd" in names else 4), names
        changed = [(r["name"], r["requested_tile"], r["resolved_tile"]) for r in gemms
                   if r["requested_tile"] % 100000 != r["resolved_tile"]]
        assert not changed, changed
        assert ("qkv_attn_fwd" in names) == (2 * B * heads >= cus), (B, names)
        if "qkv_attn_fwd" in names:
            assert not any(n.startswith("attn_fwd") for n in names), names
            assert log[names.index("qkv_attn_fwd")]["blocks"] == min(B * heads, cus)
        else:
            assert names.count("attn_fwd_res<4>" if B * heads * 2 < 256 else "attn_fwd_res<8>") == 1, names
        bwd = [n for n in names if n.startswith("attn_bwd")]
        assert len(bwd) == 1 and bwd[0].startswith("attn_bwd_fused" if B * heads >= 128 else "attn_bwd_pair32"), bwd


# ============================================================================ fused Q/K/V projection + forward
def _check_qkv_attn(hip, B, H, K, want_grid, pad_x=False):
    """test_qkv_attn_fwd_bit_exact's checks (tolerances unchanged) + finite o / lse everywhere + the
    launch record's grid."""
    T, N = B * 256, 64 * H
    if pad_x:
        wide = _rand(T, K + 64, seed=31)           # x: a column slice of a wider buffer (ldx = K + 64)
        x = wide[:, 32:32 + K]
        assert x.stride(0) == K + 64 and x.data_ptr() % 16 == 0
    else:
        x = _rand(T, K, seed=31)
    wt = (_rand(3, N, K, seed=32) * 0.05).contiguous()
    out = torch.full((T, 3 * N), float("nan"), device=dev).bfloat16()
    scale = 64 ** -0.5
    o, lse = hip.qkv_attn_fwd(x, wt, out, H, scale)
    rec = hip.last_launch()
    ref = torch.empty_like(out)
    xc = x.contiguous()
    hip.gemm(xc, wt, ref, T, N, K, K, K, 3 * N, True, True, batch=3, sA=0, sB=N * K, sC=N)
    torch.cuda.synchronize()
    assert rec["name"] == "qkv_attn_fwd" and rec["grid"] == (want_grid, 1, 1) and rec["block"] == 512, rec
    assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all()
    assert torch.equal(out, ref)
    q, k, v = (ref.view(B, 256, 3, H, 64)[:, :, i] for i in range(3))
    o_ref, lse_ref = hip.attn_fwd_lse(q, k, v, scale)
    torch.cuda.synchronize()
    o4 = o.view(B, 256, H, 64).float()
    torch.testing.assert_close(o4, o_ref.float(), rtol=0, atol=4e-3)
    assert ((o4 - o_ref.float()).abs().amax(-1) > 0).float().mean().item() < 0.02
    torch.testing.assert_close(lse.view(B, H, 256), lse_ref, rtol=1e-6, atol=1e-5)
    # fp32 softmax reference with bf16 P, a few batch elements at a time (small score tensors)
    err = err_ref = 0.0
    for b0 in range(0, B, 8):
        qs, ks, vs = (t[b0:b0 + 8].float() for t in (q, k, v))
        s_ = torch.einsum("bshd,bthd->bhst", qs, ks) * scale
        o_t = torch.einsum("bhst,bthd->bshd", torch.softmax(s_, -1).bfloat16().float(), vs)
        err = max(err, (o4[b0:b0 + 8] - o_t).abs().max().item())
        err_ref = max(err_ref, (o_ref[b0:b0 + 8].float() - o_t).abs().max().item())
    assert err <= 1.25 * err_ref + 1e-3, (err, err_ref)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("case", ["cus+8_k128", "2cus_k128", "2cus_k640", "2cus+8_k256", "cus+8_k256_ldx"])
def test_qkv_attn_fwd_above_cu_count(hip, case):
    """More (batch, head) items than CUs, at the device's real CU count: blocks walk 2 and 3 items,
    the next item's first K-tile streaming in under the current item's last K-step, epilogue and
    attention (the regime the benchmark and every step past the gate run in).  K = 128 is two
    K-tiles: the next item's tile is issued right after the item's first barrier."""
    cus, H = _cus(), 8
    items, K, pad = {"cus+8_k128": (cus + 8, 128, False), "2cus_k128": (2 * cus, 128, False),
                     "2cus_k640": (2 * cus, 640, False), "2cus+8_k256": (2 * cus + 8, 256, False),
                     "cus+8_k256_ldx": (cus + 8, 256, True)}[case]
    assert items % H == 0 and items > cus
    _check_qkv_attn(hip, items // H, H, K, cus, pad_x=pad)


@pytest.mark.parametrize("G", [1, 3, 8, 13])
@pytest.mark.parametrize("B,H,K", [(5, 4, 128), (3, 8, 256)])
def test_qkv_attn_fwd_forced_grid(hip, B, H, K, G):
    """The same item loop, deeper, on tiny shapes: a forced grid of G blocks gives up to 24 items
    per block, uneven item counts, and G < 8 / G % 8 != 0 in the XCD remap."""
    hip.set_attention_cus(G)
    try:
        _check_qkv_attn(hip, B, H, K, G)
    finally:
        hip.set_attention_cus(None)
    # restored: 16 items on min(items, CUs) blocks again
    hip.qkv_attn_fwd(_rand(512, 128, seed=1), _rand(3, 512, 128, seed=2),
                     torch.empty(512, 1536, dtype=torch.bfloat16, device=dev), 8, 0.125)
    assert hip.last_launch()["grid"] == (min(16, _cus()), 1, 1)
    torch.cuda.synchronize()


# ============================================================================ attention forward variants
def _lse2_fp64(q, k, scale, causal, q_offset):
    """log2 of the fp64 sum of exp(scale * s) over the unmasked keys, [B][H][Sq]; +inf where a row
    has no unmasked key."""
    s = torch.einsum("bfnh,btnh->bnft", q.double(), k.double()) * scale
    if causal:
        qi = torch.arange(q.shape[1], device=q.device)[:, None] + q_offset
        ki = torch.arange(k.shape[1], device=q.device)[None, :]
        s = s.masked_fill(ki > qi, float("-inf"))
    lse = torch.logsumexp(s, -1) / math.log(2.0)
    return torch.where(torch.isneginf(lse), torch.full_like(lse, float("inf")), lse)


# lse against fp64: the project's kernel-to-kernel bound (1e-5) + the fp32 torch reference's own
# distance from fp64 on these shapes (1.2e-6), rounded up.  Removing one key moves the least
# affected row's lse by >= 6.5e-5 on these shapes, so the bound still sees a one-key masking error.
_LSE_ATOL = 2e-5

_RES8_SHAPES = [(4, 64, 64, 64, False, 0), (2, 64, 200, 200, True, 0), (8, 32, 40, 40, False, 0),
                (4, 64, 130, 256, True, 64), (4, 64, 64, 100, True, 0)]


def _check_fwd_lse(hip, B, H, Sq, Sk, causal, q_offset, want):
    from learning_jax_sharding_amd.ops.kernels import attention_reference
    q = _rand(B, Sq, H, 64, seed=41)
    k, v = _rand(B, Sk, H, 64, seed=42), _rand(B, Sk, H, 64, seed=43)
    scale = 0.125
    o, lse = hip.attn_fwd_lse(q, k, v, scale, causal, q_offset)
    rec = hip.last_launch()
    torch.cuda.synchronize()
    assert rec["name"] == want and rec["acc_mode"] == 0, rec
    torch.testing.assert_close(o.float(), attention_reference(q, k, v, scale, causal, q_offset).float(), rtol=2e-2,
                               atol=2e-2)
    ref = _lse2_fp64(q, k, scale, causal, q_offset)
    inf = torch.isinf(ref)
    assert torch.equal(torch.isposinf(lse), inf)
    err = (lse.double() - ref)[~inf].abs().max().item()
    print(f"lse max |err| vs fp64: {err:.3e} ({want}, {(B, H, Sq, Sk, causal, q_offset)})")
    assert err <= _LSE_ATOL, err
    return rec


@pytest.mark.parametrize("B,H,Sq,Sk,causal,q_offset", _RES8_SHAPES)
def test_attention_fwd_res8_vs_reference(hip, B, H, Sq, Sk, causal, q_offset):
    """Default switches at >= 256 blocks of 128 queries: the 8-wave resident forward (not its 4-wave
    demotion), O against the fp32 reference and lse against fp64."""
    assert -(-Sq // 128) * H * B >= 256
    rec = _check_fwd_lse(hip, B, H, Sq, Sk, causal, q_offset, "attn_fwd_res<8>")
    assert rec["grid"] == (-(-Sq // 128) * H * B, 1, 1) and rec["block"] == 512


@pytest.mark.parametrize("res,want", [(4, "attn_fwd_res<4>"), (0, "attn_fwd_tiled<1>")])
@pytest.mark.parametrize("B,H,Sq,Sk,causal,q_offset", [_RES8_SHAPES[1], _RES8_SHAPES[3]])
def test_attention_fwd_lse_other_variants(hip, res, want, B, H, Sq, Sk, causal, q_offset):
    hip.set_attention_fwd_resident(res)
    try:
        _check_fwd_lse(hip, B, H, Sq, Sk, causal, q_offset, want)
    finally:
        hip.set_attention_fwd_resident(-1)


def test_attention_fwd_res8_demoted_below_256_blocks(hip):
    """The launcher's rule from the other side: 255 blocks of 128 queries run 4 waves."""
    _check_fwd_lse(hip, 1, 255, 64, 64, False, 0, "attn_fwd_res<4>")


@pytest.mark.parametrize("causal", [False, True])
def test_attention_fwd_inkernel_lse_merge_res8(hip, causal):
    """test_attention_fwd_inkernel_lse_merge at a shape that keeps 8 waves: the ring forward's merge
    epilogue (modes 1 / 2 / 3) in attn_fwd_res<8>, causal with one fully masked key block."""
    from learning_jax_sharding_amd.ops import kernels as K
    torch.manual_seed(0)
    B, Sq, H, sk, nblk = 4, 128, 64, 128, 3
    q = torch.randn(B, Sq, H, 64, device="cuda").bfloat16()
    k = torch.randn(B, nblk * sk, H, 64, device="cuda").bfloat16()
    v = torch.randn(B, nblk * sk, H, 64, device="cuda").bfloat16()
    q_off = sk if causal else 0     # causal: queries aligned with block 1 -> block 2 fully masked (+inf lse)
    ref = K.attention_reference(q, k, v, 0.125, causal, q_off).float()
    state = [None, None]
    out = None
    with hip.launch_log() as log:
        for i in range(nblk):
            kb, vb = k[:, i * sk:(i + 1) * sk], v[:, i * sk:(i + 1) * sk]
            out = K.attention_fwd_merge(q, kb, vb, 0.125, causal, q_off - i * sk, state, last=i == nblk - 1)
    torch.cuda.synchronize()
    assert [(r["name"], r["acc_mode"]) for r in log] == [("attn_fwd_res<8>", m) for m in (1, 2, 3)], list(log)
    np.testing.assert_allclose(out.float().cpu().numpy(), ref.cpu().numpy(), rtol=2e-2, atol=2e-2)


# ============================================================================ the record itself
def test_launch_log_ring_keeps_last_32(hip):
    A = torch.randn(1, 8, 8, device=dev)
    C = torch.empty(1, 8, 8, device=dev)
    with hip.launch_log() as log:
        for _ in range(40):
            hip._gemm_f32(A, A, C, 8, 8, 8, 8, 1, 8, 1, 8, 64, 64, 64, 1)
    torch.cuda.synchronize()
    assert log.total == 40 and len(log) == 32 and all(r["name"] == "gemm_f32" for r in log)
    n = hip.lib().ljs_launch_count()
    assert hip._launch_at(n - 33) is None and hip._launch_at(n) is None and hip._launch_at(n - 32) is not None


def test_launch_record_under_graph_capture(hip):
    """The record is made when a launch is recorded into a graph; a replay adds none."""
    A = torch.randn(1, 8, 8, device=dev)
    C = torch.empty(1, 8, 8, device=dev)
    hip._gemm_f32(A, A, C, 8, 8, 8, 8, 1, 8, 1, 8, 64, 64, 64, 1)   # (the kernel is loaded before the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with hip.launch_log() as cap:
        with torch.cuda.graph(g):
            hip._gemm_f32(A, A, C, 8, 8, 8, 8, 1, 8, 1, 8, 64, 64, 64, 1)
    with hip.launch_log() as rep:
        g.replay()
    torch.cuda.synchronize()
    assert cap.total == 1 and rep.total == 0
    torch.testing.assert_close(C, A @ A, rtol=1e-5, atol=1e-4)
