"""Fused embedding HIP kernels (csrc/kernels/embed.hip) on a real MI355X (-m gpu): the gather forward
bit for bit against ops.kernels.embed_reference, the scatter-sum backward exactly on integer
cotangents, bit for bit against the host model of its sum order (tests/test_embed.py) on random
ones, and within the rule of tests/test_xent_gpu.py of the float64 oracle: ``E_ref`` is the max-abs
error of torch's own f32 ``index_add_`` on the GPU against the oracle; an entry of dTable may be off by
``4 E_ref + 2^-23 max|f64 row|``."""
import pytest
import torch

from test_embed import embed_grad_host_model

pytestmark = pytest.mark.gpu

dev = torch.device("cuda", 0)
F32, BF16 = torch.float32, torch.bfloat16
_DT = {F32: "f32", BF16: "bf16"}
V = 97


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from learning_jax_sharding_amd.ops import hip as H
    H.lib()
    return H


def _ids(T, gen, dtype=torch.int64, vocab=V):
    """Random ids with, on the first tokens (as many as there are): V - 1, 0, -1, V and V + 5."""
    ids = torch.randint(0, vocab, (T,), generator=gen)
    for i, v in enumerate((vocab - 1, 0, -1, vocab, vocab + 5)[:T]):
        ids[i] = v
    return ids.to(dtype)


def _pattern(name, hip):
    """(ids, D) of one backward case."""
    gen = torch.Generator().manual_seed(17)
    chunk = hip.EMBED_CHUNK
    if name == "random":
        return _ids(300, gen), 24
    if name == "one-id":
        return torch.full((300,), 5, dtype=torch.int64), 24
    if name == "chunked":   # one list of two whole chunks and three tokens
        return torch.full((2 * chunk + 3,), 5, dtype=torch.int64), 8
    if name == "half":      # one list longer than a chunk among short ones, and unowned tokens
        ids = _ids(3 * chunk, gen)
        ids[5::2] = 3
        return ids, 24
    if name == "distinct":
        return torch.randperm(V, generator=gen)[:90], 640
    raise KeyError(name)


PATTERNS = ["random", "one-id", "chunked", "half", "distinct"]


def _oracle64(dy, ids, rows, offset=0):
    loc = ids.long() - offset
    own = (loc >= 0) & (loc < rows)
    return torch.zeros(rows, dy.shape[-1], dtype=torch.float64).index_add_(0, loc[own], dy.double()[own])


# ------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("ids_dtype", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("out_dtype", [F32, BF16], ids=["out-f32", "out-bf16"])
@pytest.mark.parametrize("tab_dtype", [F32, BF16], ids=["tab-f32", "tab-bf16"])
@pytest.mark.parametrize("T", [1, 300])
@pytest.mark.parametrize("D", [8, 24, 640, 1032])
def test_forward_is_bit_exact(hip, D, T, tab_dtype, out_dtype, ids_dtype):
    from learning_jax_sharding_amd.ops import kernels as K
    gen = torch.Generator().manual_seed(D + T)
    table = torch.randn(V, D, generator=gen).to(tab_dtype)
    ids = _ids(T, gen, ids_dtype)
    want = K.embed_reference(table, ids, 0, out_dtype)
    with hip.launch_log() as log:
        got = hip.embed(table.to(dev), ids.to(dev), 0, out_dtype)
    torch.cuda.synchronize()
    assert [r["name"] for r in log] == [f"embed_fwd<{_DT[tab_dtype]},{_DT[out_dtype]}>"] and log.total == 1
    assert got.dtype == out_dtype and tuple(got.shape) == (T, D) and got.is_contiguous()
    bits = torch.int32 if out_dtype == F32 else torch.int16
    assert torch.equal(got.cpu().view(bits), want.view(bits))
    for t in (ids.long() < 0).logical_or(ids.long() >= V).nonzero().flatten().tolist():
        assert not got[t].any()


def test_forward_takes_2d_ids_and_a_strided_table(hip):
    """ids [3, 100]; the table a [:, :24] view of a [97, 32] allocation (row stride 32, read in place)."""
    from learning_jax_sharding_amd.ops import kernels as K
    gen = torch.Generator().manual_seed(2)
    big = torch.randn(V, 32, generator=gen)
    ids = _ids(300, gen).reshape(3, 100)
    got = hip.embed(big.to(dev)[:, :24], ids.to(dev), 0, BF16)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (3, 100, 24)
    assert torch.equal(got.cpu(), K.embed_reference(big[:, :24], ids, 0, BF16))


# ------------------------------------------------------------------------------------- backward
@pytest.mark.parametrize("dy_dtype", [F32, BF16], ids=["dy-f32", "dy-bf16"])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_backward_is_exact_on_integer_cotangents(hip, pattern, dy_dtype):
    """Integers of magnitude <= 8 add exactly in any order: dTable equals the float64 oracle, rows
    nobody chose are +0.0 although the output buffer held NaN, and the launches are the five kernels
    (six with the combine when a list can be longer than a chunk)."""
    ids, D = _pattern(pattern, hip)
    T = ids.numel()
    gen = torch.Generator().manual_seed(T)
    dy = torch.randint(-8, 9, (T, D), generator=gen).to(dy_dtype)
    want = _oracle64(dy, ids, V)
    out = torch.full((V, D), float("nan"), device=dev)
    with hip.launch_log() as log:
        got = hip.embed_grad(dy.to(dev), ids.to(dev), V, 0, out=out)
    torch.cuda.synchronize()
    names = [r["name"] for r in log]
    tail = ["embed_combine"] if T > hip.EMBED_CHUNK else []
    assert names == ["embed_rank", "embed_scan", "embed_fill", f"embed_bwd<{_DT[dy_dtype]}>"] + tail, names
    assert got is out and got.dtype == F32
    assert torch.equal(got.cpu().double(), want)
    chosen = torch.zeros(V, dtype=torch.bool)
    chosen[ids[(ids >= 0) & (ids < V)]] = True
    empty = got.cpu()[~chosen]
    assert empty.numel() or pattern in ("random", "half")   # (97 ids among hundreds of random tokens)
    assert torch.equal(empty.view(torch.int32), torch.zeros_like(empty, dtype=torch.int32))


@pytest.mark.parametrize("dy_dtype", [F32, BF16], ids=["dy-f32", "dy-bf16"])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_backward_keeps_the_sum_order(hip, pattern, dy_dtype):
    """Random normal cotangents: dTable is the host model's bits (ascending tokens, chunks of
    EMBED_CHUNK, the chunk sums added in order)."""
    ids, D = _pattern(pattern, hip)
    T = ids.numel()
    gen = torch.Generator().manual_seed(T + 1)
    dy = torch.randn(T, D, generator=gen).to(dy_dtype)
    want = embed_grad_host_model(dy, ids, V, hip.EMBED_CHUNK)
    got = hip.embed_grad(dy.to(dev), ids.to(dev), V)
    torch.cuda.synchronize()
    assert torch.equal(got.cpu().view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("dy_dtype", [F32, BF16], ids=["dy-f32", "dy-bf16"])
@pytest.mark.parametrize("pattern", ["random", "chunked", "half"])
def test_backward_accuracy_against_float64(hip, pattern, dy_dtype):
    ids, D = _pattern(pattern, hip)
    T = ids.numel()
    gen = torch.Generator().manual_seed(T + 2)
    dy = torch.randn(T, D, generator=gen).to(dy_dtype)
    want = _oracle64(dy, ids, V)
    own = (ids >= 0) & (ids < V)
    ref32 = torch.zeros(V, D, device=dev).index_add_(0, ids[own].to(dev), dy.float()[own].to(dev)).cpu().double()
    got = hip.embed_grad(dy.to(dev), ids.to(dev), V).cpu().double()
    e_ref = (ref32 - want).abs().max().item()
    allowed = 4.0 * e_ref + 2.0 ** -23 * want.abs().amax(-1, keepdim=True)
    err = (got - want).abs()
    worst = err.max().item()
    frac = torch.where(err > 0, err / allowed.clamp_min(1e-300), torch.zeros_like(err)).max().item()
    print(f"embed-figures {pattern} T={T} D={D} dy={_DT[dy_dtype]} max_err={worst:.3e} E_ref={e_ref:.3e} "
          f"worst_fraction_of_bound={frac:.3f}")
    assert torch.isfinite(got).all()
    assert frac <= 1.0, (pattern, worst, e_ref, frac)


def test_vocabulary_offsets(hip):
    """Three unequal row ranges of one table, each looked up with its offset: the outputs sum to the
    whole lookup exactly (one non-zero contributor per row) and the three dTable pieces are the
    slices of the whole gradient bit for bit."""
    gen = torch.Generator().manual_seed(4)
    D, T = 24, 300
    table = torch.randn(V, D, generator=gen).to(dev)
    ids = _ids(T, gen).to(dev)
    dy = torch.randn(T, D, generator=gen).to(BF16).to(dev)
    whole_t = table.clone().requires_grad_(True)
    whole = hip.embed(whole_t, ids, 0, BF16)
    (whole_g,) = torch.autograd.grad(whole, whole_t, dy)
    parts = [(0, 30), (30, 31), (31, V)]
    total = torch.zeros(T, D, device=dev)
    for lo, hi in parts:
        piece = table[lo:hi].clone().requires_grad_(True)
        with hip.launch_log() as log:
            out = hip.embed(piece, ids, lo, BF16)
            (g,) = torch.autograd.grad(out, piece, dy)
        tail = ["embed_combine"] if T > hip.EMBED_CHUNK else []
        assert [r["name"] for r in log] == ["embed_fwd<f32,bf16>", "embed_rank", "embed_scan", "embed_fill",
                                            "embed_bwd<bf16>"] + tail
        own = (ids >= lo) & (ids < hi)
        assert not out[~own].any()
        total += out.float()
        assert g.dtype == F32 and torch.equal(g.view(torch.int32), whole_g[lo:hi].view(torch.int32))
    torch.cuda.synchronize()
    assert torch.equal(total, whole.float())


def test_bf16_table_gets_a_bf16_gradient(hip):
    gen = torch.Generator().manual_seed(6)
    table = torch.randn(V, 8, generator=gen).to(BF16).to(dev).requires_grad_(True)
    ids = _ids(300, gen, torch.int32).to(dev)
    dy = torch.randint(-8, 9, (300, 8), generator=gen).float().to(dev)
    (g,) = torch.autograd.grad(hip.embed(table, ids), table, dy)
    torch.cuda.synchronize()
    assert g.dtype == BF16 and torch.equal(g.cpu().double(), _oracle64(dy.cpu(), ids.cpu(), V))


def test_graph_replay_matches_eager(hip):
    """Forward + backward captured once and replayed three times on the same inputs: every replay
    gives the eager bits, and the histogram workspaces read all zero afterwards (the scan re-arms)."""
    ids, D = _pattern("half", hip)
    T = ids.numel()
    gen = torch.Generator().manual_seed(8)
    table = torch.randn(V, D, generator=gen).to(dev).requires_grad_(True)
    ids = ids.to(dev)
    dy = torch.randn(T, D, generator=gen).to(BF16).to(dev)

    def step():
        out = hip.embed(table, ids, 0, BF16)
        return out.detach(), torch.autograd.grad(out, table, dy)[0]

    eager = [t.clone() for t in step()]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.autograd.set_multithreading_enabled(False), torch.cuda.graph(graph, stream=side):
        static = step()
    for i in range(3):
        graph.replay()
        torch.cuda.synchronize()
        for name, a, b in zip(("out", "dtable"), static, eager):
            assert torch.equal(a, b), (i, name)
    ws = [t for (_, name), t in hip._WS.items() if name.startswith("embed/")]
    assert any("embed/graph/" in name for (_, name) in hip._WS) and ws
    for t in ws:
        assert not t.view(torch.int32).any()


def test_switch_off_takes_the_torch_formulation(hip, monkeypatch):
    """LJS_FUSED_EMBED=0: no embed_ launch; 1 and 2: the kernels; the results are within the rule
    (the output exact) every time."""
    from learning_jax_sharding_amd.ops import kernels as K
    ids, D = _pattern("random", hip)
    T = ids.numel()
    gen = torch.Generator().manual_seed(9)
    table = torch.randn(V, D, generator=gen)
    dy = torch.randn(T, D, generator=gen)
    want_out = K.embed_reference(table, ids)
    want = _oracle64(dy, ids, V)
    own = (ids >= 0) & (ids < V)
    ref32 = torch.zeros(V, D, device=dev).index_add_(0, ids[own].to(dev), dy[own].to(dev)).cpu().double()
    allowed = 4.0 * (ref32 - want).abs().max().item() + 2.0 ** -23 * want.abs().amax(-1, keepdim=True)
    for flag, fused in (("0", False), ("1", True), ("2", True)):
        monkeypatch.setenv("LJS_FUSED_EMBED", flag)
        tab = table.to(dev).requires_grad_(True)
        with hip.launch_log() as log:
            out = K.embed(tab, ids.to(dev))
            (g,) = torch.autograd.grad(out, tab, dy.to(dev))
        torch.cuda.synchronize()
        names = [r["name"] for r in log if r["name"].startswith("embed_")]
        assert bool(names) == fused, (flag, names)
        if flag == "2":
            assert "embed_bwd<f32>" in names
        assert torch.equal(out.detach().cpu(), want_out)
        err = (g.cpu().double() - want).abs()
        print(f"embed-figures LJS_FUSED_EMBED={flag} max_err={err.max().item():.3e}")
        assert (err <= allowed).all(), flag


def test_torch_sort_route_above_the_all_pairs_cap(hip):
    """cap + 1 tokens: the index comes from a stable torch.sort (no embed_rank / embed_fill launch),
    the sum pass is the same and gives the host model's bits."""
    T, D = hip.EMBED_ALLPAIRS_MAX_TOKENS + 1, 8
    gen = torch.Generator().manual_seed(10)
    ids = _ids(T, gen)
    ids[7::5] = 3
    dy = torch.randn(T, D, generator=gen)
    want = embed_grad_host_model(dy, ids, V, hip.EMBED_CHUNK)
    with hip.launch_log() as log:
        got = hip.embed_grad(dy.to(dev), ids.to(dev), V)
    torch.cuda.synchronize()
    assert [r["name"] for r in log] == ["embed_scan", "embed_bwd<f32>", "embed_combine"]
    assert torch.equal(got.cpu().view(torch.int32), want.view(torch.int32))
