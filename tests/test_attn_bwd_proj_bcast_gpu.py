"""attn_bwd_proj's broadcast-row GEMM phase (dy_ld = 0: one cotangent row for every token): bit-equal
to the general phase on the same row written out densely and to the dX GEMM + fused backward pair,
chosen on the stride alone, and switched off by LJS_ATTN_BWD_PROJ_BCAST=0 (run on a real MI355X:
-m gpu).  Because the two phases agree to the bit, the float64 bounds of profiles/attention/figures.txt
hold for both; no tolerance appears here."""
import pytest
import torch

pytestmark = pytest.mark.gpu

dev = torch.device("cuda", 0)
S, D = 256, 64
# M = 32: one K-tile (a loop shorter than a tile group, the ring and the piece list); 64: two tiles;
# (2, 3): an odd head count under the block remap; 640: the workload's; 672 = 21 tiles: more than the
# sixteen stages, so stages are reused, and a last group of one tile
CASES = [(1, 1, 32), (1, 1, 64), (2, 3, 96), (2, 3, 640), (2, 3, 672)]
# random; zeros with one large and one subnormal element; zeros with the subnormal element alone (beside
# the large one it is absorbed in every f32 sum: alone, every dO value is its product with one weight)
ROWS = ["random", "special", "tiny"]


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from learning_jax_sharding_amd.ops import hip as H
    H.lib()
    return H


@pytest.fixture
def forced(hip, monkeypatch):
    monkeypatch.delenv("LJS_ATTN_BWD_PROJ_BCAST", raising=False)
    hip.set_attention_bwd_fused(True)
    hip.set_attention_bwd_proj(True)
    yield hip
    hip.set_attention_bwd_fused(None)
    hip.set_attention_bwd_proj(None)


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16).to(dev)


def _row(M, kind):
    if kind == "random":
        return _rand(M, seed=33)
    # zeros, one large element, and one whose bf16 value is subnormal (2^-130; the smallest normal is 2^-126)
    row = torch.zeros(M, dtype=torch.bfloat16)
    if kind == "special":
        row[5] = 2.0 ** 40
    # (alone: 2^-127, still subnormal, so its products with the weights keep a few bits as bf16 subnormals)
    tiny = 2.0 ** (-130 if kind == "special" else -127)
    row[M - 1] = tiny
    assert row[M - 1].item() == tiny
    return row.to(dev)


def _nan_outs(B, H):
    return tuple(torch.full((B, S, H, D), float("nan"), dtype=torch.bfloat16, device=dev) for _ in range(3))


_CASES = {}


def _case(hip, B, H, M, kind):
    """Inputs, the forward, and the two references of one case, computed once and left unchanged: (b) the
    general phase on the row written out as a dense [B * 256][M] dY, (c) the dX GEMM + attn_bwd_fused."""
    key = (B, H, M, kind)
    if key not in _CASES:
        qkv = _rand(B, S, 3, H, D, seed=21)
        q, k, v = (qkv[:, :, i] for i in range(3))
        o, lse = hip.attn_fwd_lse(q, k, v, D ** -0.5)
        w = _rand(H * D, M, seed=22, scale=M ** -0.5)
        row = _row(M, kind)
        dense = row.unsqueeze(0).expand(B * S, M).contiguous()
        gen = hip.attn_bwd_proj_block(q, k, v, o, dense, M, w, lse, D ** -0.5, outs=_nan_outs(B, H))
        assert hip.attn_bwd_proj_last_path() == 0      # equal rows, but ld = M: chosen on ld, never on values
        do = torch.full((B * S, H * D), float("nan"), dtype=torch.bfloat16, device=dev)
        hip.gemm(row, w, do, B * S, H * D, M, 0, M, H * D, True, True)
        pair = hip.attn_bwd_block(q, k, v, o, do.view(B, S, H, D), lse, D ** -0.5)
        assert hip.last_launch()["name"].startswith("attn_bwd_fused")
        torch.cuda.synchronize()
        assert not any(torch.isnan(t.float()).any().item() for t in gen + tuple(pair))
        _CASES[key] = (q, k, v, o, lse, w, row, gen, pair)
    return _CASES[key]


def _equal(got, want, what):
    for a, b, name in zip(got, want, ("dq", "dk", "dv")):
        assert torch.equal(a, b), (what, name, (a.float() - b.float()).abs().max().item())


@pytest.mark.parametrize("kind", ROWS)
@pytest.mark.parametrize("B,H,M", CASES)
def test_broadcast_phase_equals_general_and_pair(forced, B, H, M, kind):
    hip = forced
    q, k, v, o, lse, w, row, gen, pair = _case(hip, B, H, M, kind)
    got = hip.attn_bwd_proj_block(q, k, v, o, row, 0, w, lse, D ** -0.5, outs=_nan_outs(B, H))
    rec = hip.last_launch()
    assert rec["name"] == "attn_bwd_proj" and rec["grid"] == (B * H, 1, 1) and rec["block"] == 512, rec
    assert hip.attn_bwd_proj_last_path() == 1
    torch.cuda.synchronize()
    _equal(got, gen, "general phase, dense dY")
    _equal(got, pair, "dX GEMM + attn_bwd_fused")


@pytest.mark.parametrize("kind", ROWS)
@pytest.mark.parametrize("B,H,M", CASES)
def test_knob_off_runs_the_general_phase(forced, monkeypatch, B, H, M, kind):
    hip = forced
    q, k, v, o, lse, w, row, gen, _ = _case(hip, B, H, M, kind)
    monkeypatch.setenv("LJS_ATTN_BWD_PROJ_BCAST", "0")
    got = hip.attn_bwd_proj_block(q, k, v, o, row, 0, w, lse, D ** -0.5, outs=_nan_outs(B, H))
    assert hip.last_launch()["name"] == "attn_bwd_proj" and hip.attn_bwd_proj_last_path() == 0
    torch.cuda.synchronize()
    _equal(got, gen, "general phase, dense dY")
    monkeypatch.setenv("LJS_ATTN_BWD_PROJ_BCAST", "1")
    hip.attn_bwd_proj_block(q, k, v, o, row, 0, w, lse, D ** -0.5, outs=_nan_outs(B, H))
    assert hip.attn_bwd_proj_last_path() == 1


def test_equal_rows_with_a_stride_take_the_general_phase(forced):
    """A dense dY whose rows happen to be equal, padded rows (ld = M + 8): the general phase, the same bits."""
    hip = forced
    B, H, M = 2, 3, 96
    q, k, v, o, lse, w, row, gen, _ = _case(hip, B, H, M, "random")
    padded = torch.zeros(B * S, M + 8, dtype=torch.bfloat16, device=dev)
    padded[:, :M] = row
    got = hip.attn_bwd_proj_block(q, k, v, o, padded, M + 8, w, lse, D ** -0.5, outs=_nan_outs(B, H))
    assert hip.attn_bwd_proj_last_path() == 0
    torch.cuda.synchronize()
    _equal(got, gen, "general phase, dense dY")


def test_a_row_wider_than_the_row_copy_takes_the_general_phase(forced):
    """dy_ld = 0 with M = 2080 > 2048 elements (the row copy's size in LDS): the general phase on the
    broadcast row, the same bits as the dX GEMM + attn_bwd_fused pair; M = 2048 still takes the
    broadcast-row phase (64 K-tiles: four times round the sixteen stages)."""
    hip = forced
    B, H = 1, 2
    for M, path in ((2080, 0), (2048, 1)):
        q, k, v, o, lse, w, row, gen, pair = _case(hip, B, H, M, "random")
        got = hip.attn_bwd_proj_block(q, k, v, o, row, 0, w, lse, D ** -0.5, outs=_nan_outs(B, H))
        assert hip.last_launch()["name"] == "attn_bwd_proj" and hip.attn_bwd_proj_last_path() == path, M
        torch.cuda.synchronize()
        _equal(got, gen, "general phase, dense dY")
        _equal(got, pair, "dX GEMM + attn_bwd_fused")
