"""attn_bwd_proj's K-loop with its two load streams split by wave (tile waves 0-3: dY / Wo K-tiles;
piece waves 4-7: K / V / Q / O / lse prologue pieces): bit-exact against the dX GEMM followed by the
fused backward at step counts around the ring depth and the piece pacing, with no prologue piece
left unissued or unwaited, and on strided operand views (run on a real MI355X: -m gpu)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

dev = torch.device("cuda", 0)
S, D = 256, 64


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from learning_jax_sharding_amd.ops import hip as H
    H.lib()
    return H


@pytest.fixture
def forced(hip):
    hip.set_attention_bwd_fused(True)
    hip.set_attention_bwd_proj(True)
    yield hip
    hip.set_attention_bwd_fused(None)
    hip.set_attention_bwd_proj(None)


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16).to(dev)


_CASES = {}


def _case(hip, B, H, M, seed=41):
    """Inputs, the forward and the materialised-dO pieces of one (B, H, M, seed) case, computed once
    and left unchanged."""
    key = (B, H, M, seed)
    if key not in _CASES:
        qkv = _rand(B, S, 3, H, D, seed=seed)
        q, k, v = (qkv[:, :, i] for i in range(3))       # strided views of the [B, S, 3, H, D] tensor
        o, lse = hip.attn_fwd_lse(q, k, v, D ** -0.5)
        w = _rand(H * D, M, seed=seed + 1, scale=M ** -0.5)
        dy = _rand(B * S, M + 8, seed=seed + 2)            # rows with 8 columns of padding
        _CASES[key] = (q, k, v, o, lse, w, dy)
    return _CASES[key]


def _dy_view(dy, M, mode):
    """(tensor handed to the kernels, row stride)."""
    if mode == "row":
        return dy[0, :M].contiguous(), 0
    if mode == "dense":
        return dy[:, :M].contiguous(), M
    return dy, M + 8


_REFS = {}


def _two_kernel(hip, key, q, k, v, o, lse, w, t, ld, B, H, M):
    """dq / dk / dv of the dX GEMM followed by the fused backward over the materialised dO."""
    if key not in _REFS:
        do = torch.full((B * S, H * D), float("nan"), dtype=torch.bfloat16, device=dev)
        hip.gemm(t, w, do, B * S, H * D, M, ld, M, H * D, True, True)
        ref = hip.attn_bwd_block(q, k, v, o, do.view(B, S, H, D), lse, D ** -0.5)
        assert hip.last_launch()["name"].startswith("attn_bwd_fused")
        _REFS[key] = ref
    return _REFS[key]


def _proj(hip, q, k, v, o, lse, w, t, ld, B, H):
    got = hip.attn_bwd_proj_block(q, k, v, o, t, ld, w, lse, D ** -0.5)
    rec = hip.last_launch()
    assert rec["name"] == "attn_bwd_proj" and rec["blocks"] == B * H, rec
    return got


def _same(got, ref):
    torch.cuda.synchronize()
    for a, b, name in zip(got, ref, ("dq", "dk", "dv")):
        assert torch.equal(a, b), (name, (a.float() - b.float()).abs().max().item())


# nk = M / 32 K-tile steps: 1 and 2 (fewer than the ring's three stages), 3 (its first wrap), 11 and
# 12 (one fewer than, and as many as, the one-piece-per-step loop needed for a wave's 11 pieces)
@pytest.mark.parametrize("mode", ["row", "dense", "padded"])
@pytest.mark.parametrize("B,H,M", [(1, 1, 32), (1, 2, 64), (2, 1, 96), (1, 3, 352), (2, 2, 384)])
def test_bit_exact_over_step_counts(forced, B, H, M, mode):
    hip = forced
    q, k, v, o, lse, w, dy = _case(hip, B, H, M)
    t, ld = _dy_view(dy, M, mode)
    ref = _two_kernel(hip, (B, H, M, 41, mode), q, k, v, o, lse, w, t, ld, B, H, M)
    _same(_proj(hip, q, k, v, o, lse, w, t, ld, B, H), ref)


def test_no_stale_lds_between_launches(forced):
    """Inputs X, then independent inputs Y, back to back on one stream: a prologue piece that was
    never issued, or not waited for, would leave X's K / V / Q / O / lse in Y's block."""
    hip = forced
    B, H, M = 2, 2, 96
    xs = _case(hip, B, H, M, seed=51)
    ys = _case(hip, B, H, M, seed=61)
    refs = []
    for seed, (q, k, v, o, lse, w, dy) in ((51, xs), (61, ys)):
        t, ld = _dy_view(dy, M, "dense")
        refs.append(_two_kernel(hip, (B, H, M, seed, "dense"), q, k, v, o, lse, w, t, ld, B, H, M))
    torch.cuda.synchronize()
    gots = []
    for q, k, v, o, lse, w, dy in (xs, ys):
        t, ld = _dy_view(dy, M, "dense")
        gots.append(_proj(hip, q, k, v, o, lse, w, t, ld, B, H))   # no synchronisation in between
    _same(gots[1], refs[1])
    _same(gots[0], refs[0])


def test_strided_views_and_other_o_head_stride(forced):
    """Q / K / V as slices of the [B, S, 3, H, D] tensor (row stride 3 H D) and O as every second
    head of a [B, S, 2 H, D] buffer (head stride 2 D, row stride 2 H D)."""
    hip = forced
    B, H, M = 2, 3, 96
    q, k, v, o, lse, w, dy = _case(hip, B, H, M)
    assert q.stride(1) == 3 * H * D and not q.is_contiguous()
    wide = torch.full((B, S, 2 * H, D), float("nan"), dtype=torch.bfloat16, device=dev)
    o2 = wide[:, :, 1::2]
    o2.copy_(o)
    assert o2.stride(2) == 2 * D != o.stride(2) and torch.equal(o2, o)
    t, ld = _dy_view(dy, M, "padded")
    ref = _two_kernel(hip, (B, H, M, 41, "padded"), q, k, v, o, lse, w, t, ld, B, H, M)
    _same(_proj(hip, q, k, v, o2, lse, w, t, ld, B, H), ref)
