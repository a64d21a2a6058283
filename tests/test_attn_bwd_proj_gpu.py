"""The fused attention backward that forms dO = dY . Wo^T itself (attn_bwd_proj): bit-exact against
the dX GEMM followed by the fused backward, close to the f32 formulation, and refusing what its
gate excludes (run on a real MI355X: -m gpu)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

dev = torch.device("cuda", 0)
S, D = 256, 64
HIP_ERROR_INVALID_VALUE = 1


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


def _case(hip, B, H, M):
    """Inputs and the forward of one (B, H, M) case, computed once and left unchanged."""
    key = (B, H, M)
    if key not in _CASES:
        qkv = _rand(B, S, 3, H, D, seed=21)
        q, k, v = (qkv[:, :, i] for i in range(3))
        o, lse = hip.attn_fwd_lse(q, k, v, D ** -0.5)
        w = _rand(H * D, M, seed=22, scale=M ** -0.5)   # the out-projection weight, [H * 64][M]
        dy = _rand(B * S, M + 8, seed=23)                # rows with 8 columns of padding
        _CASES[key] = (q, k, v, o, lse, w, dy)
    return _CASES[key]


def _dy_view(dy, M, mode):
    """(tensor handed to the kernels, row stride, the dense [T][M] matrix it stands for)."""
    T = dy.shape[0]
    if mode == "row":
        row = dy[0, :M].contiguous()
        return row, 0, row.unsqueeze(0).expand(T, M)
    if mode == "dense":
        t = dy[:, :M].contiguous()
        return t, M, t
    return dy, M + 8, dy[:, :M]


@pytest.mark.parametrize("mode", ["row", "dense", "padded"])
@pytest.mark.parametrize("B,H,M", [(1, 1, 32), (2, 3, 96), (3, 8, 160), (5, 2, 640)])
def test_bit_exact_against_two_kernels(forced, B, H, M, mode):
    hip = forced
    q, k, v, o, lse, w, dy = _case(hip, B, H, M)
    t, ld, _ = _dy_view(dy, M, mode)
    # the two-kernel path: the out-projection's dX GEMM as ops/linear.py launches it, then the
    # fused backward over the materialised dO
    do = torch.full((B * S, H * D), float("nan"), dtype=torch.bfloat16, device=dev)
    hip.gemm(t, w, do, B * S, H * D, M, ld, M, H * D, True, True)
    ref = hip.attn_bwd_block(q, k, v, o, do.view(B, S, H, D), lse, D ** -0.5)
    assert hip.last_launch()["name"].startswith("attn_bwd_fused")
    got = hip.attn_bwd_proj_block(q, k, v, o, t, ld, w, lse, D ** -0.5)
    rec = hip.last_launch()
    assert rec["name"] == "attn_bwd_proj" and rec["blocks"] == B * H, rec
    torch.cuda.synchronize()
    for a, b, name in zip(got, ref, ("dq", "dk", "dv")):
        assert torch.equal(a, b), (name, (a.float() - b.float()).abs().max().item())


@pytest.mark.parametrize("B,H,M", [(2, 3, 96), (5, 2, 640)])
def test_against_f32_reference(forced, B, H, M):
    hip = forced
    q, k, v, o, lse, w, dy = _case(hip, B, H, M)
    t, ld, dense = _dy_view(dy, M, "padded")
    got = hip.attn_bwd_proj_block(q, k, v, o, t, ld, w, lse, D ** -0.5)
    assert hip.last_launch()["name"] == "attn_bwd_proj"
    do = (dense.float() @ w.float().t()).to(torch.bfloat16).view(B, S, H, D)
    qr, kr, vr = (x.detach().float().requires_grad_() for x in (q, k, v))
    s = torch.einsum("btnh,bfnh->bnft", kr, qr) * D ** -0.5
    of = torch.einsum("bnft,btnh->bfnh", torch.softmax(s, -1), vr)
    (of * do.float()).sum().backward()
    for a, b, name in zip(got, (qr.grad, kr.grad, vr.grad), ("dq", "dk", "dv")):
        err = (a.float() - b).abs().max().item()
        assert err <= 3e-2 * max(1.0, b.abs().max().item()), (name, err)


@pytest.mark.parametrize("what", ["M=40", "misaligned", "causal"])
def test_entry_point_rejects(forced, what):
    hip = forced
    B, H, M = 2, 3, 96
    q, k, v, o, lse, w, dy = _case(hip, B, H, M)
    t, ld, _ = _dy_view(dy, M, "dense")
    causal = what == "causal"
    if what == "M=40":
        w = w[:, :40].contiguous()
        t, ld = t[:, :40].contiguous(), 40
    elif what == "misaligned":
        t = torch.cat([t.reshape(-1), t.new_zeros(8)])[4:4 + B * S * M]   # 8 bytes past a 16-byte boundary
        assert t.data_ptr() % 16 == 8
    assert not hip.attn_bwd_proj_ok(q, k, v, o, t, ld, w, causal)
    outs = tuple(torch.empty((B, S, H, D), dtype=torch.bfloat16, device=dev) for _ in range(3))
    n0 = hip.lib().ljs_launch_count()
    rc = hip.lib().ljs_attn_bwd_proj(
        hip._p(q), hip._p(k), hip._p(v), hip._p(o), hip._p(t), ld, hip._p(w), w.shape[1], hip._p(lse),
        *(hip._p(x) for x in outs), B, S, S, H, *(hip._longs(hip._strides3(x)) for x in (q, k, v, o) + outs),
        D ** -0.5, int(causal), hip._stream(q))
    assert rc == HIP_ERROR_INVALID_VALUE
    assert hip.lib().ljs_launch_count() == n0


def test_automatic_gate(hip):
    """None: where the fused backward is chosen, from 192 (batch, head) pairs (the 128-pair step
    keeps the dX GEMM + fused backward pair that test_production_picks_run_as_picked pins)."""
    hip.set_attention_bwd_proj(None)
    assert not hip.lib().ljs_attn_bwd_proj_enabled(4, 8)
    assert not hip.lib().ljs_attn_bwd_proj_enabled(16, 8)
    assert hip.lib().ljs_attn_bwd_proj_enabled(24, 8)
    assert hip.lib().ljs_attn_bwd_proj_enabled(64, 8)
    hip.set_attention_bwd_fused(False)
    assert not hip.lib().ljs_attn_bwd_proj_enabled(64, 8)
    hip.set_attention_bwd_fused(None)
    hip.set_attention_bwd_proj(False)
    assert not hip.lib().ljs_attn_bwd_proj_enabled(64, 8)
    hip.set_attention_bwd_proj(None)
