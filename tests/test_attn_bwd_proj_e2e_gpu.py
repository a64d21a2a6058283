"""The out-projection's input gradient handed to the attention backward (ops/linear.py ->
hip.defer_out_proj -> attn_bwd_proj): the block's loss and gradients do not change by a bit, the dX
GEMM is gone, and anything the pre-backward graph walk cannot prove safe keeps the two kernels
(run on a real MI355X: -m gpu)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture
def forced(gpu_devices):
    """One GPU, the fused backward and the hand-over's kernel forced on (4 x 8 blocks: below the
    automatic gate)."""
    gpu_devices(1)
    from learning_jax_sharding_amd.ops import hip
    hip.set_attention_bwd_fused(True)
    hip.set_attention_bwd_proj(True)
    yield hip
    hip.set_attention_bwd_fused(None)
    hip.set_attention_bwd_proj(None)


def _stats(hip):
    return dict(hip.ATTN_BWD_PROJ_STATS)


def test_block_on_equals_off(forced, monkeypatch):
    hip = forced
    from learning_jax_sharding_amd.ops import linear as L
    from learning_jax_sharding_amd.tree_util import tree_leaves
    from test_gpu_e2e import _run_block
    res, logs, stats = {}, {}, {}
    for on in (False, True):
        monkeypatch.setattr(L, "_PROJ_ON", on)
        _run_block((1, 1), B=4, S=256)   # (shadows, workspaces: the logged run launches the step only)
        s0 = _stats(hip)
        with hip.launch_log() as log:
            res[on] = _run_block((1, 1), B=4, S=256)
        assert log.total <= 32, log.total
        logs[on] = [r["name"] for r in log]
        stats[on] = {k: v - s0[k] for k, v in _stats(hip).items()}
    assert stats[False] == {"taken": 0, "materialised": 0}
    assert stats[True] == {"taken": 1, "materialised": 0}
    assert "attn_bwd_proj" in logs[True] and "attn_bwd_proj" not in logs[False]
    assert not any(n.startswith("attn_bwd_fused") for n in logs[True])
    gemms = {on: sum(n.startswith("gemm") for n in logs[on]) for on in logs}
    assert gemms[True] == gemms[False] - 1, logs   # the [T][512] <- [T][640] dX GEMM is gone
    assert res[True][0] == res[False][0]
    for a, b in zip(tree_leaves(res[True][1]), tree_leaves(res[False][1])):
        np.testing.assert_array_equal(a, b)


# ---- the two autograd nodes on plain tensors: an attention block written with the ops
B, S, H, D, M = 2, 256, 4, 64, 96


def _params():
    g = torch.Generator(device="cpu").manual_seed(3)
    mk = lambda *s: (torch.randn(*s, generator=g) * s[0] ** -0.5).cuda().requires_grad_()
    x = torch.randn(B, S, M, generator=g).to(torch.bfloat16).cuda()
    return x, [mk(M, H * D), mk(M, H * D), mk(M, H * D), mk(H * D, M)]


def _block(hip, L, x, ws, variant):
    q, k, v = (t.view(B, S, H, D) for t in L.linear(x, ws[:3], None, False, torch.bfloat16))
    hidden = hip.attention(q, k, v, D ** -0.5)
    inp = hidden
    if variant == "non_view":
        inp = hidden * 1.0
    y = L.linear(inp.reshape(B, S, H * D), [ws[3]], None, False, torch.bfloat16)[0]
    g = torch.Generator(device="cpu").manual_seed(4)
    c = torch.randn(B, S, M, generator=g).cuda()
    loss = (y.float() * c).sum()
    if variant == "second_consumer":
        loss = loss + hidden.float().sum()
    return loss


def _reference(x, ws, variant):
    xs = x.float()
    wr = [w.detach().clone().requires_grad_() for w in ws]
    q, k, v = ((xs @ w).view(B, S, H, D) for w in wr[:3])
    s = torch.einsum("btnh,bfnh->bnft", k, q) * D ** -0.5
    hidden = torch.einsum("bnft,btnh->bfnh", torch.softmax(s, -1), v)
    y = hidden.reshape(B, S, H * D) @ wr[3]
    g = torch.Generator(device="cpu").manual_seed(4)
    c = torch.randn(B, S, M, generator=g).cuda()
    loss = (y * c).sum()
    if variant == "second_consumer":
        loss = loss + hidden.sum()
    return torch.autograd.grad(loss, wr)


@pytest.mark.parametrize("variant,safe", [("plain", True), ("second_consumer", False), ("non_view", False)])
def test_graph_walk_and_fallback(forced, variant, safe):
    """Safe for the plain block (taken, no dX GEMM); with a second consumer of the attention output,
    or a non-view op between the two nodes, the pair is not marked, the dX GEMM runs, and the
    gradients match the f32 reference either way."""
    hip = forced
    from learning_jax_sharding_amd.ops import linear as L
    x, ws = _params()
    loss = _block(hip, L, x, ws, variant)
    marked = L.proj_safe_nodes([loss])
    assert len(marked) == (1 if safe else 0)
    s0 = _stats(hip)
    with L.defer_wgrads([loss], False), hip.launch_log() as log:
        grads = torch.autograd.grad(loss, ws)
    d = {k: v - s0[k] for k, v in _stats(hip).items()}
    names = [r["name"] for r in log]
    assert d == {"taken": int(safe), "materialised": 0}, d
    assert ("attn_bwd_proj" in names) == safe, names
    assert any(n.startswith("attn_bwd_fused") for n in names) == (not safe), names
    assert not hip._PROJ_PENDING
    for a, b in zip(grads, _reference(x, ws, variant)):
        err = (a.float() - b).abs().max().item()
        assert err <= 5e-2 * b.abs().max().item(), (variant, err, b.abs().max().item())


def test_no_deferral_outside_the_walk(forced):
    """A plain torch.autograd call (no pre-backward walk) never defers."""
    hip = forced
    from learning_jax_sharding_amd.ops import linear as L
    x, ws = _params()
    loss = _block(hip, L, x, ws, "plain")
    s0 = _stats(hip)
    with hip.launch_log() as log:
        torch.autograd.grad(loss, ws)
    assert _stats(hip) == s0 and not hip._PROJ_PENDING
    assert "attn_bwd_proj" not in [r["name"] for r in log]


def test_untaken_entry_is_materialised(forced):
    """A hand-over nobody takes (here: registered by hand) is launched as the GEMM it stands for."""
    hip = forced
    g = torch.Generator(device="cpu").manual_seed(5)
    dy = torch.randn(512, 96, generator=g).to(torch.bfloat16).cuda()
    w = torch.randn(256, 96, generator=g).to(torch.bfloat16).cuda()
    dx = torch.full((512, 256), float("nan"), dtype=torch.bfloat16, device="cuda")
    ref = torch.empty_like(dx)
    hip.gemm(dy, w, ref, 512, 256, 96, 96, 96, 256, True, True)
    s0 = _stats(hip)
    hip.defer_out_proj(dy, 96, w, dx, lambda: hip.gemm(dy, w, dx, 512, 256, 96, 96, 96, 256, True, True))
    hip.materialise_out_proj()
    assert _stats(hip)["materialised"] == s0["materialised"] + 1 and not hip._PROJ_PENDING
    assert torch.equal(dx, ref)


def test_two_step_capture_equals_single_steps(forced):
    hip = forced
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd import optim
    from learning_jax_sharding_amd.models import MultiHeadAttention
    from learning_jax_sharding_amd.training import TrainState
    model = MultiHeadAttention(640, heads=8, dim_head=64)
    x = ljs.random.normal(ljs.random.PRNGKey(0), (4, 256, 640))

    def make():
        params = model.init(ljs.random.PRNGKey(1), x)["params"]
        return TrainState.create(apply_fn=model.apply, params=params, tx=optim.adam(1e-3))

    def step(state, x):
        g = ljs.grad(lambda p: model.apply({"params": p}, x).sum())(state.params)
        return state.apply_gradients(grads=g)

    def steps2(state, x):
        return step(step(state, x), x)

    one = ljs.jit(step, donate_argnums=0, capture=True)
    two = ljs.jit(steps2, donate_argnums=0, capture=True)
    s0 = _stats(hip)
    s1, s2 = make(), make()
    for _ in range(2):   # 4 steps each: the first calls capture, the later ones replay
        for _ in range(2):
            s1 = one(s1, x)
        s2 = two(s2, x)
    torch.cuda.synchronize()
    d = {k: v - s0[k] for k, v in _stats(hip).items()}
    assert d["taken"] >= 3 and d["materialised"] == 0, d
    for a, b in zip(ljs.tree_util.tree_leaves(s1), ljs.tree_util.tree_leaves(s2)):
        np.testing.assert_array_equal(np.asarray(b), np.asarray(a))
