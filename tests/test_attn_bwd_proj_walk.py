"""The pre-backward graph walk that decides whether an out-projection's dX GEMM may be left to the
attention backward (ops/linear.proj_safe_nodes), on CPU graphs built from stand-in Functions with
the node names the walk looks for, and the shape half of the kernel's gate."""
import torch

from learning_jax_sharding_amd.ops import hip
from learning_jax_sharding_amd.ops import linear as L


class _Attention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q):
        return q * 2.0

    @staticmethod
    def backward(ctx, g):
        return g * 2.0


class _Linear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(x, w)
        return x @ w

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        return g @ w.t(), x.reshape(-1, x.shape[-1]).t() @ g.reshape(-1, g.shape[-1])


def _graph(variant):
    q = torch.randn(2, 4, 2, 3, requires_grad=True)
    w = torch.randn(6, 5, requires_grad=True)
    hidden = _Attention.apply(q)
    inp = hidden * 1.0 if variant == "non_view" else hidden
    y = _Linear.apply(inp.reshape(2, 4, 6), w)
    loss = y.sum()
    if variant == "second_consumer":
        loss = loss + hidden.sum()
    return loss, y, hidden


def test_plain_block_is_safe():
    loss, y, _ = _graph("plain")
    assert L.proj_safe_nodes([loss]) == {id(y.grad_fn)}


def test_second_consumer_is_unsafe():
    loss, _, _ = _graph("second_consumer")
    assert L.proj_safe_nodes([loss]) == set()


def test_non_view_op_between_is_unsafe():
    loss, _, _ = _graph("non_view")
    assert L.proj_safe_nodes([loss]) == set()


def test_seeded_attention_output_is_unsafe():
    """The attention output as a differentiated output of its own: its seed is a second gradient."""
    loss, _, hidden = _graph("plain")
    assert L.proj_safe_nodes([loss, hidden]) == set()


def test_linear_without_attention_is_unsafe():
    x = torch.randn(4, 6, requires_grad=True)
    w = torch.randn(6, 5, requires_grad=True)
    y = _Linear.apply(x.view(2, 2, 6), w)
    assert L.proj_safe_nodes([y.sum()]) == set()


def test_shape_gate():
    """ljs_attn_bwd_proj's own gate (hip.proj_shape_ok asks the launcher's plan step; the built
    library answers without a GPU), with the switch forced on so that the shape alone decides."""
    import os
    if not os.path.exists(hip._LIBPATH):
        from learning_jax_sharding_amd.csrc import build
        build.build_all()
    ok = hip.proj_shape_ok
    hip.set_attention_bwd_proj(True)
    try:
        assert ok(64, 256, 256, 8, 64, 640, 0, False)
        assert ok(1, 256, 256, 1, 64, 32, 32, False) and ok(1, 256, 256, 1, 64, 32, 40, False)
        assert not ok(64, 256, 256, 8, 64, 40, 40, False)       # M % 32
        assert not ok(64, 128, 256, 8, 64, 640, 640, False)     # the 2-D layout's 128 local queries
        assert not ok(64, 256, 128, 8, 64, 640, 640, False)
        assert not ok(64, 256, 256, 8, 32, 640, 640, False)     # head_dim
        assert not ok(64, 256, 256, 8, 64, 640, 640, True)      # causal
        assert not ok(64, 256, 256, 8, 64, 640, 636, False)     # rows shorter than M
        assert not ok(64, 256, 256, 8, 64, 640, 644, False)     # row stride % 8
    finally:
        hip.set_attention_bwd_proj(None)
