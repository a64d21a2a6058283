"""LayerNorm / RMSNorm layers, their dispatch to the fused kernels, and the pre-norm
TransformerLayer, on host devices."""
import warnings

import numpy as np
import pytest
import torch


def _oracle(x, scale, bias, kind, eps=1e-6):
    """The float64 formulas: (x - mean) rsqrt(var + eps) scale + bias / x rsqrt(mean(x^2) + eps) scale."""
    x = x.double()
    if kind == "layer":
        x = x - x.mean(-1, keepdim=True)
    y = x * torch.rsqrt((x * x).mean(-1, keepdim=True) + eps)
    if scale is not None:
        y = y * scale.double()
    if bias is not None:
        y = y + bias.double()
    return y


def _layer_run(kind, n, spec, mesh_shape, D=64):
    """(y, dscale, dbias or None, plan records) of the layer applied to a sharded x, with scale and
    bias set to random values, for the loss sum(y * w)."""
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd import nn
    from learning_jax_sharding_amd.mesh import Mesh, create_device_mesh
    from learning_jax_sharding_amd.sharding import NamedSharding
    from learning_jax_sharding_amd.spmd import plan as _plan
    mesh = Mesh(create_device_mesh(mesh_shape), ("data", "model"))
    model = nn.LayerNorm() if kind == "layer" else nn.RMSNorm()
    gen = torch.Generator().manual_seed(11)
    x = 3.0 + 1.5 * torch.randn(4, 8, D, generator=gen)
    w = torch.randn(4, 8, D, generator=gen)
    params = {"scale": 1.0 + 0.2 * torch.randn(D, generator=gen)}
    if kind == "layer":
        params["bias"] = 0.2 * torch.randn(D, generator=gen)
    sh = NamedSharding(mesh, spec)
    xs, ws = ljs.device_put(x.numpy(), sh), ljs.device_put(w.numpy(), sh)
    ps = ljs.device_put({k: v.numpy() for k, v in params.items()})

    def loss(p):
        return (model.apply({"params": p}, xs) * ws).sum()

    with mesh, _plan.record_plan() as rec:
        y = model.apply({"params": ps}, xs)
        g = ljs.grad(loss)(ps)
    return x, w, params, np.asarray(y), {k: np.asarray(v) for k, v in g.items()}, rec


@pytest.mark.parametrize("kind", ["layer", "rms"])
@pytest.mark.parametrize("n,mesh_shape,spec", [(1, (1, 1), ("data", "model")), (4, (4, 1), ("data",)),
                                               (4, (1, 4), (None, "model")), (4, (2, 2), ("data", "model")),
                                               (4, (1, 4), (None, None, "model"))],
                         ids=["1dev", "batch4", "seq4", "batch2xseq2", "features4"])
def test_layers_match_float64_formulas(host_devices, kind, n, mesh_shape, spec):
    """Batch-, sequence- and feature-sharded (the last: the composite with its all-reduced row
    statistics) values and parameter gradients against the float64 formulas.  f32 arithmetic over
    64-term sums of order-1 values: within 1e-5."""
    from learning_jax_sharding_amd.sharding import PartitionSpec as P
    host_devices(n)
    x, w, params, y, g, rec = _layer_run(kind, n, P(*spec), mesh_shape)
    xs = x.double()
    ps = {k: v.double().requires_grad_(True) for k, v in params.items()}
    want = _oracle(xs, ps["scale"], ps.get("bias"), kind)
    np.testing.assert_allclose(y, want.detach().numpy(), rtol=1e-5, atol=1e-5)
    grads = torch.autograd.grad((want * w.double()).sum(), list(ps.values()))
    for k, gw in zip(ps, grads):
        np.testing.assert_allclose(g[k], gw.numpy(), rtol=1e-5, atol=1e-5 * float(gw.abs().max()), err_msg=k)
    assert y.dtype == np.float32
    # host devices never take the fused op
    assert not [s for s in rec.steps if s.kind == "layer_norm"]


def test_core_layer_norm_on_host(host_devices):
    """ops.core.layer_norm itself: whole features -> x's sharding kept, parameters replicated, the
    op recorded; sharded features -> None (the caller composes the norm)."""
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd.mesh import Mesh, create_device_mesh
    from learning_jax_sharding_amd.ops import core
    from learning_jax_sharding_amd.sharding import NamedSharding, PartitionSpec as P
    from learning_jax_sharding_amd.spmd import plan as _plan
    host_devices(4)
    mesh = Mesh(create_device_mesh((2, 2)), ("data", "model"))
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(4, 8, 64, generator=gen)
    scale, bias = 1.0 + 0.2 * torch.randn(64, generator=gen), 0.2 * torch.randn(64, generator=gen)
    xs = ljs.device_put(x.numpy(), NamedSharding(mesh, P("data", "model")))
    sc, bi = ljs.device_put(scale.numpy()), ljs.device_put(bias.numpy())
    with mesh, _plan.record_plan() as rec:
        for kind in ("layer", "rms"):
            y = core.layer_norm(xs, sc, bi, 1e-6, kind, torch.bfloat16)
            assert y.dtype == torch.bfloat16 and y.sharding == xs.sharding
            want = _oracle(x, scale, bias if kind == "layer" else None, kind)
            np.testing.assert_allclose(np.asarray(y.astype(torch.float32)), want.numpy(), rtol=2.0 ** -7, atol=1e-5)
        xf = ljs.device_put(x.numpy(), NamedSharding(mesh, P(None, None, "model")))
        assert core.layer_norm(xf, sc, bi) is None
    assert [s.info["norm"] for s in rec.steps if s.kind == "layer_norm"] == ["layer", "rms"]
    with pytest.raises(ValueError):
        core.layer_norm(xs, sc, bi, kind="batch")


def test_norm_dispatch(monkeypatch):
    """The per-shard entry point takes the HIP kernels for a GPU tensor of 8..8192 features in
    multiples of 8, f32 or bf16; another width runs the torch formulation, warned once per width;
    meta tensors and LJS_FUSED_NORM=0 never take them."""
    from learning_jax_sharding_amd.ops import kernels as K
    assert not K._hip_norm(torch.empty(4, 640, device="meta"), torch.float32)   # the real use_hip
    assert not K._hip_norm(torch.zeros(4, 640), torch.float32)                  # a host tensor
    monkeypatch.setattr(K, "use_hip", lambda t: not t.is_meta)
    monkeypatch.setattr(K, "_WARNED_NORM_D", set())
    monkeypatch.delenv("LJS_FUSED_NORM", raising=False)
    for dt in (torch.float32, torch.bfloat16):
        assert K._hip_norm(torch.zeros(4, 640, dtype=dt), torch.bfloat16)
        assert K._hip_norm(torch.zeros(2, 3, 8, dtype=dt), torch.float32)
        assert K._hip_norm(torch.zeros(1, 8192, dtype=dt), dt)
    assert not K._hip_norm(torch.zeros(4, 640, dtype=torch.float64), torch.float32)
    assert not K._hip_norm(torch.zeros(4, 640, dtype=torch.float16), torch.float16)
    assert not K._hip_norm(torch.empty(4, 640, device="meta"), torch.float32)
    with pytest.warns(UserWarning, match="100 features"):
        assert not K._hip_norm(torch.zeros(4, 100), torch.float32)
    with pytest.warns(UserWarning, match="8200 features"):
        assert not K._hip_norm(torch.zeros(4, 8200), torch.float32)
    with warnings.catch_warnings():
        warnings.simplefilter("error")     # once per width
        assert not K._hip_norm(torch.zeros(4, 100), torch.float32)
    monkeypatch.setenv("LJS_FUSED_NORM", "0")
    assert not K._hip_norm(torch.zeros(4, 640), torch.float32)
    # and what runs instead is the torch formulation, differentiable by autograd
    x = torch.randn(4, 100, requires_grad=True)
    y = K.layer_norm(x, torch.ones(100), None, 1e-6, "rms", torch.float32)
    np.testing.assert_allclose(y.detach().numpy(), _oracle(x.detach(), None, None, "rms").numpy(), rtol=1e-5,
                               atol=1e-5)
    y.sum().backward()
    assert x.grad is not None and torch.isfinite(x.grad).all()


def _layer_model(norm, **kw):
    from learning_jax_sharding_amd.models import TransformerLayer
    return TransformerLayer(64, heads=2, dim_head=16, ff_dim=128, norm=norm, **kw)


@pytest.mark.parametrize("norm", ["layer", "rms"])
def test_prenorm_transformer_layer_on_host(host_devices, norm):
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd import nn, optim
    from learning_jax_sharding_amd.training import TrainState
    host_devices(1)
    model = _layer_model(norm)
    x = ljs.random.normal(ljs.random.PRNGKey(0), (2, 16, 64))

    def init_fn(k, x):
        return TrainState.create(apply_fn=model.apply, params=model.init(k, x)["params"], tx=optim.adam(1e-2))

    abstract = ljs.eval_shape(init_fn, ljs.random.PRNGKey(1), x)
    state = init_fn(ljs.random.PRNGKey(1), x)
    names = {f"{k}/{n}" for k, v in nn.unbox(state.params).items() for n in v}
    want = {"norm1/scale", "norm2/scale"} | ({"norm1/bias", "norm2/bias"} if norm == "layer" else set())
    assert want <= names and {n for n in names if n.startswith("norm")} == want
    a_names = {f"{k}/{n}" for k, v in nn.unbox(abstract.params).items() for n in v}
    assert a_names == names
    assert tuple(nn.unbox(abstract.params)["norm1"]["scale"].shape) == (64,)
    y = model.apply({"params": state.params}, x)
    assert tuple(y.shape) == (2, 16, 64) and y.dtype == torch.bfloat16

    def loss(p):
        return (model.apply({"params": p}, x).astype(torch.float32) ** 2).sum()

    before = np.asarray(nn.unbox(state.params)["norm1"]["scale"]).copy()
    l0, g = ljs.value_and_grad(loss)(state.params)
    state = state.apply_gradients(grads=g)
    after = np.asarray(nn.unbox(state.params)["norm1"]["scale"])
    assert int(np.asarray(state.step)) == 1
    assert np.isfinite(float(np.asarray(l0))) and np.isfinite(after).all() and not np.array_equal(before, after)
    with pytest.raises(ValueError):
        _layer_model("batch").init(ljs.random.PRNGKey(1), x)


def test_transformer_layer_without_norm_is_unchanged(host_devices):
    """The default layer has today's parameter tree, and norm=None is the default, bit for bit."""
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd import nn
    from learning_jax_sharding_amd.models import TransformerLayer
    host_devices(1)
    x = ljs.random.normal(ljs.random.PRNGKey(0), (2, 16, 64))
    default = TransformerLayer(64, heads=2, dim_head=16, ff_dim=128)
    assert default.norm is None
    p0 = nn.unbox(default.init(ljs.random.PRNGKey(1), x)["params"])
    assert {k: sorted(v) for k, v in p0.items()} == {"attn": ["to_k", "to_out_0", "to_q", "to_v"],
                                                     "ff": ["w_in", "w_out"]}
    p1 = nn.unbox(_layer_model(None).init(ljs.random.PRNGKey(1), x)["params"])
    l0, l1 = ljs.tree_util.tree_leaves(p0), ljs.tree_util.tree_leaves(p1)
    assert len(l0) == len(l1) == 7   # four projection kernels, the out-projection bias, two FF kernels
    for a, b in zip(l0, l1):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    y0 = default.apply({"params": p0}, x)
    y1 = _layer_model(None).apply({"params": p1}, x)
    assert np.array_equal(np.asarray(y0.astype(torch.float32)), np.asarray(y1.astype(torch.float32)))


def test_norm_instances_use_no_scratch():
    """Every instance of the two norm kernels (2 kinds x 2 x 2 dtypes x 3 mappings, forward and
    backward) is in the gfx950 code object and keeps its rows in registers: no scratch, no spills."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "learning_jax_sharding_amd", "_lib", "libljs_kernels.so")
    if not os.path.exists(lib):
        from learning_jax_sharding_amd.csrc import build
        build.build_all()
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(root, "scripts",
                                                                                   "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    res = {n: k for n, k in kr.resources(lib).items() if "norm_fwd_kernel" in n or "norm_bwd_kernel" in n}
    assert len([n for n in res if "norm_fwd_kernel" in n]) == 24 and len(res) == 48, sorted(res)
    for n, k in res.items():
        assert k.get("scratch", 0) == 0 and k.get("vgpr_spill", 0) == 0 and k.get("sgpr_spill", 0) == 0, (n, k)
