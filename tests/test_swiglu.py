"""SwiGLU on host devices: the torch formulation (ops/kernels.py swiglu_reference, the semantics the
HIP kernels share) against the float64 oracle of tests/swiglu_oracle.py, the sharded ``core.swiglu``,
``nn.GatedFeedForward`` and the ``ff`` field of the model classes."""
import numpy as np
import pytest
import torch

import swiglu_oracle as O

F32, BF16 = torch.float32, torch.bfloat16
_DT = {F32: "f32", BF16: "bf16"}
PAIRS = [(a, b) for a in (F32, BF16) for b in (F32, BF16)]


# ------------------------------------------------------------------------------------ reference
@pytest.mark.parametrize("idt,odt", PAIRS, ids=[f"{_DT[a]}-{_DT[b]}" for a, b in PAIRS])
def test_reference_matches_float64_oracle(idt, odt):
    """Forward and the explicit backward of the torch formulation under the oracle's bounds."""
    from learning_jax_sharding_amd.ops import kernels as K
    g, u, dh = O.inputs((3, 41, 264), idt, odt)
    assert (g == 0).sum() >= 2 and g.max() == 80 and g.min() == -80
    assert ((g.float() > -1.4) & (g.float() < -1.1)).sum() >= 8
    gs, us = g.clone().requires_grad_(True), u.clone().requires_grad_(True)
    h = K.swiglu_reference(gs, us, odt)
    assert h.dtype == odt
    dg, du = torch.autograd.grad(h, [gs, us], dh)
    assert dg.dtype == idt and du.dtype == idt
    tag = f"ref {_DT[idt]}->{_DT[odt]}"
    O.check(f"{tag} h", h, *O.forward64(g, u), O.U_H)
    dg64, mdg, du64, mdu = O.backward64(g, u, dh)
    O.check(f"{tag} dg", dg, dg64, mdg, O.U_DG)
    O.check(f"{tag} du", du, du64, mdu, O.U_DU)


def test_reference_backward_is_explicit_and_stable():
    """The backward is the Function's own (not the autograd of a composite), and c = 1 - sigmoid(g) keeps
    its relative accuracy where the subtraction would lose it: at g = 40 sigmoid(g) rounds to 1 in f32
    and 1 - s is 0, while c is exp(-40) to a few units."""
    from learning_jax_sharding_amd.ops import kernels as K
    g = torch.tensor([40.0, -40.0, 17.0], requires_grad=True)
    h = K.swiglu_reference(g, torch.ones(3))
    assert "SwigluReference" in type(h.grad_fn).__name__
    s, c = K._sigmoid_pair(g.detach())
    want_c = torch.sigmoid(-g.detach().double())
    assert float(((c.double() - want_c).abs() / want_c).max()) <= 4 * 2.0 ** -24
    assert float(1.0 - s[0]) == 0.0 and float(c[0]) > 0.0      # what the subtraction would have lost


def test_oracle_gradients_match_finite_differences():
    """The oracle's dg and du against central differences of its own float64 forward (a sign or
    formula error in the oracle itself would show here): relative 1e-7 of the term sum."""
    g = torch.tensor([-30.0, -3.0, -1.278, -0.5, 0.0, 0.7, 2.5, 30.0], dtype=torch.float64)
    u = torch.tensor([1.5, -0.75, 2.0, 0.3, -1.1, 0.9, -2.2, 0.6], dtype=torch.float64)
    dh = torch.tensor([0.5, 1.25, -0.8, 1.0, -1.5, 0.4, 0.9, -0.3], dtype=torch.float64)
    dg, mdg, du, mdu = O.backward64(g, u, dh)
    eps = 1e-6
    fd_g = dh * (O.forward64(g + eps, u)[0] - O.forward64(g - eps, u)[0]) / (2 * eps)
    fd_u = dh * (O.forward64(g, u + eps)[0] - O.forward64(g, u - eps)[0]) / (2 * eps)
    scale = dh.abs() * u.abs() + dh.abs() * g.abs() + 1e-30
    print(f"swiglu-figures fd dg={(fd_g - dg).abs().max():.3e} du={(fd_u - du).abs().max():.3e}")
    assert ((fd_g - dg).abs() <= 1e-7 * scale).all() and ((fd_u - du).abs() <= 1e-7 * scale).all()
    # and torch's own autograd of the float64 composite agrees
    g2, u2 = g.clone().requires_grad_(True), u.clone().requires_grad_(True)
    ag, au = torch.autograd.grad(torch.nn.functional.silu(g2) * u2, [g2, u2], dh)
    assert torch.allclose(ag, dg, rtol=1e-12, atol=1e-300) and torch.allclose(au, du, rtol=1e-12, atol=1e-300)


def test_derived_constants_cover_the_error_expressions():
    """U_H, U_DU and U_DG are at least the suprema of the docstring's error expressions (7 and 9, both
    as g -> 0 from below), with at most one unit to spare."""
    g = torch.cat([torch.linspace(-80, 80, 400001, dtype=torch.float64),
                   torch.tensor([-1e-9, 1e-9], dtype=torch.float64)])
    fwd, dg = O.derived_units(g)
    print(f"swiglu-figures derived sup h/du={float(fwd.max()):.4f} dg={float(dg.max()):.4f}")
    assert float(fwd.max()) <= O.U_H <= float(fwd.max()) + 1 and O.U_DU == O.U_H
    assert float(dg.max()) <= O.U_DG <= float(dg.max()) + 1


def test_dispatch_on_host_and_meta_tensors(monkeypatch):
    """Host and meta tensors take the torch formulation whatever LJS_FUSED_SWIGLU says, with no warning."""
    import warnings
    from learning_jax_sharding_amd.ops import kernels as K
    g, u, _ = O.inputs((2, 3, 12), F32, F32)
    for v in ("0", "1"):
        monkeypatch.setenv("LJS_FUSED_SWIGLU", v)
        assert K.fused_swiglu_enabled() == (v == "1")
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            h = K.swiglu(g, u, BF16)
            hm = K.swiglu(g.to("meta"), u.to("meta"), BF16)
        assert torch.equal(h, K.swiglu_reference(g, u, BF16))
        assert hm.is_meta and hm.dtype == BF16 and tuple(hm.shape) == (2, 3, 12)


def test_swiglu_instances_use_no_scratch():
    """Every instance of the kernel is in the gfx950 code object (f32 / bf16 in x f32 / bf16 out x
    forward / backward = 8), uses no scratch and no LDS, spills nothing, and stays within 64 VGPRs."""
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
    res = {n: k for n, k in kr.resources(lib).items() if "swiglu_kernel" in n}
    assert len(res) == 8, sorted(res)
    for n, k in res.items():
        assert k.get("scratch", 0) == 0 and k.get("vgpr_spill", 0) == 0 and k.get("sgpr_spill", 0) == 0, (n, k)
        assert k.get("lds", 0) == 0 and k["vgpr"] <= 64, (n, k)


# ------------------------------------------------------------------------------------ core.swiglu
def _put(x, mesh_shape, spec):
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd.mesh import Mesh, create_device_mesh
    from learning_jax_sharding_amd.sharding import NamedSharding, PartitionSpec as P
    mesh = Mesh(create_device_mesh(mesh_shape), ("data", "model"))
    return ljs.device_put(x.numpy(), NamedSharding(mesh, P(*spec)))


def test_sharded_swiglu_equals_one_device(host_devices):
    """On a 2 x 2 mesh with batch over data and the feature dim over model: the one-device bits, gate's
    sharding kept, one ``swiglu`` plan step and nothing else (no collective); an ``up`` laid out otherwise
    is resharded onto gate's tile first."""
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd.ops import core
    from learning_jax_sharding_amd.ops import kernels as K
    from learning_jax_sharding_amd.spmd import plan as _plan
    g, u, dh = O.inputs((4, 6, 16), F32, F32)
    host_devices(1)
    one = core.swiglu(_put(g, (1, 1), ()), _put(u, (1, 1), ()), dtype=BF16).to_torch()
    assert one.dtype == BF16 and torch.equal(one, K.swiglu_reference(g, u, BF16))
    host_devices(4)
    spec = ("data", None, "model")
    gs, us = _put(g, (2, 2), spec), _put(u, (2, 2), spec)
    with _plan.record_plan() as rec:
        hs = core.swiglu(gs, us, dtype=BF16)
    assert [s.kind for s in rec.steps] == ["swiglu"], [s.kind for s in rec.steps]
    assert tuple(rec.steps[0].info["tiles"]) == (2, 1, 2)
    assert hs.tile == gs.tile and hs.dtype == BF16
    assert torch.equal(hs.to_torch(), one)
    u_other = _put(u, (2, 2), (None, "model"))
    assert u_other.tile != gs.tile
    with _plan.record_plan() as rec:
        h2 = core.swiglu(gs, u_other, dtype=BF16)
    kinds = [s.kind for s in rec.steps]
    assert kinds.count("swiglu") == 1 and len(kinds) > 1, kinds      # the reshard of up shows in the plan
    assert h2.tile == gs.tile and torch.equal(h2.to_torch(), one)
    # gradients flow to both operands through the sharded op
    val, (dg, du) = ljs.value_and_grad(lambda a, b: core.swiglu(a, b).sum(), argnums=(0, 1))(gs, us)
    dg64, _, du64, _ = O.backward64(g, u, torch.ones_like(g))
    assert torch.allclose(dg.to_torch().double(), dg64, rtol=1e-5, atol=1e-6)
    assert torch.allclose(du.to_torch().double(), du64, rtol=1e-5, atol=1e-6)
    with pytest.raises(ValueError):
        core.swiglu(gs, _put(u[:, :3], (1, 1), ()))


# ------------------------------------------------------------------------------------ modules
def test_gated_feed_forward_parameters(host_devices):
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd import nn
    host_devices(1)
    model = nn.GatedFeedForward(48)
    assert not hasattr(model, "fp8")
    x = ljs.random.normal(ljs.random.PRNGKey(0), (2, 8, 32))
    params = model.init(ljs.random.PRNGKey(1), x)["params"]
    assert sorted(params) == ["w_gate", "w_out", "w_up"]
    shapes = ljs.tree_map(lambda a: (tuple(a.shape), a.dtype), nn.unbox(params))
    assert shapes == {"w_gate": ((32, 48), F32), "w_up": ((32, 48), F32), "w_out": ((48, 32), F32)}
    axes = {k: tuple(v.names) for k, v in params.items()}
    assert axes == {"w_gate": ("embed", "hidden"), "w_up": ("embed", "hidden"), "w_out": ("hidden", "embed")}
    # the module computes what it says, residual included (f32 compute: the formula to 1e-5)
    m32 = nn.GatedFeedForward(48, dtype=F32)
    y = m32.apply({"params": params}, x, residual=x).to_torch()
    p = ljs.tree_map(lambda a: a.to_torch(), nn.unbox(params))
    xt = x.to_torch()
    want = xt + (torch.nn.functional.silu(xt @ p["w_gate"]) * (xt @ p["w_up"])) @ p["w_out"]
    np.testing.assert_allclose(y.numpy(), want.numpy(), rtol=1e-5, atol=1e-5 * want.abs().max().item())


def _gff_loss_and_grads(mesh_shape, B=4, S=64, M=128, F=512):
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd import nn
    from learning_jax_sharding_amd.mesh import Mesh, create_device_mesh
    from learning_jax_sharding_amd.parallel.tensor import MEGATRON_RULES as rules
    from learning_jax_sharding_amd.sharding import NamedSharding, PartitionSpec as P
    from learning_jax_sharding_amd.spmd import plan as _plan
    mesh = Mesh(create_device_mesh(mesh_shape), ("data", "model"))
    model = nn.GatedFeedForward(F)
    x = ljs.random.normal(ljs.random.PRNGKey(0), (B, S, M))
    params = model.init(ljs.random.PRNGKey(1), x)["params"]
    params = ljs.device_put(params, nn.logical_to_mesh_sharding(nn.get_partition_spec(params), mesh, rules))
    x = ljs.device_put(x, NamedSharding(mesh, P("data")))

    def loss(p):
        y = model.apply({"params": p}, x, residual=x)
        return (y.astype(ljs.numpy.float32) * y.astype(ljs.numpy.float32)).sum()

    with mesh, nn.axis_rules(rules), _plan.record_plan() as rec:
        y = model.apply({"params": params}, x, residual=x)
        val, g = ljs.value_and_grad(loss)(params)
    spec = ljs.tree_map(lambda a: tuple(a.tile.tile_shape), nn.unbox(params))
    grads = ljs.tree_map(lambda a: np.asarray(a), nn.unbox(g))
    return float(np.asarray(val)), np.asarray(y.astype(ljs.numpy.float32)), grads, rec.steps, spec


def test_gated_feed_forward_megatron_matches_single_device(host_devices):
    """Under MEGATRON_RULES on 2 x 2 host devices (hidden over model): the output, the loss and the three
    weight gradients against the single-device module, within tests/test_ff_tp.py's tolerances for the same
    comparison; the activation runs on hidden shards."""
    host_devices(4)
    v1, y1, g1, _, _ = _gff_loss_and_grads((1, 1))
    vn, yn, gn, steps, spec = _gff_loss_and_grads((2, 2))
    assert spec == {"w_gate": (1, 2), "w_up": (1, 2), "w_out": (2, 1)}
    sw = [s for s in steps if s.kind == "swiglu"]
    assert len(sw) == 2 and all(tuple(s.info["tiles"])[-1] == 2 for s in sw), [s.kind for s in steps]
    assert abs(v1 - vn) <= 3e-2 * max(1.0, abs(v1)), (v1, vn)
    np.testing.assert_allclose(yn, y1, rtol=5e-2, atol=5e-2 * np.abs(y1).max(), err_msg="output")
    assert sorted(g1) == ["w_gate", "w_out", "w_up"]
    for name in g1:
        a, b = g1[name], gn[name]
        np.testing.assert_allclose(b, a, rtol=5e-2, atol=5e-2 * np.abs(a).max(), err_msg=name)


LM = dict(vocab_size=64, dim=32, layers=2, heads=2, dim_head=16)


def _paths(lm):
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd import nn
    from learning_jax_sharding_amd.models import TransformerLM
    model = TransformerLM(**lm)
    ids = ljs.device_put(np.zeros((2, 8), dtype=np.int64))
    params = nn.unbox(model.init(ljs.random.PRNGKey(1), ids)["params"])

    def flatten(tree, path=()):
        if isinstance(tree, dict):
            for k in sorted(tree):
                yield from flatten(tree[k], path + (k,))
        else:
            yield "/".join(path), tuple(tree.shape)
    return dict(flatten(params)), model.apply({"params": params}, ids)


def test_transformer_lm_with_a_gated_feed_forward(host_devices):
    from learning_jax_sharding_amd.models import TransformerLM, TransformerLayer
    host_devices(1)
    relu, _ = _paths(LM)
    same, _ = _paths(dict(LM, ff="relu"))
    assert relu == same and relu["layer_0/ff/w_in"] == (32, 128) and "layer_0/ff/w_gate" not in relu
    gated, logits = _paths(dict(LM, ff="swiglu", causal=True, rope_theta=1e4))
    assert tuple(logits.shape) == (2, 8, 64) and torch.isfinite(logits.to_torch().float()).all()
    for i in range(2):
        assert gated[f"layer_{i}/ff/w_gate"] == gated[f"layer_{i}/ff/w_up"] == (32, 128)
        assert gated[f"layer_{i}/ff/w_out"] == (128, 32)
    assert set(gated) - set(relu) == {f"layer_{i}/ff/{w}" for i in range(2) for w in ("w_gate", "w_up")}
    assert set(relu) - set(gated) == {f"layer_{i}/ff/w_in" for i in range(2)}
    # ff_dim=None: 4 dim for relu; the multiple of 128 at or above 8 dim / 3 for swiglu
    assert TransformerLM(1024, 640, 1).default_ff_dim() == 2560
    assert TransformerLM(1024, 640, 1, ff="swiglu").default_ff_dim() == 1792
    assert TransformerLM(1024, 96, 1, ff="swiglu").default_ff_dim() == 256
    assert TransformerLM(1024, 48, 1, ff="swiglu").default_ff_dim() == 128
    assert _paths(dict(LM, ff="swiglu", ff_dim=40))[0]["layer_1/ff/w_up"] == (32, 40)
    for cls, args in ((TransformerLayer, (32,)), (TransformerLM, (64, 32, 1))):
        with pytest.raises(ValueError, match="fp8"):
            cls(*args, ff="swiglu", fp8=True)
        with pytest.raises(ValueError, match="'relu' or 'swiglu'"):
            cls(*args, ff="geglu")


def test_layer_flops_count_three_gemms_when_gated():
    from learning_jax_sharding_amd.models import attention_block_flops, transformer_layer_flops
    B, S, M, H, D, F = 4, 256, 640, 8, 64, 1792
    att_t, att_f = attention_block_flops(B, S, M, H, D, True), attention_block_flops(B, S, M, H, D, False)
    one = 2 * B * S * M * F                       # one [T, M] x [M, F] GEMM
    assert transformer_layer_flops(B, S, M, H, D, F, True) == att_t + 3 * 2 * one
    assert transformer_layer_flops(B, S, M, H, D, F, True, gated=False) == att_t + 3 * 2 * one
    assert transformer_layer_flops(B, S, M, H, D, F, True, gated=True) == att_t + 3 * 3 * one
    assert transformer_layer_flops(B, S, M, H, D, F, False, gated=True) == att_f + 3 * one
