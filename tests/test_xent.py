"""Softmax cross-entropy with integer labels (optim.softmax_cross_entropy_with_integer_labels,
ops.core.softmax_cross_entropy) on host devices: whole and vocabulary-sharded logits against
torch's F.cross_entropy in float64 on the unsharded arrays."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

B, S, V = 4, 16, 1000


def _problem():
    """Logits [4, 16, 1000] and labels [4, 16]: column 0, column V - 1, both sides of the boundary
    between two vocabulary shards (499 | 500), one ignored row, the rest random."""
    gen = torch.Generator().manual_seed(23)
    x = 2.0 * torch.randn(B, S, V, generator=gen)
    lab = torch.randint(0, V, (B, S), generator=gen)
    lab[0, 0], lab[0, 1], lab[1, 2], lab[1, 3], lab[2, 4], lab[3, 15] = 0, V - 1, V // 2 - 1, V // 2, -1, V - 1
    return x, lab


def _oracle(x, lab):
    """(loss rows, d mean(loss) / d logits) in float64; the mean runs over every row, ignored ones
    included (their loss is 0)."""
    xs = x.double().requires_grad_(True)
    loss = F.cross_entropy(xs.reshape(-1, V), lab.reshape(-1), reduction="none", ignore_index=-1).reshape(B, S)
    (g,) = torch.autograd.grad(loss.mean(), xs)
    return loss.detach().numpy(), g.numpy()


MESHES = [(1, (1, 1), ("data", None, "model"), 1), (4, (4, 1), ("data", None, None), 1),
          (4, (2, 2), ("data", None, "model"), 2)]


@pytest.mark.parametrize("n,mesh_shape,spec,vocab_shards", MESHES, ids=["1x1", "4x1-rows", "2x2-vocab"])
def test_loss_and_gradient_match_float64(host_devices, n, mesh_shape, spec, vocab_shards):
    """f32 arithmetic over 1000-term sums of order-1 values: loss rows within 1e-5, the gradient of
    the mean within 1e-5 of its largest entry.  On 2 x 2 the loss rows are replicated over the
    vocabulary axis: a cotangent counted twice (or half) over it would be off by a factor of 2."""
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd import optim
    from learning_jax_sharding_amd.mesh import Mesh, create_device_mesh
    from learning_jax_sharding_amd.sharding import NamedSharding, PartitionSpec as P
    from learning_jax_sharding_amd.spmd import plan as _plan
    host_devices(n)
    mesh = Mesh(create_device_mesh(mesh_shape), ("data", "model"))
    x, lab = _problem()
    want_loss, want_grad = _oracle(x, lab)
    logits = ljs.device_put(x.numpy(), NamedSharding(mesh, P(*spec)))
    labels = ljs.device_put(lab.numpy(), NamedSharding(mesh, P("data")))
    fn = optim.softmax_cross_entropy_with_integer_labels

    def mean_loss(lg):
        return fn(lg, labels).mean()

    with mesh, _plan.record_plan() as rec:
        loss = fn(logits, labels)
        grad = ljs.grad(mean_loss)(logits)
        abstract = ljs.eval_shape(fn, logits, labels)
        jitted = ljs.jit(fn)(logits, labels)
    assert tuple(loss.shape) == (B, S) and loss.dtype == torch.float32
    assert loss.tile.tile_shape == logits.tile.tile_shape[:-1]
    got = np.asarray(loss)
    np.testing.assert_allclose(got, want_loss, rtol=1e-5, atol=1e-5)
    assert got[2, 4] == 0.0
    assert tuple(grad.shape) == (B, S, V) and grad.sharding == logits.sharding
    g = np.asarray(grad)
    np.testing.assert_allclose(g, want_grad, rtol=1e-4, atol=1e-5 * np.abs(want_grad).max())
    assert not g[2, 4].any()
    assert [s.info["vocab_shards"] for s in rec.steps if s.kind == "softmax_xent"] == [vocab_shards] * 4
    assert tuple(abstract.shape) == (B, S) and abstract.dtype == torch.float32
    assert np.array_equal(np.asarray(jitted), got)


def test_int32_labels_and_errors(host_devices):
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd import optim
    host_devices(1)
    x, lab = _problem()
    logits = ljs.device_put(x.numpy())
    fn = optim.softmax_cross_entropy_with_integer_labels
    a = np.asarray(fn(logits, ljs.device_put(lab.numpy())))
    b = np.asarray(fn(logits, ljs.device_put(lab.numpy().astype(np.int32))))
    assert np.array_equal(a, b)
    with pytest.raises(ValueError):
        fn(logits, ljs.device_put(lab.numpy()[:, :8]))
    with pytest.raises(TypeError):
        fn(logits, ljs.device_put(lab.numpy().astype(np.float32)))
    with pytest.raises(TypeError):
        fn(logits, lab)


def test_shard_statistics_merge_to_the_whole_row():
    """The per-shard statistics of the torch formulation (the float64 oracle of the GPU tests) for
    three unequal column ranges, merged as ops.core does, give F.cross_entropy and its gradient."""
    from learning_jax_sharding_amd.ops import kernels as K
    x, lab = _problem()
    x, lab = x.double().reshape(-1, V)[:9], lab.reshape(-1)[:9]
    lab[5] = -1
    xs = x.clone().requires_grad_(True)
    parts = [(0, 300), (300, 301), (301, V)]
    st = [K.xent_stats_reference(xs[:, lo:hi], lab, lo) for lo, hi in parts]
    m = torch.stack([s[0] for s in st])
    assert not m.requires_grad
    ls, t = torch.stack([s[1] for s in st]), torch.stack([s[2] for s in st])
    own = torch.stack([(lab >= lo) & (lab < hi) for lo, hi in parts]).double()
    rel = m - m.amax(0)
    loss = torch.log((ls.exp() * rel.exp()).sum(0)) - (own * (t + rel)).sum(0)
    loss = torch.where(lab >= 0, loss, torch.zeros_like(loss))
    xr = x.clone().requires_grad_(True)
    want = F.cross_entropy(xr, lab, reduction="none", ignore_index=-1)
    w = torch.linspace(0.5, 1.5, 9, dtype=torch.float64)
    np.testing.assert_allclose(loss.detach().numpy(), want.detach().numpy(), rtol=1e-12, atol=1e-12)
    (g,), (gw,) = torch.autograd.grad(loss, xs, w), torch.autograd.grad(want, xr, w)
    np.testing.assert_allclose(g.numpy(), gw.numpy(), rtol=1e-10, atol=1e-13)
    whole = K.softmax_xent_reference(x, lab)
    np.testing.assert_allclose(whole.numpy(), want.detach().numpy(), rtol=1e-12, atol=1e-12)


def test_xent_dispatch(monkeypatch):
    """GPU tensors of f32 / bf16 logits with int32 / int64 labels take the HIP kernels; host and meta
    tensors, other dtypes and LJS_FUSED_XENT=0 take the torch formulation."""
    from learning_jax_sharding_amd.ops import kernels as K
    lab = torch.zeros(4, dtype=torch.int64)
    assert not K._hip_xent(torch.zeros(4, 7), lab)
    assert not K._hip_xent(torch.empty(4, 7, device="meta"), torch.empty(4, dtype=torch.int64, device="meta"))
    monkeypatch.setattr(K, "use_hip", lambda t: not t.is_meta)
    monkeypatch.delenv("LJS_FUSED_XENT", raising=False)
    assert K.fused_xent_enabled()
    for dt in (torch.float32, torch.bfloat16):
        for V_ in (1, 7, 50257):
            assert K._hip_xent(torch.zeros(4, V_, dtype=dt), lab)
            assert K._hip_xent(torch.zeros(4, V_, dtype=dt), lab.int())
    assert K._hip_xent(torch.zeros(2, 2, 7), torch.zeros(2, 2, dtype=torch.int64))
    assert not K._hip_xent(torch.zeros(4, 7, dtype=torch.float64), lab)
    assert not K._hip_xent(torch.zeros(4, 7, dtype=torch.float16), lab)
    assert not K._hip_xent(torch.zeros(4, 7), lab.short())
    assert not K._hip_xent(torch.zeros(4, 7), lab[:3])
    assert not K._hip_xent(torch.zeros(0, 7), lab[:0])
    monkeypatch.setenv("LJS_FUSED_XENT", "0")
    assert not K.fused_xent_enabled() and not K._hip_xent(torch.zeros(4, 7), lab)


def test_xent_instances_use_no_scratch():
    """Every instance of the two kernels (f32 / bf16 logits x int32 / int64 labels x wave / block
    mapping) is in the gfx950 code object and uses no scratch and spills nothing."""
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
    res = {n: k for n, k in kr.resources(lib).items() if "xent_fwd_kernel" in n or "xent_bwd_kernel" in n}
    assert len([n for n in res if "xent_fwd_kernel" in n]) == 8 and len(res) == 16, sorted(res)
    for n, k in res.items():
        assert k.get("scratch", 0) == 0 and k.get("vgpr_spill", 0) == 0 and k.get("sgpr_spill", 0) == 0, (n, k)
