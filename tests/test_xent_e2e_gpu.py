"""End-to-end on a real MI355X: one language-model train step, TransformerLayer(norm="rms") ->
Dense(1024) -> softmax cross-entropy -> mean, through the fused cross-entropy kernels matches the
same step on host devices, on one GPU and on a virtual 2x2 mesh whose model axis shards the
vocabulary (a vocab-parallel head: per-shard statistics merged over the axis)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

VOCAB = 1024


def _model(M, heads, ff):
    from learning_jax_sharding_amd import nn
    from learning_jax_sharding_amd.models import TransformerLayer
    from learning_jax_sharding_amd.nn import initializers as init
    from learning_jax_sharding_amd.nn.partitioning import with_logical_constraint, with_logical_partitioning

    class LM(nn.Module):
        def setup(self):
            self.layer = TransformerLayer(M, heads=heads, dim_head=64, ff_dim=ff, norm="rms", name="layer")
            self.head = nn.Dense(VOCAB, use_bias=False, dtype=torch.bfloat16, name="head",
                                 kernel_init=with_logical_partitioning(init.lecun_normal(), ("head_in", "vocab")))

        def __call__(self, x):
            h = with_logical_constraint(self.layer(x), ("batch", None, "head_in"))
            return with_logical_constraint(self.head(h), ("batch", None, "vocab"))

    return LM()


def _flatten(tree, path=()):
    if isinstance(tree, dict):
        for k in sorted(tree):
            yield from _flatten(tree[k], path + (k,))
    else:
        yield "/".join(path), tree


def _train_step(mesh_shape, B=4, S=128, M=640, heads=8, ff=1280, probe=None):
    """(loss, gradients, updated parameters, vocab_shards the loss ran with).  ``probe``: a list that
    receives the kernel launches of the loss alone, forward and backward, for the step's logits."""
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd import nn, optim
    from learning_jax_sharding_amd.mesh import Mesh, create_device_mesh
    from learning_jax_sharding_amd.sharding import NamedSharding, PartitionSpec as P
    from learning_jax_sharding_amd.spmd import plan as _plan
    from learning_jax_sharding_amd.training import TrainState
    mesh = Mesh(create_device_mesh(mesh_shape), ("data", "model"))
    rules = (("batch", "data"), ("embed", "model"), ("hidden", "model"), ("vocab", "model"))
    model = _model(M, heads, ff)
    x = ljs.random.normal(ljs.random.PRNGKey(0), (B, S, M))
    gen = torch.Generator().manual_seed(3)
    lab = torch.randint(0, VOCAB, (B, S), generator=gen)
    lab[0, 0], lab[0, 1], lab[1, 0], lab[1, 1], lab[2, 5] = 0, VOCAB - 1, VOCAB // 2 - 1, VOCAB // 2, -1
    with mesh, nn.axis_rules(rules):
        params = model.init(ljs.random.PRNGKey(1), x)["params"]
    params = ljs.device_put(params, nn.logical_to_mesh_sharding(nn.get_partition_spec(params), mesh, rules))
    x = ljs.device_put(x, NamedSharding(mesh, P("data", "model")))
    labels = ljs.device_put(lab.numpy(), NamedSharding(mesh, P("data")))
    state = TrainState.create(apply_fn=model.apply, params=params, tx=optim.adam(1e-2))

    def loss_fn(p):
        logits = model.apply({"params": p}, x)
        return optim.softmax_cross_entropy_with_integer_labels(logits, labels).mean()

    with mesh, nn.axis_rules(rules), _plan.record_plan() as rec:
        val, g = ljs.value_and_grad(loss_fn)(state.params)
        state = state.apply_gradients(grads=g)
        if probe is not None:
            from learning_jax_sharding_amd.ops import hip
            logits = model.apply({"params": params}, x)
            with hip.launch_log() as log:
                ljs.grad(lambda lg: optim.softmax_cross_entropy_with_integer_labels(lg, labels).mean())(logits)
            probe.extend(r["name"] for r in log)
    assert int(np.asarray(state.step)) == 1
    shards = [s.info["vocab_shards"] for s in rec.steps if s.kind == "softmax_xent"]
    grads = dict(_flatten(ljs.tree_map(lambda a: np.asarray(a), nn.unbox(g))))
    new = dict(_flatten(ljs.tree_map(lambda a: np.asarray(a), nn.unbox(state.params))))
    return float(np.asarray(val)), grads, new, shards


# The shape of the step: 16384 tokens through a narrow layer (128 wide, 2 heads, 256 hidden units).
# The token count is set by the gradient bound, not by the loss kernels.  The GPU and host forward
# passes differ by bf16 ulps, so a ReLU gate whose pre-activation lies within that difference of
# zero is open in one run and closed in the other (about one gate in a thousand), and the whole
# contribution x_token dh[token, j] of that token to column j of the w_in gradient is present in
# one run and absent in the other.  Under a sum loss every token has the same cotangent and a
# column's sum is coherent; under cross-entropy it is not: a column is a sum of N terms of random
# sign, so one token's term is about 1 / (4 sqrt(N)) of the largest entry times a product of two
# normal variates, whose tail falls like exp(-z).  5 % of the largest entry is z = 0.2 sqrt(N):
# z = 4.5 at 512 tokens (measured on one MI355X with the 640-wide layer: 461 of 819200 entries of
# w_in outside the bound, largest difference 13.6 %; the same with torch computing the loss on the
# GPU, and reproduced on the host alone by moving its attention output one bf16 ulp), 12.8 at 4096
# (3 entries, 6.0 %), 25.6 at 16384, where not one entry in 10^9 is expected outside (the host
# alone, perturbed the same way, differs by 2.5 % at most).  The layer is narrow so that the host
# step of 16384 tokens still takes two seconds.
SHAPE = dict(B=32, S=512, M=128, heads=2, ff=256)

_STEPS = {}


def _both_steps(mesh_shape, host_devices, gpu_devices):
    """The step on host devices and on the GPU for one mesh: run once, shared by the tests below."""
    if mesh_shape not in _STEPS:
        from learning_jax_sharding_amd.ops import kernels as K
        n = int(np.prod(mesh_shape))
        calls, ref = [], K.xent_stats_reference
        K.xent_stats_reference = lambda *a, **k: (calls.append(1), ref(*a, **k))[1]
        try:
            host_devices(n)
            host = _train_step(mesh_shape, **SHAPE)
            host_calls = len(calls)
            del calls[:]
            gpu_devices(n)
            from learning_jax_sharding_amd.ops import hip
            hip.lib()
            probe = []
            gpu = _train_step(mesh_shape, probe=probe, **SHAPE)
            gpu_calls = len(calls)
        finally:
            K.xent_stats_reference = ref
        _STEPS[mesh_shape] = (host, gpu, probe, host_calls, gpu_calls)
    return _STEPS[mesh_shape]


@pytest.mark.parametrize("mesh_shape", [(1, 1), (2, 2)])
def test_lm_train_step_runs_the_kernels(host_devices, gpu_devices, mesh_shape):
    """The GPU step takes xent_fwd / xent_bwd on every device and never the torch formulation (no
    [tokens, vocab] softmax is materialised by torch); on 2 x 2 the loss runs over two vocabulary
    shards; the loss and the head's gradient - the loss kernels' cotangent through one GEMM - match
    the host step within the block-parity tolerances of tests/test_gpu_e2e.py."""
    n = int(np.prod(mesh_shape))
    (vh, gh, ph, sh), (vg, gg, pg, sg), probe, host_calls, gpu_calls = _both_steps(mesh_shape, host_devices,
                                                                                   gpu_devices)
    assert host_calls and not gpu_calls
    assert set(sh) == set(sg) == {mesh_shape[1]}
    xent = [s for s in probe if s.startswith("xent_")]
    assert xent == ["xent_fwd<bf16,wave>"] * n + ["xent_bwd<bf16,wave>"] * n, probe
    print(f"xent-e2e {mesh_shape} loss host={vh:.6g} gpu={vg:.6g}")
    assert abs(vh - vg) <= 3e-2 * max(1.0, abs(vh)), (vh, vg)
    a, b = gh["head/kernel"], gg["head/kernel"]
    np.testing.assert_allclose(b, a, rtol=5e-2, atol=5e-2 * np.abs(a).max(), err_msg="head/kernel")
    for name in sorted(ph):
        assert np.isfinite(pg[name]).all(), name


@pytest.mark.parametrize("mesh_shape", [(1, 1), (2, 2)])
def test_lm_train_step_gradients_match_host(host_devices, gpu_devices, mesh_shape):
    """Every parameter gradient of the step against the host step, rtol 5e-2 and atol 5e-2 max|host|,
    the block-parity bound of tests/test_gpu_e2e.py (see SHAPE for why the step has 16384 tokens)."""
    (vh, gh, _, _), (vg, gg, _, _), _, _, _ = _both_steps(mesh_shape, host_devices, gpu_devices)
    assert set(gh) == set(gg)
    failed = []
    for name in sorted(gh):
        a, b = gh[name], gg[name]
        bad = np.abs(b - a) > 5e-2 * np.abs(a) + 5e-2 * np.abs(a).max()
        print(f"xent-e2e {mesh_shape} {name} max|host|={np.abs(a).max():.4g} max|gpu-host|={np.abs(b - a).max():.4g} "
              f"outside={int(bad.sum())}/{bad.size}")
        if bad.any():
            failed.append(name)
    assert not failed, failed
