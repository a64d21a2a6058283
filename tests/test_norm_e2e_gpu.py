"""End-to-end on a real MI355X: the pre-norm TransformerLayer through the fused norm kernels
matches the host-device (torch) run on one GPU and on a virtual 2x2 mesh, where the norms'
parameter gradients are sums over the devices' shards."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _run_layer(mesh_shape, norm, explicit=True, B=4, S=256, M=640, ff=1280, launches=None):
    import learning_jax_sharding_amd as ljs
    import learning_jax_sharding_amd.numpy as jnp
    from learning_jax_sharding_amd import nn
    from learning_jax_sharding_amd.mesh import Mesh, create_device_mesh
    from learning_jax_sharding_amd.models import TransformerLayer
    from learning_jax_sharding_amd.sharding import NamedSharding, PartitionSpec as P
    mesh = Mesh(create_device_mesh(mesh_shape), ("data", "model"))
    rules = (("batch", "data"), ("embed", "model"), ("hidden", "model"))
    kw = {"norm": norm} if explicit else {}
    model = TransformerLayer(M, heads=8, dim_head=64, ff_dim=ff, **kw)
    x = ljs.random.normal(ljs.random.PRNGKey(0), (B, S, M))
    params = model.init(ljs.random.PRNGKey(1), x)["params"]
    params = ljs.device_put(params, nn.logical_to_mesh_sharding(nn.get_partition_spec(params), mesh, rules))
    x = ljs.device_put(x, NamedSharding(mesh, P("data", "model")))

    def loss(p):
        return model.apply({"params": p}, x).astype(jnp.float32).sum()

    with mesh, nn.axis_rules(rules):
        if launches is not None:
            from learning_jax_sharding_amd.ops import hip
            # the ring keeps the last 32 launches: look at the forward alone, then take the step
            with hip.launch_log() as log:
                model.apply({"params": params}, x)
            launches.extend(r["name"] for r in log)
        val, g = ljs.value_and_grad(loss)(params)
    leaves = {"/".join(str(k) for k in path): np.asarray(a)
              for path, a in _flatten(ljs.tree_map(lambda a: np.asarray(a), nn.unbox(g)))}
    pl = {"/".join(str(k) for k in path): np.asarray(a) for path, a in _flatten(nn.unbox(params))}
    return float(np.asarray(val)), leaves, pl


def _flatten(tree, path=()):
    if isinstance(tree, dict):
        for k in sorted(tree):
            yield from _flatten(tree[k], path + (k,))
    else:
        yield path, tree


@pytest.mark.parametrize("mesh_shape", [(1, 1), (2, 2)])
@pytest.mark.parametrize("norm", ["layer", "rms"])
def test_prenorm_layer_gpu_matches_host(host_devices, gpu_devices, norm, mesh_shape):
    n = int(np.prod(mesh_shape))
    host_devices(n)
    vh, gh, _ = _run_layer(mesh_shape, norm)
    gpu_devices(n)
    from learning_jax_sharding_amd.ops import hip
    hip.lib()
    launches = []
    vg, gg, _ = _run_layer(mesh_shape, norm, launches=launches)
    want = {"norm1/scale", "norm2/scale"} | ({"norm1/bias", "norm2/bias"} if norm == "layer" else set())
    assert want <= set(gh) and set(gh) == set(gg)
    print(f"norm-e2e {norm} {mesh_shape} loss host={vh:.6g} gpu={vg:.6g}")
    assert abs(vh - vg) <= 3e-2 * max(1.0, abs(vh)), (vh, vg)
    for name in sorted(gh):
        a, b = gh[name], gg[name]
        print(f"norm-e2e {norm} {mesh_shape} {name} max|host|={np.abs(a).max():.4g} "
              f"max|gpu-host|={np.abs(b - a).max():.4g}")
        np.testing.assert_allclose(b, a, rtol=5e-2, atol=5e-2 * np.abs(a).max(), err_msg=name)
    # the launch ring keeps the last 32 records, so on four virtual devices only the later ones
    fwd = [s for s in launches if s.startswith("norm_fwd<")]
    assert fwd and set(fwd) <= {f"norm_fwd<{norm},f32,bf16,wave>", f"norm_fwd<{norm},bf16,bf16,wave>"}, launches
    if n == 1:
        assert fwd == [f"norm_fwd<{norm},f32,bf16,wave>", f"norm_fwd<{norm},bf16,bf16,wave>"], launches


def test_layer_without_norm_is_the_default_layer(gpu_devices):
    """norm=None on the GPU: parameters and loss equal to the layer built with the field left at
    its default, bit for bit, and no norm kernel runs."""
    gpu_devices(1)
    from learning_jax_sharding_amd.ops import hip
    hip.lib()
    launches = []
    v0, g0, p0 = _run_layer((1, 1), None, explicit=False, S=128)
    v1, g1, p1 = _run_layer((1, 1), None, explicit=True, S=128, launches=launches)
    assert set(p0) == set(p1) and not [k for k in p0 if k.startswith("norm")]
    for k in p0:
        assert np.array_equal(p0[k], p1[k]), k
    assert v0 == v1 and set(g0) == set(g1)
    assert not [s for s in launches if s.startswith("norm_")]
