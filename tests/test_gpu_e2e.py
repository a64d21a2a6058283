"""End-to-end on a real MI355X: the partitioned attention block through the HIP kernels
matches the host-device (torch) run, on 1 GPU and on virtual 2x2 / 2x4 meshes."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_block(mesh_shape, B=4, S=128, M=640, heads=8, dh=64, rules=None):
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd import nn
    from learning_jax_sharding_amd.mesh import Mesh, create_device_mesh
    from learning_jax_sharding_amd.models import MultiHeadAttention
    from learning_jax_sharding_amd.sharding import NamedSharding, PartitionSpec as P
    mesh = Mesh(create_device_mesh(mesh_shape), ("data", "model"))
    rules = rules or (("batch", "data"), ("embed", "model"), ("hidden", "model"))
    model = MultiHeadAttention(M, heads=heads, dim_head=dh)
    x = ljs.random.normal(ljs.random.PRNGKey(0), (B, S, M))
    params = model.init(ljs.random.PRNGKey(1), x)["params"]
    params = ljs.device_put(params, nn.logical_to_mesh_sharding(nn.get_partition_spec(params), mesh, rules))
    x = ljs.device_put(x, NamedSharding(mesh, P("data", "model")))

    def loss(p):
        return model.apply({"params": p}, x).sum()

    with mesh, nn.axis_rules(rules):
        val, g = ljs.value_and_grad(loss)(params)
    g = nn.unbox(g)
    return float(np.asarray(val)), ljs.tree_map(lambda a: np.asarray(a), g)


@pytest.mark.parametrize("mesh_shape", [(1, 1), (2, 2), (2, 4)])
def test_block_gpu_matches_host(host_devices, gpu_devices, mesh_shape):
    n = int(np.prod(mesh_shape))
    host_devices(n)
    vh, gh = _run_block(mesh_shape)
    gpu_devices(n)
    from learning_jax_sharding_amd.ops import hip
    hip.lib()
    vg, gg = _run_block(mesh_shape)
    assert abs(vh - vg) <= 3e-2 * max(1.0, abs(vh)), (vh, vg)
    for k in gh:
        for name in gh[k]:
            a, b = gh[k][name], gg[k][name]
            np.testing.assert_allclose(b, a, rtol=5e-2, atol=5e-2 * np.abs(a).max(), err_msg=f"{k}/{name}")


def test_block_gpu_case5_rules_odd_tokens(host_devices, gpu_devices):
    """case5 rules (embed -> data: Wq/Wk/Wv/Wo FSDP-sharded, gathered as bf16-shadow proxies) with
    20 local tokens per device (not a multiple of 8): the dense layers take the padded path and
    read the proxies' values from the gathered bf16 copies instead of raising."""
    rules = (("batch", "data"), ("embed", "data"), ("hidden", "model"))
    host_devices(4)
    vh, gh = _run_block((2, 2), B=4, S=20, rules=rules)
    gpu_devices(4)
    vg, gg = _run_block((2, 2), B=4, S=20, rules=rules)
    assert abs(vh - vg) <= 3e-2 * max(1.0, abs(vh)), (vh, vg)
    for k in gh:
        for name in gh[k]:
            a, b = gh[k][name], gg[k][name]
            np.testing.assert_allclose(b, a, rtol=5e-2, atol=5e-2 * np.abs(a).max(), err_msg=f"{k}/{name}")


@pytest.mark.parametrize("mesh_shape,dh", [((1, 1), 32), ((2, 2), 128)])
def test_block_gpu_other_head_dims_match_host(host_devices, gpu_devices, mesh_shape, dh):
    """head_dim other than the HIP kernels' 64 (heads x dh = 512 kept): the GPU run takes the torch
    attention formulation (with a warning) around the HIP GEMMs and matches the host run."""
    heads = 512 // dh
    n = int(np.prod(mesh_shape))
    host_devices(n)
    vh, gh = _run_block(mesh_shape, heads=heads, dh=dh)
    gpu_devices(n)
    from learning_jax_sharding_amd.ops import hip
    hip.lib()
    with pytest.warns(UserWarning, match="head_dim 64"):
        vg, gg = _run_block(mesh_shape, heads=heads, dh=dh)
    assert abs(vh - vg) <= 3e-2 * max(1.0, abs(vh)), (vh, vg)
    for k in gh:
        for name in gh[k]:
            a, b = gh[k][name], gg[k][name]
            np.testing.assert_allclose(b, a, rtol=5e-2, atol=5e-2 * np.abs(a).max(), err_msg=f"{k}/{name}")


def test_native_library_loaded(gpu_devices):
    gpu_devices(1)
    import learning_jax_sharding_amd as ljs
    x = ljs.random.normal(ljs.random.PRNGKey(0), (64, 64))
    y = ljs.lax.dot(x, x)
    torch.cuda.synchronize()
    maps = open(f"/proc/{os.getpid()}/maps").read()
    assert "libljs_kernels.so" in maps


@pytest.mark.parametrize("case", ["case1a.py", "case3_fully_sharded.py", "case6_attention.py"])
def test_cases_on_gpu(case):
    env = dict(os.environ, PYTHONPATH=ROOT, LJS_PLATFORM="gpu")
    env.pop("LJS_NUM_DEVICES", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "cases", case)], capture_output=True, text=True, env=env,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "GPU 0" in r.stdout


def test_jit_graph_train_step_matches_eager(gpu_devices):
    """Captured (hipGraph) donated train steps == eager steps; inputs passed again are read in
    place (aliased), a different input buffer triggers one private re-capture, and the
    caller's arrays are never written."""
    gpu_devices(1)
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd import optim
    from learning_jax_sharding_amd.models import MultiHeadAttention
    from learning_jax_sharding_amd.training import TrainState
    model = MultiHeadAttention(640, heads=8, dim_head=64)
    x1 = ljs.random.normal(ljs.random.PRNGKey(0), (4, 128, 640))
    x2 = ljs.random.normal(ljs.random.PRNGKey(5), (4, 128, 640))
    x1_copy = np.asarray(x1).copy()

    def make():
        params = model.init(ljs.random.PRNGKey(1), x1)["params"]
        return TrainState.create(apply_fn=model.apply, params=params, tx=optim.adam(1e-3))

    def step(state, x):
        g = ljs.grad(lambda p: model.apply({"params": p}, x).sum())(state.params)
        return state.apply_gradients(grads=g)

    eager = ljs.jit(step, capture=False)
    graph = ljs.jit(step, donate_argnums=0, capture=True)
    se, sg = make(), make()
    for x in (x1, x1, x1, x2, x2, x1):
        se = eager(se, x)
        sg = graph(sg, x)
    torch.cuda.synchronize()
    assert int(np.asarray(sg.step)) == 6 and int(np.asarray(se.step)) == 6
    np.testing.assert_array_equal(np.asarray(x1), x1_copy)
    pe, pg = ljs.tree_util.tree_leaves(se.params), ljs.tree_util.tree_leaves(sg.params)
    for a, b in zip(pe, pg):
        np.testing.assert_allclose(np.asarray(b), np.asarray(a), rtol=1e-4, atol=1e-5)


def test_jit_graph_multi_step_capture_matches_single_steps(gpu_devices):
    """bench.py --graph-steps: G complete train steps captured into one hipGraph give the same
    state as G replays of the one-step graph (same kernels, same order: bit-exact)."""
    gpu_devices(1)
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

    def steps3(state, x):
        for _ in range(3):
            state = step(state, x)
        return state

    one = ljs.jit(step, donate_argnums=0, capture=True)
    three = ljs.jit(steps3, donate_argnums=0, capture=True)
    s1, s3 = make(), make()
    for _ in range(3):  # 9 steps each: the first calls capture, later ones replay
        for _ in range(3):
            s1 = one(s1, x)
        s3 = three(s3, x)
    torch.cuda.synchronize()
    assert int(np.asarray(s1.step)) == 9 and int(np.asarray(s3.step)) == 9
    for a, b in zip(ljs.tree_util.tree_leaves(s1), ljs.tree_util.tree_leaves(s3)):
        np.testing.assert_array_equal(np.asarray(b), np.asarray(a))


def test_jit_graph_multi_step_reads_step_between_steps(gpu_devices):
    """Inside a G-step graph the Adam count increments are deferred to one launch per graph
    (ops/hip._defer_step_inc); a step that READS ``state.step`` (an RNG fold, an LR schedule) must
    still see the count eager steps see: the read launches the pending increments first
    (optim/adam.CountLocal).  Accumulated reads are compared against eager steps."""
    gpu_devices(1)
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd import optim
    from learning_jax_sharding_amd.models import MultiHeadAttention
    from learning_jax_sharding_amd.training import TrainState
    model = MultiHeadAttention(640, heads=8, dim_head=64)
    x = ljs.random.normal(ljs.random.PRNGKey(0), (2, 128, 640))

    def make():
        params = model.init(ljs.random.PRNGKey(1), x)["params"]
        return TrainState.create(apply_fn=model.apply, params=params, tx=optim.adam(1e-3))

    def steps3(carry, x):
        state, acc = carry
        for _ in range(3):
            acc = acc + state.step.astype(torch.float32) * 10.0
            g = ljs.grad(lambda p: model.apply({"params": p}, x).sum())(state.params)
            state = state.apply_gradients(grads=g)
        return state, acc + state.step.astype(torch.float32)

    zero = ljs.numpy.asarray(np.zeros((), np.float32))
    eager = ljs.jit(steps3, donate_argnums=0, capture=False)
    graph = ljs.jit(steps3, donate_argnums=0, capture=True, warmup_calls=0)
    se, sg = (make(), zero), (make(), zero)
    for _ in range(2):   # the first graph call captures, the second replays
        se = eager(se, x)
        sg = graph(sg, x)
    torch.cuda.synchronize()
    ae, ag = (float(np.asarray(a[1]).reshape(-1)[0]) for a in (se, sg))
    # per call: 10 * (c + c+1 + c+2) + (c+3) added at c = 0, then c = 3: 33 + 126 = 159
    assert ae == 159.0, ae
    assert int(np.asarray(se[0].step)) == 6 and int(np.asarray(sg[0].step)) == 6
    assert ae == ag, (ae, ag)


def test_jit_graph_multi_step_input_cast_prefetch_bit_exact(gpu_devices, monkeypatch):
    """A multi-step graph whose steps register the next step's input (ops/linear.
    prefetch_next_input): the next cast runs in the optimizer launch's extra blocks and the next
    step's dense takes it -- the state equals single-step replays bit for bit, each step's cast
    ran, and nothing stays registered after the capture."""
    gpu_devices(1)
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd import optim
    from learning_jax_sharding_amd.models import MultiHeadAttention
    from learning_jax_sharding_amd.ops import linear as lin
    from learning_jax_sharding_amd.training import TrainState
    model = MultiHeadAttention(640, heads=8, dim_head=64)
    x = ljs.random.normal(ljs.random.PRNGKey(0), (8, 256, 640))   # 1.3 M f32: prefetched

    def make():
        params = model.init(ljs.random.PRNGKey(1), x)["params"]
        return TrainState.create(apply_fn=model.apply, params=params, tx=optim.adam(1e-3))

    def step(state, x):
        g = ljs.grad(lambda p: model.apply({"params": p}, x).sum())(state.params)
        return state.apply_gradients(grads=g)

    monkeypatch.setattr(lin, "_PRECAST_MODE", "join")
    monkeypatch.setattr(lin, "_OPT_PRECAST", "1")
    taken = []
    orig = lin._take_precast

    def spy(t):
        r = orig(t)
        taken.append(r is not None)
        return r
    lin._take_precast = spy
    try:
        def steps3(state, x):
            for i in range(3):
                if i + 1 < 3:
                    lin.prefetch_next_input(x)
                state = step(state, x)
            lin.join_precasts()
            return state

        one = ljs.jit(step, donate_argnums=0, capture=True)
        three = ljs.jit(steps3, donate_argnums=0, capture=True)
        s1, s3 = make(), make()
        for _ in range(3):
            for _ in range(3):
                s1 = one(s1, x)
            s3 = three(s3, x)
        torch.cuda.synchronize()
    finally:
        lin._take_precast = orig
    assert any(taken), "no dense took a prefetched cast"
    assert not lin._PRECAST and not lin._NEXT_INPUTS
    assert int(np.asarray(s1.step)) == 9 and int(np.asarray(s3.step)) == 9
    for a, b in zip(ljs.tree_util.tree_leaves(s1), ljs.tree_util.tree_leaves(s3)):
        np.testing.assert_array_equal(np.asarray(b), np.asarray(a))


def _run_layer(mesh_shape, fp8, B=2, S=128, M=640, ff=2560):
    import learning_jax_sharding_amd as ljs
    import learning_jax_sharding_amd.numpy as jnp
    from learning_jax_sharding_amd import nn
    from learning_jax_sharding_amd.mesh import Mesh, create_device_mesh
    from learning_jax_sharding_amd.models import TransformerLayer
    from learning_jax_sharding_amd.sharding import NamedSharding, PartitionSpec as P
    mesh = Mesh(create_device_mesh(mesh_shape), ("data", "model"))
    rules = (("batch", "data"), ("embed", "model"), ("hidden", "model"))
    model = TransformerLayer(M, ff_dim=ff, fp8=fp8)
    x = ljs.random.normal(ljs.random.PRNGKey(0), (B, S, M))
    params = model.init(ljs.random.PRNGKey(1), x)["params"]
    params = ljs.device_put(params, nn.logical_to_mesh_sharding(nn.get_partition_spec(params), mesh, rules))
    x = ljs.device_put(x, NamedSharding(mesh, P("data", "model")))

    def loss(p):
        return model.apply({"params": p}, x).astype(jnp.float32).sum()

    with mesh, nn.axis_rules(rules):
        val, g = ljs.value_and_grad(loss)(params)
    return float(np.asarray(val)), ljs.tree_map(lambda a: np.asarray(a), nn.unbox(g))


@pytest.mark.parametrize("mesh_shape", [(1, 1), (2, 2)])
def test_fp8_layer_gpu_matches_host_emulation(host_devices, gpu_devices, mesh_shape):
    """attention + MX-fp8 FF layer: HIP block-scaled MFMA path == host emulation.

    The two differ only in f32 summation order, but an e4m3 rounding (or a block's shared
    exponent, which moves all 32 of its elements) can land on the other side of a boundary: the
    gradients agree to a few % in norm (the small key-projection gradient the most) with at most
    a handful of elements (1e-4) outside 5 % + 5 % of the largest."""
    n = int(np.prod(mesh_shape))
    host_devices(n)
    vh, gh = _run_layer(mesh_shape, True)
    gpu_devices(n)
    vg, gg = _run_layer(mesh_shape, True)
    assert abs(vh - vg) <= 3e-2 * max(1.0, abs(vh)), (vh, vg)
    for path in gh:
        for k in gh[path]:
            a, b = gh[path][k], gg[path][k]
            pairs = [(a[n_], b[n_], n_) for n_ in a] if isinstance(a, dict) else [(a, b, "")]
            for x_, y_, n_ in pairs:
                x_, y_ = np.asarray(x_, np.float64), np.asarray(y_, np.float64)
                rel = np.linalg.norm(y_ - x_) / max(np.linalg.norm(x_), 1e-12)
                off = np.mean(np.abs(y_ - x_) > 5e-2 * np.abs(x_) + 5e-2 * np.abs(x_).max())
                assert rel < 5e-2 and off < 1e-4, (f"{path}/{k}/{n_}", rel, off)


@pytest.mark.parametrize("causal", [False, True])
def test_ring_attention_gpu_matches_allgather(gpu_devices, causal):
    """Ring attention on the HIP flash kernels (per-block lse, global-lse backward) == the
    all-gather-KV plan, on a 1x4 virtual mesh over one MI355X."""
    gpu_devices(4)
    import learning_jax_sharding_amd as ljs
    import learning_jax_sharding_amd.numpy as jnp
    from learning_jax_sharding_amd.array import ShardedArray
    from learning_jax_sharding_amd.mesh import Mesh, create_device_mesh
    from learning_jax_sharding_amd.parallel import sequence as SQ
    from learning_jax_sharding_amd.sharding import NamedSharding, PartitionSpec as P
    from learning_jax_sharding_amd.spmd.api import _fresh_leaf
    mesh = Mesh(create_device_mesh((1, 4)), ("data", "model"))
    g = torch.Generator().manual_seed(0)
    arrs = [torch.randn(2, 256, 4, 64, generator=g).bfloat16() for _ in range(3)]
    cot = torch.randn(2, 256, 4, 64, generator=g)
    sh = NamedSharding(mesh, P("data", "model"))
    res = {}
    for mode in ("allgather", "ring", "ulysses"):
        leaves = [_fresh_leaf(ljs.device_put(a, sh)) for a in arrs]
        out = SQ.context_parallel_attention(*leaves, causal=causal, mode=mode)
        loss = (out.astype(jnp.float32) * ljs.device_put(cot, sh)).sum()
        ins = [t for l in leaves for t in l.local.values()]
        outs = list(loss.local.values())
        gs = torch.autograd.grad(outs, ins, [torch.full_like(t, 1.0 / len(outs)) for t in outs])
        n_loc = len(leaves[0].local)
        glob = []
        for ai, leaf in enumerate(leaves):
            loc = {d: gs[ai * n_loc + i].float() for i, d in enumerate(leaf.local)}
            glob.append(np.asarray(ShardedArray(leaf.shape, torch.float32, leaf.sharding, loc)))
        res[mode] = (np.asarray(out.astype(jnp.float32)), glob)
    for mode in ("ring", "ulysses"):
        np.testing.assert_allclose(res[mode][0], res["allgather"][0], rtol=2e-2, atol=2e-2)
        for a, b in zip(res[mode][1], res["allgather"][1]):
            np.testing.assert_allclose(a, b, rtol=3e-2, atol=3e-2 * max(1.0, np.abs(b).max()))


def test_captured_value_and_grad_fresh_every_replay(gpu_devices):
    """A captured jit of value_and_grad returns THIS call's loss and gradients on every replay
    (lazy outputs - the unread loss, uncombined weight-gradient slabs - are forced inside the
    capture, not in an eager thunk cached after the first replay)."""
    gpu_devices(1)
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd.models import MultiHeadAttention
    model = MultiHeadAttention(640, heads=8, dim_head=64)
    xs = [ljs.random.normal(ljs.random.PRNGKey(10 + i), (2, 128, 640)) for i in range(3)]
    params = model.init(ljs.random.PRNGKey(1), xs[0])["params"]

    def vg(p, x):
        return ljs.value_and_grad(lambda q: model.apply({"params": q}, x).sum())(p)

    eager = ljs.jit(vg, capture=False)
    graph = ljs.jit(vg, capture=True)
    for x in xs + xs[::-1]:
        ve, ge = eager(params, x)
        vgr, gg = graph(params, x)
        torch.cuda.synchronize()
        v_e, v_g = float(np.asarray(ve)), float(np.asarray(vgr))
        assert abs(v_e - v_g) <= 1e-3 * max(1.0, abs(v_e)), (v_e, v_g)
        for a, b in zip(ljs.tree_util.tree_leaves(ge), ljs.tree_util.tree_leaves(gg)):
            a, b = np.asarray(a), np.asarray(b)
            np.testing.assert_allclose(b, a, rtol=1e-3, atol=1e-3 * np.abs(a).max())


def test_grad_wrt_detached_relu_output_is_not_premasked(gpu_devices):
    """d/dh of dense(h) where h is a .detach()ed ReLU-dense output: no ReLU mask may be applied
    (the premask is keyed on the autograd edge, not on the storage)."""
    gpu_devices(1)
    from learning_jax_sharding_amd.ops import hip
    torch.manual_seed(0)
    x = torch.randn(256, 128, device="cuda").bfloat16()
    w1 = torch.randn(128, 256, device="cuda") * 0.1
    w2 = torch.randn(256, 128, device="cuda") * 0.1
    h = hip.linear(x, [w1], None, torch.bfloat16, True, torch.bfloat16)[0]
    hd = h.detach().requires_grad_(True)
    y = hip.linear(hd, [w2], None, torch.bfloat16, False, torch.bfloat16)[0]
    dy = torch.randn_like(y)
    (g,) = torch.autograd.grad(y, hd, dy)
    ref = (dy.float() @ w2.bfloat16().float().t())
    assert (h == 0).any()
    zero = (h == 0)
    # where h == 0 the true gradient is generally non-zero; a wrongly applied mask zeroes it
    assert g.float()[zero].abs().max() > 0
    np.testing.assert_allclose(g.float().cpu().numpy(), ref.cpu().numpy(), rtol=5e-2, atol=5e-2)


def test_mse_loss_kernel_matches_torch(gpu_devices):
    """HIP fused MSE (value + dY in one pass) vs the f32 torch oracle, f32 and bf16 targets,
    with a length that is not a multiple of 8 (scalar tail)."""
    gpu_devices(1)
    from learning_jax_sharding_amd.ops import hip
    for n, tdt in ((1 << 20, torch.float32), (1000003, torch.bfloat16)):
        y = torch.randn(n, device="cuda").bfloat16().requires_grad_(True)
        t = torch.randn(n, device="cuda").to(tdt)
        scale = 1.0 / n
        with hip.launch_log() as log:
            loss = hip.mse_loss(y, t, scale)
        want = "mse<tf32,dy>" if tdt == torch.float32 else "mse<tbf16,dy>"
        assert [r["name"] for r in log if r["name"].startswith("mse")] == [want], list(log)   # the kernel, not the fallback
        (gy,) = torch.autograd.grad(loss, y, torch.tensor(1.0, device="cuda"))
        yf = y.detach().float()
        ref = ((yf - t.float()) ** 2).sum() * scale
        assert abs(float(loss) - float(ref)) <= 1e-4 * float(ref)
        ref_g = (2 * scale * (yf - t.float()))
        np.testing.assert_allclose(gy.float().cpu().numpy(), ref_g.cpu().numpy(), rtol=1e-2, atol=1e-9)


def test_mse_colsum_kernel_and_bias_grad(gpu_devices):
    """The fused MSE (value + dY + dY's column sums in one pass) under a dense layer with a bias:
    value, input gradient and bias gradient vs the f32 torch oracle; also for a seq-major
    prediction (y stored [seq][batch][features])."""
    gpu_devices(1)
    from learning_jax_sharding_amd.ops import hip
    torch.manual_seed(0)
    for seq_major in (False, True):
        x = torch.randn(8, 128, 256, device="cuda")
        w = (torch.randn(256, 640, device="cuda") * 0.05).requires_grad_(True)
        b = (torch.randn(640, device="cuda") * 0.1).requires_grad_(True)
        t = torch.randn(8, 128, 640, device="cuda")
        xin = x.transpose(0, 1).contiguous().transpose(0, 1) if seq_major else x
        y = hip.linear(xin, [w], b, torch.bfloat16, False, torch.bfloat16)[0]
        loss = hip.mse_loss(y, t, 1.0 / y.numel())
        gw, gb = torch.autograd.grad(loss, (w, b), torch.tensor(1.0, device="cuda"))
        yr = y.detach().float()
        ref_loss = ((yr - t) ** 2).mean()
        dy = (2.0 / y.numel()) * (yr - t)
        ref_gb = dy.to(torch.bfloat16).float().sum((0, 1))
        ref_gw = x.reshape(-1, 256).bfloat16().float().t() @ dy.to(torch.bfloat16).float().reshape(-1, 640)
        assert abs(float(loss) - float(ref_loss)) <= 1e-4 * float(ref_loss)
        np.testing.assert_allclose(gb.cpu().numpy(), ref_gb.cpu().numpy(), rtol=2e-3, atol=1e-7)
        np.testing.assert_allclose(gw.cpu().numpy(), ref_gw.cpu().numpy(), rtol=2e-2,
                                   atol=2e-2 * float(ref_gw.abs().max()))


def _run_fsdp_stack(n, B=8, S=128, M=256, layers=3):
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd import nn
    from learning_jax_sharding_amd.mesh import Mesh, create_device_mesh
    from learning_jax_sharding_amd.models import DenseStack
    from learning_jax_sharding_amd.parallel import fsdp
    from learning_jax_sharding_amd.sharding import NamedSharding, PartitionSpec as P
    mesh = Mesh(create_device_mesh((n, 1)), ("data", "model"))
    model = DenseStack(M, layers=layers)
    x = ljs.random.normal(ljs.random.PRNGKey(0), (B, S, M))
    params = model.init(ljs.random.PRNGKey(1), x)["params"]
    params = ljs.device_put(params, fsdp.fsdp_shardings(params, mesh, "data"))
    x = ljs.device_put(x, NamedSharding(mesh, P("data")))

    def loss(p):
        return model.apply({"params": p}, x).sum()

    with mesh:
        val, g = ljs.value_and_grad(loss)(params)
    g = nn.unbox(g)
    return float(np.asarray(val)), ljs.tree_map(lambda a: np.asarray(a), g)


def test_fsdp_stack_virtual_devices_matches_host(host_devices, gpu_devices):
    """FSDP dense stack on 4 virtual devices of one GPU (bf16 shadow gathers shared by the
    devices, weight gradients reduce-scattered straight from every device's split-K slabs) ==
    the host-device run."""
    host_devices(4)
    vh, gh = _run_fsdp_stack(4)
    gpu_devices(4)
    from learning_jax_sharding_amd.parallel import weight_gather as wg
    n0 = wg.STATS["slab_sum"]
    vg, gg = _run_fsdp_stack(4)
    assert wg.STATS["slab_sum"] > n0, wg.STATS          # the one-pass slab reduce-scatter ran
    assert abs(vh - vg) <= 3e-2 * max(1.0, abs(vh)), (vh, vg)
    for k in gh:
        for name in gh[k]:
            a, b = gh[k][name], gg[k][name]
            np.testing.assert_allclose(b, a, rtol=5e-2, atol=5e-2 * np.abs(a).max(), err_msg=f"{k}/{name}")


def test_block_gpu_local_first_kv_gather(host_devices, gpu_devices, monkeypatch):
    """2x2 virtual mesh with the local-first all-gather attention forced (own K/V block first on
    the compute stream while the gathers run on a side stream, in-kernel LSE merges) == host."""
    host_devices(4)
    vh, gh = _run_block((2, 2))
    gpu_devices(4)
    from learning_jax_sharding_amd.ops import core
    monkeypatch.setattr(core, "_KV_LOCAL_FIRST", "1")
    vg, gg = _run_block((2, 2))
    assert abs(vh - vg) <= 3e-2 * max(1.0, abs(vh)), (vh, vg)
    for k in gh:
        for name in gh[k]:
            a, b = gh[k][name], gg[k][name]
            np.testing.assert_allclose(b, a, rtol=5e-2, atol=5e-2 * np.abs(a).max(), err_msg=f"{k}/{name}")


def _ff_fp8_run(mesh_shape, B=4, S=128, M=640, F=1280):
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd import nn
    from learning_jax_sharding_amd.mesh import Mesh, create_device_mesh
    from learning_jax_sharding_amd.sharding import NamedSharding, PartitionSpec as P
    from learning_jax_sharding_amd.spmd import plan as _plan
    rules = (("batch", "data"), ("embed", "model"), ("hidden", "model"))   # case6_attention.py:183-187
    mesh = Mesh(create_device_mesh(mesh_shape), ("data", "model"))
    model = nn.FeedForward(F, fp8=True)
    x = ljs.random.normal(ljs.random.PRNGKey(0), (B, S, M))
    params = model.init(ljs.random.PRNGKey(1), x)["params"]
    params = ljs.device_put(params, nn.logical_to_mesh_sharding(nn.get_partition_spec(params), mesh, rules))
    x = ljs.device_put(x, NamedSharding(mesh, P("data", "model")))

    def loss(p):
        y = model.apply({"params": p}, x, residual=x)
        return (y.astype(ljs.numpy.float32) * y.astype(ljs.numpy.float32)).sum()

    with mesh, nn.axis_rules(rules), _plan.record_plan() as rec:
        val, g = ljs.value_and_grad(loss)(params)
    notes = [st.info.get("note", "") for st in rec.steps]
    return float(np.asarray(val)), ljs.tree_map(lambda a: np.asarray(a), nn.unbox(g)), notes


def test_fp8_ff_block_2d_gathers_mx_shadows(gpu_devices):
    """Reference rules on a 2x2 virtual mesh shard both FF weights along M over 'model': the
    fused MX-fp8 block gathers the shards' MX-fp8 shadows (64-aligned shards hold whole MX
    blocks, so the gathered codes are the full weight's quantization) instead of the f32
    weights; loss and gradients match the 1x1 run."""
    gpu_devices(1)
    v1, g1, _ = _ff_fp8_run((1, 1))
    gpu_devices(4)
    v4, g4, notes = _ff_fp8_run((2, 2))
    assert sum("mx_shadows" in n for n in notes) == 2, notes
    assert abs(v1 - v4) <= 2e-2 * max(1.0, abs(v1)), (v1, v4)
    for k in g1:
        a, b = np.asarray(g1[k], np.float64), np.asarray(g4[k], np.float64)
        rel = np.linalg.norm(b - a) / max(np.linalg.norm(a), 1e-12)
        assert rel < 3e-2, (k, rel)


def test_fused_qkv_attention_matches_unfused(gpu_devices, monkeypatch):
    """The attention block with the attention forward fused into the Q/K/V projection kernel
    (ops/linear.attention_next -> hip.qkv_attn_fwd) gives the loss and gradients of the separate
    projection + attention kernels (up to the f32 rounding differences of the two forward kernels'
    softmax state: see test_qkv_attn_fwd_bit_exact), and the fused result is what the attention op
    used."""
    from learning_jax_sharding_amd.ops import hip as H
    from learning_jax_sharding_amd.ops import linear as L
    res = {}
    monkeypatch.setattr(L, "_cu_count", lambda dev: 1)   # (4 x 8 items: below the gate of one item per two CUs)
    for on in (False, True):
        monkeypatch.setattr(L, "_QKV_ATTN", on)
        before = H.FUSED_ATTN_STATS["taken"]
        res[on] = _run_block((1, 1), B=4, S=256)
        res[(on, "taken")] = H.FUSED_ATTN_STATS["taken"] - before
    assert res[(False, "taken")] == 0 and res[(True, "taken")] >= 1
    assert abs(res[True][0] - res[False][0]) <= 1e-4 * abs(res[False][0])
    fa, fb = res[True][1], res[False][1]
    from learning_jax_sharding_amd.tree_util import tree_leaves
    for a, b in zip(tree_leaves(fa), tree_leaves(fb)):
        assert np.abs(a - b).max() <= 1e-2 * np.abs(b).max()
