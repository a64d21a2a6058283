"""End-to-end on a real MI355X: clipped, scheduled AdamW steps of a small causal RoPE / RMSNorm /
SwiGLU TransformerLM -- against host devices, eager against captured (one- and multi-step graphs),
the launches one step makes, and a virtual 2 x 2 mesh against one device."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LM = dict(vocab_size=512, dim=128, layers=2, heads=2, dim_head=64, causal=True, rope_theta=10000.0, norm="rms",
          ff="swiglu")
BATCH, SEQ = 2, 64
RULES = (("batch", "data"), ("embed", "model"), ("hidden", "model"))
# AdamW's eps.  With the default 1e-8 the update m / (sqrt(v) + eps) does not depend on the
# gradients' scale at all, so a wrong clipping scale would go unseen, and an element whose gradient
# is rounding noise takes a step of +-lr whichever way the noise points (tests/test_distributed_gloo.py
# _adam_close), which no tolerance relative to the parameter covers.  At 1e-3, the size of a typical
# clipped gradient element here (norm ~1 over ~5e5 parameters), the update of a small gradient is
# ~lr g / eps: proportional to the clipped gradient, and moved by rounding noise only in proportion.
EPS = 1e-3


def _setup(mesh_shape, max_norm, clip=True):
    """(mesh, step function, fresh-state factory, ids, labels) of the clipped LM step."""
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd import nn, optim
    from learning_jax_sharding_amd.mesh import Mesh, create_device_mesh
    from learning_jax_sharding_amd.models import TransformerLM, lm_loss
    from learning_jax_sharding_amd.sharding import NamedSharding, PartitionSpec as P
    from learning_jax_sharding_amd.training import TrainState
    mesh = Mesh(create_device_mesh(mesh_shape), ("data", "model"))
    model = TransformerLM(**LM)
    gen = torch.Generator().manual_seed(3)
    tok = torch.randint(0, LM["vocab_size"], (BATCH, SEQ), generator=gen)
    lab = torch.randint(0, LM["vocab_size"], (BATCH, SEQ), generator=gen)
    adamw = optim.adamw(optim.warmup_cosine_decay_schedule(1e-4, 1e-2, 2, 10, 1e-3), eps=EPS, weight_decay=1e-2)
    tx = optim.chain(optim.clip_by_global_norm(max_norm), adamw) if clip else adamw
    with mesh, nn.axis_rules(RULES):
        ids = ljs.device_put(tok.numpy(), NamedSharding(mesh, P("data")))
        labels = ljs.device_put(lab.numpy(), NamedSharding(mesh, P("data")))

    def make():
        with mesh, nn.axis_rules(RULES):
            params = model.init(ljs.random.PRNGKey(1), ids)["params"]
        params = ljs.device_put(params, nn.logical_to_mesh_sharding(nn.get_partition_spec(params), mesh, RULES))
        return TrainState.create(apply_fn=model.apply, params=params, tx=tx)

    def step(state, ids, labels):
        g = ljs.grad(lambda p: lm_loss(model, p, ids, labels))(state.params)
        return state.apply_gradients(grads=g)

    return mesh, step, make, ids, labels, model


def _leaves(state):
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd import nn
    return [np.asarray(a) for a in ljs.tree_util.tree_leaves(nn.unbox(state.params))]


def _norms_and_params(mesh_shape, max_norm, nsteps, on_gpu):
    """Eager steps: ([the gradients' global norm before each step], params after the last, the
    step_hyper records after each step on the GPU)."""
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd import nn, optim
    from learning_jax_sharding_amd.models import lm_loss
    from learning_jax_sharding_amd.optim.adam import last_step_hyper
    mesh, step, make, ids, labels, model = _setup(mesh_shape, max_norm)
    state, norms, recs = make(), [], []
    with mesh, nn.axis_rules(RULES):
        for _ in range(nsteps):
            g = ljs.grad(lambda p: lm_loss(model, p, ids, labels))(state.params)
            norms.append(float(np.asarray(optim.global_norm(g))))
            state = step(state, ids, labels)
            if on_gpu:
                recs.append({d: r.cpu().clone() for d, r in last_step_hyper().items()})
    return norms, _leaves(state), recs


_HOST = {}


def _host_run(host_devices, nsteps):
    """The host run, shared: the first gradient's norm gives max_norm (half of it), so that the
    clip is active from the start; returns (max_norm, norms, params)."""
    if nsteps not in _HOST:
        host_devices(1)
        n0, _, _ = _norms_and_params((1, 1), 1e30, 1, False)
        max_norm = 0.5 * n0[0]
        norms, params, _ = _norms_and_params((1, 1), max_norm, nsteps, False)
        _HOST[nsteps] = (max_norm, norms, params)
    return _HOST[nsteps]


def _close(got, want, what):
    # tests/test_gpu_e2e.py's tolerances
    for i, (b, a) in enumerate(zip(got, want)):
        np.testing.assert_allclose(b, a, rtol=5e-2, atol=5e-2 * np.abs(a).max(), err_msg=f"{what} leaf {i}")


def test_three_clipped_steps_match_host(host_devices, gpu_devices):
    max_norm, hnorms, hparams = _host_run(host_devices, 3)
    assert hnorms[1] > max_norm, (hnorms, max_norm)              # clipping is active on step 1
    gpu_devices(1)
    gnorms, gparams, recs = _norms_and_params((1, 1), max_norm, 3, True)
    print(f"clip-e2e max_norm={max_norm:.5g} host norms={hnorms} gpu norms={gnorms} "
          f"records={[r[0].tolist() for r in recs]}")
    assert len(recs) == 3 and all(len(r) == 1 for r in recs)
    sc1, lr1, n1 = (recs[1][0][i].item() for i in range(3))
    assert sc1 < 1.0 and abs(n1 - hnorms[1]) <= 5e-2 * hnorms[1]
    assert abs(sc1 - max_norm / n1) <= 2.0 ** -22 * sc1
    _close(gparams, hparams, "gpu vs host")


def test_eager_equals_captured_one_and_multi_step_graphs(gpu_devices):
    """Donated eager steps == jit(capture=True) steps == a 3-step graph (the count's increments
    deferred to one launch per graph, the schedule reading the pending offset), bit for bit."""
    gpu_devices(1)
    import learning_jax_sharding_amd as ljs
    mesh, step, make, ids, labels, _ = _setup((1, 1), 0.5)

    def steps3(state, ids, labels):
        for _ in range(3):
            state = step(state, ids, labels)
        return state

    eager = ljs.jit(step, donate_argnums=0, capture=False)
    one = ljs.jit(step, donate_argnums=0, capture=True)
    three = ljs.jit(steps3, donate_argnums=0, capture=True)
    se, s1, s3 = make(), make(), make()
    for _ in range(2):      # 6 steps each: the first calls warm up and capture, later ones replay
        for _ in range(3):
            se = eager(se, ids, labels)
            s1 = one(s1, ids, labels)
        s3 = three(s3, ids, labels)
    torch.cuda.synchronize()
    assert [int(np.asarray(s.step)) for s in (se, s1, s3)] == [6, 6, 6]
    for what, s in (("one-step graph", s1), ("three-step graph", s3)):
        for i, (a, b) in enumerate(zip(ljs.tree_util.tree_leaves(se), ljs.tree_util.tree_leaves(s))):
            np.testing.assert_array_equal(np.asarray(b), np.asarray(a), err_msg=f"{what} leaf {i}")


def test_one_step_launches_and_no_forced_combine(gpu_devices):
    """One clipped step issues grad_sumsq, step_hyper and the dynamic Adam instance; the optimizer
    reads the deferred weight gradients as slabs and launches no slab_reduce of its own (the
    backward's combines of the gradients it does not defer are not the optimizer's)."""
    gpu_devices(1)
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd import nn
    from learning_jax_sharding_amd.models import lm_loss
    from learning_jax_sharding_amd.ops import hip
    L = hip.lib()
    seen = {}
    for clip in (False, True):
        mesh, _, make, ids, labels, model = _setup((1, 1), 0.5, clip=clip)
        state = make()
        n_reduce, forms = [0], []
        saved_reduce, saved_sumsq = L.ljs_slab_reduce, hip.grad_sumsq

        def reduce_watched(*a):
            n_reduce[0] += 1
            return saved_reduce(*a)

        def sumsq_watched(sources, device):
            forms.extend(type(g).__name__ for _, g in sources)
            return saved_sumsq(sources, device)

        L.ljs_slab_reduce, hip.grad_sumsq = reduce_watched, sumsq_watched
        try:
            with mesh, nn.axis_rules(RULES):
                g = ljs.grad(lambda p: lm_loss(model, p, ids, labels))(state.params)
                in_backward = n_reduce[0]
                with hip.launch_log() as log:
                    state = state.apply_gradients(grads=g)
        finally:
            L.ljs_slab_reduce, hip.grad_sumsq = saved_reduce, saved_sumsq
        torch.cuda.synchronize()
        seen[clip] = (n_reduce[0] - in_backward, forms, [r["name"] for r in log])
    (r0, _, names0), (r1, forms, names1) = seen[False], seen[True]
    print(f"clip-e2e optimizer launches clipped={names1} unclipped={names0} sources={sorted(set(forms))}")
    assert names1.count("grad_sumsq") == 1 and names1.count("step_hyper") == 1
    dyn = [i for i, n in enumerate(names1) if n.startswith("adam_multi_dyn<")]
    assert len(dyn) == 1 and names1.index("grad_sumsq") < names1.index("step_hyper") < dyn[0]
    assert "grad_sumsq" not in names0 and names0.count("step_hyper") == 1     # the schedule alone: no norm pass
    assert not [n for n in names1 if "slab_reduce" in n]
    assert "SlabGrad" in forms                # deferred gradients were read where they lie
    assert r0 == 0 and r1 == 0, (r0, r1)      # and neither the norm nor Adam combined one


def test_virtual_2x2_mesh_matches_one_device(host_devices, gpu_devices):
    """hidden and embed sharded over a virtual 2 x 2 mesh: the parameters after two steps match the
    one-device run, and every device's record holds the same norm bits."""
    max_norm, _, _ = _host_run(host_devices, 3)
    gpu_devices(1)
    _, p1, _ = _norms_and_params((1, 1), max_norm, 2, True)
    gpu_devices(4)
    _, p4, recs = _norms_and_params((2, 2), max_norm, 2, True)
    assert all(len(r) == 4 for r in recs)
    for r in recs:
        bits = [r[d].view(torch.int32)[2].item() for d in sorted(r)]
        assert len(set(bits)) == 1 and r[0][2].item() > 0, bits
        assert len({r[d].view(torch.int32)[0].item() for d in r}) == 1
    _close(p4, p1, "2x2 vs 1x1")
