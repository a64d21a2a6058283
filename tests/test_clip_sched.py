"""Learning-rate schedules, global_norm / clip_by_global_norm and the fused chain's contract on
host devices, against the float64 oracles of tests/clip_oracle.py."""
import math
import os
import pickle
import tempfile

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import clip_oracle as CO

WARMUP, DECAY = 5, 20
COUNTS = (0, 1, WARMUP - 1, WARMUP, WARMUP + 1, DECAY - 1, DECAY, DECAY + 17)


def _schedules():
    """(name, schedule object, float64 oracle) of every schedule form the checks use."""
    from learning_jax_sharding_amd import optim
    return [
        ("constant", optim.constant_schedule(3e-4), lambda c: 3e-4),
        ("linear", optim.linear_schedule(1e-3, 1e-5, DECAY), lambda c: CO.linear(1e-3, 1e-5, DECAY, 0, c)),
        ("linear_begin", optim.linear_schedule(2e-3, 1e-4, DECAY - WARMUP, transition_begin=WARMUP),
         lambda c: CO.linear(2e-3, 1e-4, DECAY - WARMUP, WARMUP, c)),
        ("linear_steps0", optim.linear_schedule(1e-3, 1e-5, 0), lambda c: CO.linear(1e-3, 1e-5, 0, 0, c)),
        ("cosine", optim.cosine_decay_schedule(1e-3, DECAY, alpha=0.1), lambda c: CO.cosine(1e-3, DECAY, 0.1, c)),
        ("warmup_cosine", optim.warmup_cosine_decay_schedule(1e-5, 1e-3, WARMUP, DECAY, end_value=1e-4),
         lambda c: CO.warmup_cosine(1e-5, 1e-3, WARMUP, DECAY, 1e-4, c)),
    ]


def test_schedules_match_float64_formulas():
    worst = 0.0
    for name, s, want in _schedules():
        for c in COUNTS:
            got = s(c)
            assert isinstance(got, float), name
            u = CO.ulps64(got, want(c))
            worst = max(worst, u)
            assert u <= 1.0, (name, c, got, want(c))
    print(f"clip-figures schedules worst_ulps_f64={worst}")
    s = dict((n, o) for n, o, _ in _schedules())
    assert s["linear_steps0"](7) == 1e-3                      # transition_steps = 0: init
    assert s["linear_begin"](WARMUP) == 2e-3 and s["linear_begin"](0) == 2e-3
    assert s["warmup_cosine"](WARMUP) == 1e-3 and math.isclose(s["warmup_cosine"](0), 1e-5, rel_tol=1e-14)
    assert math.isclose(s["warmup_cosine"](DECAY + 17), 1e-4, rel_tol=1e-15)


def test_schedule_torch_value_matches_host():
    """The on-device form used by host devices (a count tensor, no .item()): f32(schedule(count))
    within 1 f32 ulp."""
    for name, s, _ in _schedules():
        for c in COUNTS:
            got = s.torch_value(torch.tensor(c, dtype=torch.int32))
            assert got.dtype == torch.float32 and got.dim() == 0
            assert CO.ulps32(got.item(), s(c)) <= 1.0, (name, c)


def test_schedule_hashing():
    from learning_jax_sharding_amd import optim
    a = optim.warmup_cosine_decay_schedule(0.0, 1e-3, 5, 20, 1e-5)
    b = optim.warmup_cosine_decay_schedule(0.0, 1e-3, 5, 20, 1e-5)
    c = optim.warmup_cosine_decay_schedule(0.0, 1e-3, 6, 20, 1e-5)
    assert a == b and hash(a) == hash(b) and a != c and hash(a) != hash(c)
    assert optim.constant_schedule(1e-3) != optim.cosine_decay_schedule(1e-3, 10)
    with pytest.raises(AttributeError):
        a.kind = 1
    assert hash(optim.adam(a)) == hash(optim.adam(b)) and optim.adam(a) == optim.adam(b)
    assert hash(optim.adam(optim.constant_schedule(1e-3))) != hash(optim.adam(1e-3))
    assert optim.adam(optim.constant_schedule(1e-3)) != optim.adam(1e-3)
    t1 = optim.chain(optim.clip_by_global_norm(1.0), optim.adamw(a))
    t2 = optim.chain(optim.clip_by_global_norm(1.0), optim.adamw(b))
    t3 = optim.chain(optim.clip_by_global_norm(2.0), optim.adamw(b))
    assert t1 == t2 and hash(t1) == hash(t2) and t1 != t3
    with pytest.raises(ValueError):
        optim.cosine_decay_schedule(1e-3, 0)
    with pytest.raises(ValueError):
        optim.clip_by_global_norm(0.0)


def _tree(gen, scale=1.0):
    return {"a": scale * torch.randn(33, 65, generator=gen), "b": {"c": scale * torch.randn(7, generator=gen),
                                                                  "d": scale * torch.randn(64, 64, generator=gen)}}


def _leaves(tree):
    return [tree["a"], tree["b"]["c"], tree["b"]["d"]]


def _put(ljs, tree):
    return ljs.device_put({"a": tree["a"].numpy(), "b": {k: v.numpy() for k, v in tree["b"].items()}})


def test_global_norm_host(host_devices):
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd import optim
    host_devices(1)
    tree = _tree(torch.Generator().manual_seed(3))
    n = optim.global_norm(_put(ljs, tree))
    assert n.shape == () and n.dtype == torch.float32 and n.is_fully_replicated
    want = CO.norm64(_leaves(tree))
    allowed = CO.host_allowed(want, CO.norm32(_leaves(tree)))
    err = abs(float(np.asarray(n)) - want)
    print(f"clip-figures global_norm err={err:.3e} allowed={allowed:.3e}")
    assert err <= allowed


@pytest.mark.parametrize("case", ["active", "inactive", "zero", "equal"])
def test_clip_by_global_norm_host(host_devices, case):
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd import optim
    host_devices(1)
    tree = _tree(torch.Generator().manual_seed(4))
    if case == "zero":
        tree = {"a": torch.zeros(33, 65), "b": {"c": torch.zeros(7), "d": torch.zeros(64, 64)}}
    if case == "equal":
        # norm == max_norm exactly (3-4-12-84 -> 85): the `<` test takes the max_norm / norm branch, = 1
        tree = {"a": torch.zeros(33, 65), "b": {"c": torch.tensor([3.0, 4, 12, 84, 0, 0, 0]), "d": torch.zeros(64, 64)}}
        assert CO.norm64(_leaves(tree)) == 85.0
    norm = CO.norm64(_leaves(tree))
    max_norm = {"active": 0.37 * norm, "inactive": 1.5 * norm, "zero": 1.0, "equal": 85.0}[case]
    tx = optim.clip_by_global_norm(max_norm)
    init, update = tx
    st = init(None)
    assert st == optim.EmptyState() and isinstance(st, optim.EmptyState)
    upd, st2 = update(_put(ljs, tree), st)
    assert isinstance(st2, optim.EmptyState)
    sc = CO.scale64(norm, max_norm)
    assert (sc < 1.0) == (case == "active")
    sc32 = 1.0 if CO.norm32(_leaves(tree)) < max_norm else np.float32(max_norm) / np.float32(CO.norm32(_leaves(tree)))
    got = [upd["a"], upd["b"]["c"], upd["b"]["d"]]
    for g, t in zip(got, _leaves(tree)):
        want = t.double() * sc
        ref32 = t * torch.tensor(sc32, dtype=torch.float32)
        err = (torch.as_tensor(np.asarray(g)).double() - want).abs().max().item()
        assert err <= CO.host_allowed(want, ref32), (case, err)
        if case != "active":
            assert torch.equal(torch.as_tensor(np.asarray(g)), t)     # scale exactly 1


B1, B2, EPS, WD = 0.9, 0.999, 1e-8, 1e-2


def test_clipped_adamw_three_steps_host(host_devices):
    """chain(clip, adamw(warmup_cosine)) through TrainState.apply_gradients against the loop in
    clip_oracle.clip_adamw (float64), bounded by the same loop in f32."""
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd import optim
    from learning_jax_sharding_amd.training import TrainState
    host_devices(1)
    gen = torch.Generator().manual_seed(5)
    params = _tree(gen, 0.5)
    grads = [_tree(gen, s) for s in (3.0, 0.01, 1.0)]
    max_norm = 0.5 * CO.norm64(_leaves(grads[2]))          # active on steps 0 and 2, inactive on step 1
    sched = optim.warmup_cosine_decay_schedule(1e-4, 1e-2, 2, 10, 1e-3)
    tx = optim.chain(optim.clip_by_global_norm(max_norm), optim.adamw(sched, b1=B1, b2=B2, eps=EPS, weight_decay=WD))
    state = TrainState.create(apply_fn=None, params=_put(ljs, params), tx=tx)
    glists = [_leaves(g) for g in grads]
    want = CO.clip_adamw(_leaves(params), glists, sched, max_norm, B1, B2, EPS, WD, torch.float64)
    ref = CO.clip_adamw(_leaves(params), glists, sched, max_norm, B1, B2, EPS, WD, torch.float32)
    worst = 0.0
    for k, g in enumerate(grads):
        state = state.apply_gradients(grads=_put(ljs, g))
        got = [state.params["a"], state.params["b"]["c"], state.params["b"]["d"]]
        assert int(np.asarray(state.step)) == k + 1
        for a, w, r in zip(got, want[k], ref[k]):
            err = (torch.as_tensor(np.asarray(a)).double() - w).abs().max().item()
            allowed = CO.host_allowed(w, r)
            worst = max(worst, err / allowed)
            assert err <= allowed, (k, err, allowed)
    print(f"clip-figures clipped_adamw_host worst_fraction_of_bound={worst:.3f}")


def test_state_layout_and_step_counter(host_devices):
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd import optim
    from learning_jax_sharding_amd.training import TrainState
    host_devices(1)
    params = _put(ljs, _tree(torch.Generator().manual_seed(6)))
    tx = optim.chain(optim.clip_by_global_norm(1.0), optim.adamw(optim.constant_schedule(1e-3)))
    assert isinstance(tx, optim.GradientTransformation) and hasattr(tx, "apply")
    init, update = tx
    st = init(params)
    assert len(st) == 2 and isinstance(st[0], optim.EmptyState)
    assert isinstance(st[1], tuple) and len(st[1]) == 2
    assert isinstance(st[1][0], optim.ScaleByAdamState) and isinstance(st[1][1], optim.EmptyState)
    st2 = optim.chain(optim.clip_by_global_norm(1.0), optim.clip_by_global_norm(2.0), optim.adam(1e-3)).init(params)
    assert len(st2) == 3 and isinstance(st2[1], optim.EmptyState) and isinstance(st2[2][0], optim.ScaleByAdamState)
    state = TrainState.create(apply_fn=None, params=params, tx=tx)
    assert state.step is state.opt_state[1][0].count
    state = state.apply_gradients(grads=params)
    assert state.step is state.opt_state[1][0].count and int(np.asarray(state.step)) == 1
    # the unpacked update gives the same step as the fused apply
    upd, _ = update(params, st, params)
    np.testing.assert_array_equal(np.asarray(optim.apply_updates(params, upd)["a"]), np.asarray(state.params["a"]))
    # plain adam: unchanged
    s1 = TrainState.create(apply_fn=None, params=params, tx=optim.adam(1e-3))
    assert s1.step is s1.opt_state[0].count


def test_chain_unchanged_elsewhere():
    from learning_jax_sharding_amd import optim
    for tx in (optim.chain(optim.scale(-1.0)), optim.chain(optim.adam(1e-3)),
               optim.chain(optim.adam(1e-3), optim.clip_by_global_norm(1.0)),
               optim.chain(optim.clip_by_global_norm(1.0))):
        assert type(tx) is optim.GradientTransformation and not hasattr(tx, "apply")


def test_global_norm_sharded_counts_each_tile_once(host_devices):
    """2x2 mesh; one array replicated, one sharded on one axis (replicated on the other), one sharded
    on both: the norm of the gathered arrays, the same bits on all four devices."""
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd import optim
    from learning_jax_sharding_amd.mesh import Mesh, create_device_mesh
    from learning_jax_sharding_amd.sharding import NamedSharding, PartitionSpec as P
    host_devices(4)
    mesh = Mesh(create_device_mesh((2, 2)), ("data", "model"))
    gen = torch.Generator().manual_seed(7)
    ts = [torch.randn(6, 10, generator=gen), torch.randn(8, 12, generator=gen), torch.randn(4, 16, generator=gen)]
    specs = [P(), P("data"), P("data", "model")]
    with mesh:
        tree = [ljs.device_put(t.numpy(), NamedSharding(mesh, s)) for t, s in zip(ts, specs)]
        n = optim.global_norm({"x": tree})
        vals = [n.local[d] for d in sorted(n.local)]
        assert len(vals) == 4 and n.is_fully_replicated
        for v in vals[1:]:
            assert torch.equal(v.view(torch.int32), vals[0].view(torch.int32))
        want = CO.norm64(ts)
        assert abs(float(vals[0]) - want) <= CO.host_allowed(want, CO.norm32(ts))
        # and the clip scales every shard by the one scale
        upd, _ = optim.clip_by_global_norm(0.25 * want).update(tree, optim.EmptyState())
        for u, t in zip(upd, ts):
            w = t.double() * 0.25
            assert (torch.as_tensor(np.asarray(u)).double() - w).abs().max().item() <= CO.host_allowed(w, t * 0.25)


# ---------------------------------------------------------------------------- two ranks over gloo
def _worker(rank, world, port, out_dir):
    os.environ.update({"RANK": str(rank), "WORLD_SIZE": str(world), "LOCAL_RANK": str(rank),
                       "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "LJS_PLATFORM": "cpu"})
    os.environ.pop("LJS_NUM_DEVICES", None)
    torch.set_num_threads(1)
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd.runtime.devices import reset_backend
    reset_backend()
    ljs.initialize_distributed()
    reset_backend()
    res = _job_clipped_dp(ljs)
    with open(os.path.join(out_dir, f"r{rank}.pkl"), "wb") as f:
        pickle.dump(res, f)
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def _job_clipped_dp(ljs):
    """Two clipped, scheduled data-parallel steps of the attention layer of test_distributed_gloo."""
    from learning_jax_sharding_amd import nn, optim
    from learning_jax_sharding_amd.mesh import Mesh, create_device_mesh
    from learning_jax_sharding_amd.models import MultiHeadAttention
    from learning_jax_sharding_amd.sharding import NamedSharding, PartitionSpec as P
    from learning_jax_sharding_amd.training import TrainState
    mesh = Mesh(create_device_mesh((2, 1)), ("data", "model"))
    rules = (("batch", "data"), ("embed", "model"), ("hidden", "model"))
    model = MultiHeadAttention(64, heads=4, dim_head=16, dtype=torch.float32)
    x = ljs.random.normal(ljs.random.PRNGKey(0), (4, 32, 64))
    params = model.init(ljs.random.PRNGKey(1), x)["params"]
    params = ljs.device_put(params, nn.logical_to_mesh_sharding(nn.get_partition_spec(params), mesh, rules))
    x = ljs.device_put(x, NamedSharding(mesh, P("data", "model")))
    tx = optim.chain(optim.clip_by_global_norm(1.0), optim.adamw(optim.warmup_cosine_decay_schedule(1e-4, 1e-2, 1, 8)))
    state = TrainState.create(apply_fn=model.apply, params=params, tx=tx)
    norms = []
    with mesh, nn.axis_rules(rules):
        for _ in range(2):
            g = ljs.grad(lambda p: model.apply({"params": p}, x).sum())(state.params)
            norms.append(float(np.asarray(optim.global_norm(g))))
            state = state.apply_gradients(grads=g)
    return norms, {k: np.asarray(v["kernel"].value if hasattr(v["kernel"], "value") else v["kernel"])
                   for k, v in state.params.items()}


def test_two_ranks_clipped_steps_agree():
    world, port = 2, 29500 + (os.getpid() % 1000) + 3
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_worker, args=(world, port, d), nprocs=world, join=True)
        out = []
        for r in range(world):
            with open(os.path.join(d, f"r{r}.pkl"), "rb") as f:
                out.append(pickle.load(f))
    (n0, p0), (n1, p1) = out
    assert n0 == n1 and all(n > 1.0 for n in n0), (n0, n1)      # clipping was active on both steps
    assert p0.keys() == p1.keys() and len(p0) > 0
    for k in p0:
        np.testing.assert_array_equal(p0[k], p1[k], err_msg=k)
