"""The fused rotary embedding HIP kernel (csrc/kernels/rope.hip) on a real MI355X (-m gpu) against
the float64 oracle and bounds of tests/rope_oracle.py.  Every kernel case goes through the dispatcher
(ops/kernels.py rope) and asserts from the launch log that a ``rope<...>`` instance ran and that the
torch formulation was not called."""
import warnings

import numpy as np
import pytest
import torch

import rope_oracle as O

pytestmark = pytest.mark.gpu

dev = torch.device("cuda", 0)
F32, BF16 = torch.float32, torch.bfloat16
_DT = {F32: "f32", BF16: "bf16"}
THETA = 10000.0


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from learning_jax_sharding_amd.ops import hip as H
    H.lib()
    return H


@pytest.fixture
def watch(hip, monkeypatch):
    """run(fn) -> (result, launch names, calls of rope_reference)."""
    from learning_jax_sharding_amd.ops import kernels as K
    calls, ref = [], K.rope_reference
    monkeypatch.setattr(K, "rope_reference", lambda *a, **k: (calls.append(1), ref(*a, **k))[1])

    def run(fn):
        del calls[:]
        with hip.launch_log() as log:
            out = fn()
        torch.cuda.synchronize()
        return out, list(log), len(calls)
    return run


def _qk(shape, dtype, seed=0):
    gen = torch.Generator().manual_seed(seed + shape[-1] + 7 * shape[1])
    return torch.randn(*shape, generator=gen).to(dtype), torch.randn(*shape, generator=gen).to(dtype)


def _names(log):
    return [r["name"] for r in log if r["name"].startswith("rope<")]


CASES = ([((2, 5, 3, 64), a, a) for a in (BF16, F32)]
         + [((1, 3, 2, 16), a, b) for a in (F32, BF16) for b in (F32, BF16)]
         + [((1, 3, 1, 256), a, a) for a in (BF16, F32)]
         + [((2, 300, 8, 64), BF16, BF16)])


@pytest.mark.parametrize("off", [0, 1000])
@pytest.mark.parametrize("shape,idt,odt", CASES,
                         ids=["x".join(map(str, s)) + f"-{_DT[a]}-{_DT[b]}" for s, a, b in CASES])
def test_kernel_matches_float64_oracle(watch, shape, idt, odt, off):
    """q' and k' of one launch, and dq / dk of the inverse launch, per shape and dtype pair."""
    from learning_jax_sharding_amd.ops import kernels as K
    q, k = _qk(shape, idt)
    gq, gk = _qk(shape, odt, seed=50)
    qs, ks = q.to(dev).requires_grad_(True), k.to(dev).requires_grad_(True)

    def step():
        qo, ko = K.rope(qs, ks, off, THETA, odt)
        return (qo, ko) + torch.autograd.grad([qo, ko], [qs, ks], [gq.to(dev), gk.to(dev)])

    (qo, ko, dq, dk), log, ref_calls = watch(step)
    name, inv = f"rope<{_DT[idt]},{_DT[odt]}>", f"rope<{_DT[odt]},{_DT[idt]},inv>"
    assert _names(log) == [name, inv] and not ref_calls, (log, ref_calls)
    assert all(r["blocks"] >= 1 and r["block"] == 256 for r in log if r["name"].startswith("rope<"))
    assert qo.dtype == odt and ko.dtype == odt and dq.dtype == idt and dk.dtype == idt
    tag = f"{shape} {_DT[idt]}->{_DT[odt]} off={off}"
    O.check(f"{tag} q'", qo, *O.rotate64(q, off, THETA))
    O.check(f"{tag} k'", ko, *O.rotate64(k, off, THETA))
    O.check(f"{tag} dq", dq, *O.rotate64(gq, off, THETA, inverse=True))
    O.check(f"{tag} dk", dk, *O.rotate64(gk, off, THETA, inverse=True))


def test_grid_stride_tail(hip, watch):
    """(2, 300, 8, 64) bf16: 38400 items.  Capped at 7 blocks (1792 items per pass, a last pass of 768)
    the kernel walks the items grid-stride and gives the bits of the uncapped launch."""
    from learning_jax_sharding_amd.ops import kernels as K
    q, k = _qk((2, 300, 8, 64), BF16)
    qd, kd = q.to(dev), k.to(dev)
    (q0, k0), log0, _ = watch(lambda: K.rope(qd, kd, 3, THETA))
    hip.set_rope_max_blocks(7)
    try:
        (q1, k1), log1, ref_calls = watch(lambda: K.rope(qd, kd, 3, THETA))
    finally:
        hip.set_rope_max_blocks(None)
    recs = [r for r in log1 if r["name"] == "rope<bf16,bf16>"]
    assert len(recs) == 1 and recs[0]["blocks"] == 7 and not ref_calls, log1
    assert [r["blocks"] for r in log0 if r["name"] == "rope<bf16,bf16>"] == [150]
    assert torch.equal(q0, q1) and torch.equal(k0, k1)
    O.check("grid-stride q'", q1, *O.rotate64(q, 3, THETA))
    O.check("grid-stride k'", k1, *O.rotate64(k, 3, THETA))


def test_table_grows_between_calls(watch):
    """A table of its own (theta 5000): the first call makes 1024 rows, the second needs rows up to
    1000 + 37 and doubles it; the old table stays alive and both results hold the bounds."""
    from learning_jax_sharding_amd.ops import kernels as K
    theta = 5000.0
    q, k = _qk((2, 37, 3, 64), BF16)
    qd, kd = q.to(dev), k.to(dev)
    key = K.RopeTableCache._key(dev, 64, theta)
    assert key not in K._ROPE_TABLES.live
    n_old = len(K._ROPE_TABLES.superseded)
    (q0, _), log, _ = watch(lambda: K.rope(qd, kd, 0, theta))
    first = K._ROPE_TABLES.live[key]
    assert first[0].shape[0] == 1024 and first[0].is_cuda
    (q1, k1), log1, ref_calls = watch(lambda: K.rope(qd, kd, 1000, theta))
    assert _names(log) == _names(log1) == ["rope<bf16,bf16>"] and not ref_calls
    second = K._ROPE_TABLES.live[key]
    assert second[0].shape[0] == 2048 and torch.equal(second[0][:1024], first[0])
    assert len(K._ROPE_TABLES.superseded) == n_old + 1 and K._ROPE_TABLES.superseded[-1][0] is first[0]
    O.check("grow off=0 q'", q0, *O.rotate64(q, 0, theta))
    O.check("grow off=1000 q'", q1, *O.rotate64(q, 1000, theta))
    O.check("grow off=1000 k'", k1, *O.rotate64(k, 1000, theta))


def test_strided_inputs_in_place_of_the_fused_buffer(watch):
    """q and k as column blocks 0 and 1 of a [B, S, 3, H, D] projection buffer, and in seq-major
    storage: the bits of the launch on contiguous copies; the V block is not touched."""
    from learning_jax_sharding_amd.ops import kernels as K
    B, S, H, D = 2, 19, 3, 64
    gen = torch.Generator().manual_seed(11)
    buf = torch.randn(B, S, 3, H, D, generator=gen).to(BF16).to(dev)
    before = buf.clone()
    q, k = buf[:, :, 0], buf[:, :, 1]
    assert not q.is_contiguous()
    (qc, kc), _, _ = watch(lambda: K.rope(q.contiguous(), k.contiguous(), 5, THETA))
    (qv, kv), log, ref_calls = watch(lambda: K.rope(q, k, 5, THETA))
    assert _names(log) == ["rope<bf16,bf16>"] and not ref_calls
    assert torch.equal(qv, qc) and torch.equal(kv, kc)
    assert torch.equal(buf, before)            # inputs (and V) untouched: the rotation is out of place
    O.check("fused-buffer q'", qv, *O.rotate64(q, 5, THETA))
    qs = torch.empty(S, B, H, D, dtype=BF16, device=dev).permute(1, 0, 2, 3).copy_(q)
    ks = torch.empty(S, B, H, D, dtype=BF16, device=dev).permute(1, 0, 2, 3).copy_(k)
    assert qs.stride(1) > qs.stride(0)
    (qm, km), log, ref_calls = watch(lambda: K.rope(qs, ks, 5, THETA))
    assert _names(log) == ["rope<bf16,bf16>"] and not ref_calls
    assert qm.stride(1) > qm.stride(0)         # stored like the input
    assert torch.equal(qm, qc) and torch.equal(km, kc)


def test_single_tensor_position_zero_and_determinism(watch):
    """k = None; the row of position 0 is the input bit for bit; dx from autograd against the oracle,
    twice with identical bits."""
    from learning_jax_sharding_amd.ops import kernels as K
    for dtype in (F32, BF16):
        q, _ = _qk((2, 9, 3, 64), dtype)
        g, _ = _qk((2, 9, 3, 64), dtype, seed=9)
        qs = q.to(dev).requires_grad_(True)

        def step():
            qo, none = K.rope(qs, None, 0, THETA)
            assert none is None
            return qo, torch.autograd.grad(qo, qs, g.to(dev))[0]

        (qo, dx), log, ref_calls = watch(step)
        (qo2, dx2), _, _ = watch(step)
        assert _names(log) == [f"rope<{_DT[dtype]},{_DT[dtype]}>", f"rope<{_DT[dtype]},{_DT[dtype]},inv>"]
        assert not ref_calls
        assert torch.equal(qo[:, 0].cpu(), q[:, 0]) and not torch.equal(qo[:, 1].cpu(), q[:, 1])
        assert torch.equal(qo, qo2) and torch.equal(dx, dx2)
        O.check(f"k=None {_DT[dtype]} q'", qo, *O.rotate64(q, 0, THETA))
        O.check(f"k=None {_DT[dtype]} dx", dx, *O.rotate64(g, 0, THETA, inverse=True))


def test_rejected_shapes_write_nothing_and_take_the_torch_path(hip, watch):
    """head_dim 24 and a base misaligned by 2 bytes: the launcher returns a non-zero code and the
    output keeps its bits; the dispatcher runs the torch formulation with its warning."""
    from learning_jax_sharding_amd.ops import kernels as K
    cos, sin = K.rope_table(dev, 64, THETA, 16)
    cos24, sin24 = (t.to(dev) for t in K.rope_table_host(16, 24, THETA))
    q24 = torch.randn(1, 4, 2, 24).to(BF16).to(dev)
    flat = torch.randn(1 * 4 * 2 * 64 + 8).to(BF16).to(dev)
    qmis = flat[1:1 + 512].view(1, 4, 2, 64)
    assert qmis.data_ptr() % 16 == 2
    for name, q, c, s in (("D=24", q24, cos24, sin24), ("misaligned", qmis, cos, sin)):
        out = torch.full(q.shape, 7.0, dtype=BF16, device=dev)
        with hip.launch_log() as log:
            rc = hip.rope_raw(q, None, out, None, c, s, 0)
        torch.cuda.synchronize()
        assert rc != 0 and not _names(log), (name, rc)
        assert (out == 7.0).all(), name
        with pytest.raises(NotImplementedError):
            hip.rope(q, None, 0, THETA)
        K._WARNED_ROPE_D.discard(q.shape[-1])
        with pytest.warns(UserWarning, match="torch formulation"):
            (qo, _), log, ref_calls = watch(lambda: K.rope(q, None, 2, THETA))
        assert not _names(log) and ref_calls == 1, name
        O.check(f"{name} torch path", qo, *O.rotate64(q, 2, THETA))
    # a misaligned output is rejected as well
    q = torch.randn(1, 4, 2, 64).to(BF16).to(dev)
    assert hip.rope_raw(q, None, qmis, None, cos, sin, 0) != 0
    # and positions past the table
    assert hip.rope_raw(q, None, torch.empty_like(q), None, cos, sin, cos.shape[0] - 3) != 0


def test_fused_rope_off_takes_the_torch_path(watch, monkeypatch):
    from learning_jax_sharding_amd.ops import kernels as K
    monkeypatch.setenv("LJS_FUSED_ROPE", "0")
    q, k = _qk((2, 5, 3, 64), BF16)
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*rope kernel.*")   # a supported shape: no warning
        (qo, ko), log, ref_calls = watch(lambda: K.rope(q.to(dev), k.to(dev), 1000, THETA))
    assert not _names(log) and ref_calls == 1
    assert qo.is_cuda
    O.check("LJS_FUSED_ROPE=0 q'", qo, *O.rotate64(q, 1000, THETA))
    O.check("LJS_FUSED_ROPE=0 k'", ko, *O.rotate64(k, 1000, THETA))


def test_sharded_over_length_on_two_devices(gpu_devices, hip):
    """core.rope on 2 virtual GPU devices over length: the one-device bits, one launch per device."""
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd.mesh import Mesh, create_device_mesh
    from learning_jax_sharding_amd.ops import core
    from learning_jax_sharding_amd.sharding import NamedSharding, PartitionSpec as P
    q, k = _qk((2, 24, 2, 64), F32)
    gpu_devices(1)
    q1, k1 = core.rope(ljs.device_put(q.numpy()), ljs.device_put(k.numpy()), theta=THETA, dtype=BF16)
    one_q, one_k = q1.to_torch().cpu(), k1.to_torch().cpu()
    gpu_devices(2)
    mesh = Mesh(create_device_mesh((1, 2)), ("data", "model"))
    sh = NamedSharding(mesh, P(None, "model"))
    with hip.launch_log() as log:
        q2, k2 = core.rope(ljs.device_put(q.numpy(), sh), ljs.device_put(k.numpy(), sh), theta=THETA, dtype=BF16)
    torch.cuda.synchronize()
    assert _names(log) == ["rope<f32,bf16>"] * 2
    assert q2.tile.tile_shape == (1, 2, 1, 1)
    assert torch.equal(q2.to_torch().cpu(), one_q) and torch.equal(k2.to_torch().cpu(), one_k)
    O.check("sharded q'", one_q, *O.rotate64(q, 0, THETA))


def test_graph_capture_of_a_causal_rope_attention_block(gpu_devices, hip):
    """jit(capture=True) of a causal + RoPE MultiHeadAttention forward + grad: the warm-up call makes
    the table, the capture records the rope launches, the replays give the eager bits."""
    gpu_devices(1)
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd.models import MultiHeadAttention
    model = MultiHeadAttention(128, heads=2, dim_head=64, causal=True, rope_theta=THETA)
    x = ljs.random.normal(ljs.random.PRNGKey(0), (2, 64, 128))
    params = model.init(ljs.random.PRNGKey(1), x)["params"]
    loss = lambda p: model.apply({"params": p}, x).sum()  # noqa: E731
    with hip.launch_log() as log:
        v, g = ljs.value_and_grad(loss)(params)
    assert _names(log) == ["rope<bf16,bf16>", "rope<bf16,bf16,inv>"], [r["name"] for r in log]
    step = ljs.jit(ljs.value_and_grad(loss), capture=True)
    for _ in range(3):
        vj, gj = step(params)
    torch.cuda.synchronize()
    assert torch.equal(v.to_torch(), vj.to_torch())
    eager = [l.to_torch().clone() for l in ljs.tree_util.tree_leaves(ljs.nn.unbox(g))]
    graph = [l.to_torch().clone() for l in ljs.tree_util.tree_leaves(ljs.nn.unbox(gj))]
    assert len(eager) == 5
    for a, b in zip(eager, graph):
        assert torch.isfinite(a.float()).all() and torch.equal(a, b), (a.float() - b.float()).abs().max()
