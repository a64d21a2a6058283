"""The fused SwiGLU HIP kernels (csrc/kernels/swiglu.hip) on a real MI355X (-m gpu) against the
float64 oracle and bounds of tests/swiglu_oracle.py.  Every kernel case goes through the dispatcher
(ops/kernels.py swiglu) and asserts from the launch log that exactly the expected ``swiglu<...>`` /
``swiglu_bwd<...>`` instances ran and that the torch formulation was not called."""
import warnings

import numpy as np
import pytest
import torch

import swiglu_oracle as O

pytestmark = pytest.mark.gpu

dev = torch.device("cuda", 0)
F32, BF16 = torch.float32, torch.bfloat16
_DT = {F32: "f32", BF16: "bf16"}


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from learning_jax_sharding_amd.ops import hip as H
    H.lib()
    return H


@pytest.fixture
def watch(hip, monkeypatch):
    """run(fn) -> (result, launch records, calls of swiglu_reference)."""
    from learning_jax_sharding_amd.ops import kernels as K
    calls, ref = [], K.swiglu_reference
    monkeypatch.setattr(K, "swiglu_reference", lambda *a, **k: (calls.append(1), ref(*a, **k))[1])

    def run(fn):
        del calls[:]
        with hip.launch_log() as log:
            out = fn()
        torch.cuda.synchronize()
        return out, list(log), len(calls)
    return run


def _names(log):
    recs = [r for r in log if r["name"].startswith("swiglu")]
    assert all(r["block"] == 256 and r["blocks"] >= 1 for r in recs), recs
    return [r["name"] for r in recs]


def _fwd_bwd(g, u, dh, odt):
    """(h, dg, du) through the dispatcher and autograd, from host tensors."""
    from learning_jax_sharding_amd.ops import kernels as K
    gs, us = g.to(dev).requires_grad_(True), u.to(dev).requires_grad_(True)

    def step():
        h = K.swiglu(gs, us, odt)
        return (h,) + torch.autograd.grad(h, [gs, us], dh.to(dev))
    return step


def _check(tag, g, u, dh, h, dg, du):
    """All three results against the oracle; returns the worst figures."""
    dg64, mdg, du64, mdu = O.backward64(g, u, dh)
    return (O.check(f"{tag} h", h, *O.forward64(g, u), O.U_H), O.check(f"{tag} dg", dg, dg64, mdg, O.U_DG),
            O.check(f"{tag} du", du, du64, mdu, O.U_DU))


CASES = ([((1, 3, 8), a, b) for a in (F32, BF16) for b in (F32, BF16)]
         + [((2, 5, 264), a, a) for a in (BF16, F32)]
         + [((1, 2, 14336), BF16, BF16)])


@pytest.mark.parametrize("shape,idt,odt", CASES,
                         ids=["x".join(map(str, s)) + f"-{_DT[a]}-{_DT[b]}" for s, a, b in CASES])
def test_kernel_matches_float64_oracle(watch, shape, idt, odt):
    """h of the forward launch and (dg, du) of the backward launch, per shape and dtype pair."""
    g, u, dh = O.inputs(shape, idt, odt)
    (h, dg, du), log, ref_calls = watch(_fwd_bwd(g, u, dh, odt))
    assert _names(log) == [f"swiglu<{_DT[idt]},{_DT[odt]}>", f"swiglu_bwd<{_DT[odt]},{_DT[idt]}>"], log
    assert not ref_calls
    assert h.dtype == odt and dg.dtype == idt and du.dtype == idt
    _check(f"{shape} {_DT[idt]}->{_DT[odt]}", g, u, dh, h, dg, du)


def test_column_blocks_of_the_fused_projection_buffer(watch):
    """g and u as the two column blocks of one [T][2F] bf16 buffer: read in place, and dg and du come
    back as the same two column blocks of one fresh buffer (what ops/linear.py _wgrads tests for)."""
    T, F = 10, 264
    g, u, dh = O.inputs((1, T, F), BF16, BF16, seed=3)
    buf = torch.cat([g[0], u[0]], dim=1).to(dev)
    before = buf.clone()
    gv, uv = buf[:, :F].requires_grad_(True), buf[:, F:].requires_grad_(True)
    assert not gv.is_contiguous() and uv.data_ptr() == gv.data_ptr() + 2 * F
    from learning_jax_sharding_amd.ops import kernels as K

    def step():
        h = K.swiglu(gv, uv)
        return (h,) + torch.autograd.grad(h, [gv, uv], dh[0].to(dev))

    (h, dg, du), log, ref_calls = watch(step)
    assert _names(log) == ["swiglu<bf16,bf16>", "swiglu_bwd<bf16,bf16>"] and not ref_calls
    assert torch.equal(buf, before)
    assert tuple(h.shape) == (T, F) and h.is_contiguous()
    assert du.data_ptr() == dg.data_ptr() + 2 * F and dg.stride() == du.stride() == (2 * F, 1)
    _check("fused-buffer", g[0], u[0], dh[0], h, dg, du)
    # separate tensors give two contiguous gradients with the same bits
    (h2, dg2, du2), _, _ = watch(_fwd_bwd(g[0], u[0], dh[0], BF16))
    assert dg2.is_contiguous() and du2.is_contiguous()
    assert torch.equal(h, h2) and torch.equal(dg, dg2) and torch.equal(du, du2)


def test_seq_major_view(watch):
    """[S][B][F] storage presented as (B, S, F): the bits of the launch on contiguous copies, and the
    results stored like the input."""
    from learning_jax_sharding_amd.ops import kernels as K
    B, S, F = 3, 7, 72
    g, u, dh = O.inputs((B, S, F), BF16, BF16, seed=5)
    (hc, dgc, duc), _, _ = watch(_fwd_bwd(g, u, dh, BF16))

    def seq_major(t):
        return torch.empty(S, B, F, dtype=t.dtype, device=dev).permute(1, 0, 2).copy_(t)

    gs, us = seq_major(g).requires_grad_(True), seq_major(u).requires_grad_(True)
    assert gs.stride(1) > gs.stride(0)

    def step():
        h = K.swiglu(gs, us)
        return (h,) + torch.autograd.grad(h, [gs, us], dh.to(dev))

    (h, dg, du), log, ref_calls = watch(step)
    assert _names(log) == ["swiglu<bf16,bf16>", "swiglu_bwd<bf16,bf16>"] and not ref_calls
    assert h.stride(1) > h.stride(0) and dg.stride(1) > dg.stride(0)
    assert torch.equal(h, hc) and torch.equal(dg, dgc) and torch.equal(du, duc)


def test_grid_stride_tail(hip, watch):
    """(2, 300, 640) bf16: 48000 items, 188 blocks.  Capped at 7 blocks (1792 items per pass, a last
    pass of 1408) the kernels walk the items grid-stride and give the bits of the uncapped launches."""
    g, u, dh = O.inputs((2, 300, 640), BF16, BF16)
    step = _fwd_bwd(g, u, dh, BF16)
    out0, log0, _ = watch(step)
    hip.set_swiglu_max_blocks(7)
    try:
        out1, log1, ref_calls = watch(step)
    finally:
        hip.set_swiglu_max_blocks(None)
    assert [r["blocks"] for r in log0 if r["name"].startswith("swiglu")] == [188, 188]
    assert [r["blocks"] for r in log1 if r["name"].startswith("swiglu")] == [7, 7] and not ref_calls
    assert _names(log1) == ["swiglu<bf16,bf16>", "swiglu_bwd<bf16,bf16>"]
    for a, b in zip(out0, out1):
        assert torch.equal(a, b)
    _check("grid-stride", g, u, dh, *out1)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_extreme_gates(watch, dtype):
    """g in {+-100, +-1e4} with |u|, |dh| <= 4: everything finite; for g > 0 the usual bounds; for
    g <= -100 |h|, |dg| and |du| are at most 2^-120 (the true values are below 2e-41; a flushed
    subnormal is allowed)."""
    gen = torch.Generator().manual_seed(17)
    vals = torch.tensor([100.0, 1e4, -100.0, -1e4])
    g = vals.view(1, 4, 1).expand(1, 4, 16).contiguous().to(dtype)

    def mag():
        t = torch.randn(1, 4, 16, generator=gen) * 2
        return (torch.where(t < 0, -1.0, 1.0) * t.abs().clamp(2.0 ** -10, 4.0)).to(dtype)

    u, dh = mag(), mag()
    (h, dg, du), log, ref_calls = watch(_fwd_bwd(g, u, dh, dtype))
    assert _names(log) == [f"swiglu<{_DT[dtype]},{_DT[dtype]}>", f"swiglu_bwd<{_DT[dtype]},{_DT[dtype]}>"]
    assert not ref_calls
    for t in (h, dg, du):
        assert torch.isfinite(t).all()
        assert float(t.detach()[:, 2:].float().abs().max()) <= 2.0 ** -120
    _check(f"extremes {_DT[dtype]} g>0", g[:, :2], u[:, :2], dh[:, :2], h[:, :2], dg[:, :2], du[:, :2])


def test_rejected_shapes_write_nothing_and_take_the_torch_path(hip, watch):
    """F = 12 and a base misaligned by 2 bytes: the launchers return a non-zero code, launch nothing
    and leave the outputs as they were; the dispatcher runs the torch formulation with its warning."""
    from learning_jax_sharding_amd.ops import kernels as K
    g12, u12, dh12 = O.inputs((1, 4, 12), BF16, BF16)
    gm, um, dhm = O.inputs((1, 4, 64), BF16, BF16)

    def misaligned(t):
        flat = torch.zeros(t.numel() + 8, dtype=t.dtype, device=dev)
        v = flat[1:1 + t.numel()].view(t.shape).copy_(t)
        assert v.data_ptr() % 16 == 2
        return v

    for name, g, u, dh, gd, ud in (("F=12", g12, u12, dh12, g12.to(dev), u12.to(dev)),
                                   ("misaligned", gm, um, dhm, misaligned(gm), um.to(dev))):
        out = torch.full(g.shape, 7.0, dtype=BF16, device=dev)
        o2, o3 = out.clone(), out.clone()
        with hip.launch_log() as log:
            rc = hip.swiglu_raw(gd, ud, out)
            rcb = hip.swiglu_bwd_raw(gd, ud, dh.to(dev), o2, o3)
        torch.cuda.synchronize()
        assert rc != 0 and rcb != 0 and not _names(log), (name, rc, rcb)
        assert (out == 7.0).all() and (o2 == 7.0).all() and (o3 == 7.0).all(), name
        assert not hip.swiglu_supported(gd, ud)
        with pytest.raises(NotImplementedError):
            hip.swiglu(gd, ud)
        K._WARNED_SWIGLU.discard(g.shape[-1])
        gs, us = gd.requires_grad_(True), ud.requires_grad_(True)

        def step():
            h = K.swiglu(gs, us)
            return (h,) + torch.autograd.grad(h, [gs, us], dh.to(dev))

        with pytest.warns(UserWarning, match="torch formulation"):
            (h, dg, du), log, ref_calls = watch(step)
        assert not _names(log) and ref_calls == 1 and h.is_cuda, name
        _check(f"{name} torch path", g, u, dh, h, dg, du)
    # a misaligned output is rejected as well
    assert hip.swiglu_raw(gm.to(dev), um.to(dev), misaligned(gm)) != 0


def test_fused_swiglu_off_takes_the_torch_path(watch, monkeypatch):
    monkeypatch.setenv("LJS_FUSED_SWIGLU", "0")
    g, u, dh = O.inputs((2, 5, 264), BF16, BF16)
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*swiglu kernels.*")   # a supported shape: no warning
        (h, dg, du), log, ref_calls = watch(_fwd_bwd(g, u, dh, BF16))
    assert not _names(log) and ref_calls == 1 and h.is_cuda
    _check("LJS_FUSED_SWIGLU=0", g, u, dh, h, dg, du)


def test_two_runs_are_bit_equal(watch):
    g, u, dh = O.inputs((2, 37, 264), BF16, BF16, seed=9)
    step = _fwd_bwd(g, u, dh, BF16)
    a, log, ref_calls = watch(step)
    b, _, _ = watch(step)
    assert _names(log) == ["swiglu<bf16,bf16>", "swiglu_bwd<bf16,bf16>"] and not ref_calls
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def _gff(F=256):
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd import nn
    model = nn.GatedFeedForward(F)
    x = ljs.random.normal(ljs.random.PRNGKey(0), (2, 128, 128))
    params = model.init(ljs.random.PRNGKey(1), x)["params"]

    cot = ljs.random.normal(ljs.random.PRNGKey(2), (2, 128, 128))     # the output's cotangent, of order one

    def loss(p, xs):
        y = model.apply({"params": p}, xs, residual=xs)
        return (y.astype(ljs.numpy.float32) * cot).sum()
    return model, x, params, loss


def test_graph_capture_of_a_gated_feed_forward_step(gpu_devices, hip):
    """jit(capture=True) of a GatedFeedForward forward + grad (T = 256, d = 128, F = 256): the warm-up
    call and the capture each record the two launches, the replays record none and give the eager bits."""
    gpu_devices(1)
    import learning_jax_sharding_amd as ljs
    model, x, params, loss = _gff()
    with hip.launch_log() as log:
        v, g = ljs.value_and_grad(lambda p: loss(p, x))(params)
    assert _names(log) == ["swiglu<bf16,bf16>", "swiglu_bwd<bf16,bf16>"], [r["name"] for r in log]
    step = ljs.jit(ljs.value_and_grad(lambda p: loss(p, x)), capture=True)
    seen = []
    for _ in range(4):
        with hip.launch_log() as log:
            vj, gj = step(params)
        seen.append(_names(log))
    torch.cuda.synchronize()
    assert seen[0] == seen[1] == ["swiglu<bf16,bf16>", "swiglu_bwd<bf16,bf16>"], seen
    assert seen[2] == seen[3] == [], seen
    assert torch.equal(v.to_torch(), vj.to_torch())
    eager = [l.to_torch().clone() for l in ljs.tree_util.tree_leaves(ljs.nn.unbox(g))]
    graph = [l.to_torch().clone() for l in ljs.tree_util.tree_leaves(ljs.nn.unbox(gj))]
    assert len(eager) == 3
    for a, b in zip(eager, graph):
        assert torch.isfinite(a.float()).all() and torch.equal(a, b), (a.float() - b.float()).abs().max()


def test_gated_feed_forward_matches_host(host_devices, gpu_devices, hip):
    """GatedFeedForward at T = 256, d = 128, F = 256 on one GPU against the same module on host
    devices: output, dx and the three weight gradients within rtol 2e-2, atol 5e-2 (the bf16
    tolerance of tests/test_dense_paths_gpu.py)."""
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd import nn
    res = {}
    for kind, make in (("host", host_devices), ("gpu", gpu_devices)):
        make(1)
        model, x, params, loss = _gff()
        with hip.launch_log() as log:
            y = model.apply({"params": params}, x, residual=x)
            val, (gp, gx) = ljs.value_and_grad(loss, argnums=(0, 1))(params, x)
        names = _names(log)
        out = {"y": y.to_torch().float().cpu(), "dx": gx.to_torch().float().cpu()}
        out.update({k: v.to_torch().float().cpu() for k, v in nn.unbox(gp).items()})
        res[kind] = out
        assert names == (["swiglu<bf16,bf16>"] * 2 + ["swiglu_bwd<bf16,bf16>"] if kind == "gpu" else []), names
    assert sorted(res["gpu"]) == ["dx", "w_gate", "w_out", "w_up", "y"]
    for k, a in res["host"].items():
        b = res["gpu"][k]
        print(f"swiglu-figures module {k} max|host|={a.abs().max():.4g} max|gpu-host|={(b - a).abs().max():.4g}")
        np.testing.assert_allclose(b.numpy(), a.numpy(), rtol=2e-2, atol=5e-2, err_msg=k)
