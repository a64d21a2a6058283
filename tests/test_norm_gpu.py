"""Fused LayerNorm / RMSNorm HIP kernels (csrc/kernels/norm.hip) against a float64 oracle on the
CPU (run on a real MI355X: -m gpu).

The tolerance is measured against the reference, never against the kernels: ``E_ref`` is the
max-abs error of torch's own f32 evaluation of the same function on the GPU against the float64
oracle, per output.  An f32 output may be off by ``4 E_ref + 2^-23 max|f64|`` (another, equally
valid summation order; the floor covers outputs torch gets exactly, d(bias) of a single row), a
bf16 output by one bf16 ulp of the rounded oracle on top of that."""
import warnings

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

dev = torch.device("cuda", 0)
EPS = 1e-6
F32, BF16 = torch.float32, torch.bfloat16
_DT = {F32: "f32", BF16: "bf16"}
WAVE_MAX_D = 1024   # rows up to here: one wave per row; wider: one block per row


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from learning_jax_sharding_amd.ops import hip as H
    H.lib()
    return H


def _mapping(D):
    return "wave" if D <= WAVE_MAX_D else "block"


def _inputs(R, D, offset, xdt, ydt, params, kind, seed=0):
    """x (in xdt), the cotangent g (in ydt), scale, bias (f32 or None) on the CPU."""
    gen = torch.Generator(device="cpu").manual_seed(seed + 7 * R + D)
    x = (offset + 1.5 * torch.randn(R, D, generator=gen)).to(xdt)
    g = torch.randn(R, D, generator=gen).to(ydt)
    scale = (1.0 + 0.2 * torch.randn(D, generator=gen)) if params else None
    bias = (0.2 * torch.randn(D, generator=gen)) if params and kind == "layer" else None
    return x, g, scale, bias


def _formula(x, scale, bias, kind):
    """The function itself in x's precision (f64: the oracle; f32 on the GPU: torch's own error)."""
    if kind == "layer":
        return F.layer_norm(x, (x.shape[-1],), scale, bias, EPS)
    y = x * torch.rsqrt((x * x).mean(-1, keepdim=True) + EPS)
    return y if scale is None else y * scale


def _evaluate(x, g, scale, bias, kind, dtype, device):
    """(y, dx, dscale, dbias) of the formula evaluated in ``dtype`` on ``device``, as f64 on the CPU."""
    xs = x.to(device=device, dtype=dtype).requires_grad_(True)
    ps = [p.to(device=device, dtype=dtype).requires_grad_(True) if p is not None else None for p in (scale, bias)]
    y = _formula(xs, ps[0], ps[1], kind)
    wrt = [xs] + [p for p in ps if p is not None]
    grads = list(torch.autograd.grad(y, wrt, g.to(device=device, dtype=dtype)))
    out = {"y": y.detach(), "dx": grads.pop(0)}
    out["dscale"] = grads.pop(0) if ps[0] is not None else None
    out["dbias"] = grads.pop(0) if ps[1] is not None else None
    return {k: (v.double().cpu() if v is not None else None) for k, v in out.items()}


def _run_kernel(hip, x, g, scale, bias, kind, ydt, need_x=True, need_p=True):
    xs = x.to(dev).requires_grad_(need_x)
    ps = [p.to(dev).requires_grad_(need_p) if p is not None else None for p in (scale, bias)]
    y = hip.norm(xs, ps[0], ps[1], EPS, kind, ydt)
    wrt = ([xs] if need_x else []) + ([p for p in ps if p is not None] if need_p else [])
    grads = list(torch.autograd.grad(y, wrt, g.to(dev))) if wrt else []
    out = {"y": y.detach(), "dx": grads.pop(0) if need_x else None}
    out["dscale"] = grads.pop(0) if need_p and ps[0] is not None else None
    out["dbias"] = grads.pop(0) if need_p and ps[1] is not None else None
    return out


def _check(name, got, want64, ref32):
    """Assert one output against the rule of the module docstring; prints the figures first."""
    e_ref = (ref32 - want64).abs().max().item()
    slack = 4.0 * e_ref + 2.0 ** -23 * want64.abs().max().item()
    if got.dtype == BF16:
        want = want64.to(BF16).double()
        allowed = 2.0 ** -7 * want.abs() + slack
    else:
        want = want64
        allowed = torch.full_like(want, slack)
    err = (got.double().cpu() - want).abs()
    frac = (err / allowed).max().item()
    ratio = err.max().item() / e_ref if e_ref > 0 else float("inf") if err.max().item() > 0 else 0.0
    print(f"norm-figures {name} dtype={_DT[got.dtype]} max_err={err.max().item():.3e} E_ref={e_ref:.3e} "
          f"err/E_ref={ratio:.3f} worst_fraction_of_bound={frac:.3f}")
    assert torch.isfinite(got).all(), name
    assert frac <= 1.0, (name, err.max().item(), e_ref, frac)


SHAPES = [(257, 640), (1000, 512), (3, 64), (130, 8), (1, 648), (64, 4096), (5, 1024), (5, 1032)]
ALL4 = [(F32, F32), (F32, BF16), (BF16, F32), (BF16, BF16)]
CASES = [(R, D, xdt, ydt) for (R, D) in SHAPES
         for (xdt, ydt) in (ALL4 if (R, D) == (257, 640) else [(F32, BF16), (BF16, BF16)])]


@pytest.mark.parametrize("params", [True, False], ids=["params", "noparams"])
@pytest.mark.parametrize("kind", ["layer", "rms"])
@pytest.mark.parametrize("offset", [0.0, 100.0], ids=["centred", "offset100"])
@pytest.mark.parametrize("R,D,xdt,ydt", CASES, ids=[f"{R}x{D}-{_DT[a]}-{_DT[b]}" for R, D, a, b in CASES])
def test_norm_matches_float64_oracle(hip, R, D, xdt, ydt, offset, kind, params):
    x, g, scale, bias = _inputs(R, D, offset, xdt, ydt, params, kind)
    want = _evaluate(x, g, scale, bias, kind, torch.float64, "cpu")
    ref32 = _evaluate(x, g, scale, bias, kind, F32, dev)
    with hip.launch_log() as log:
        got = _run_kernel(hip, x, g, scale, bias, kind, ydt)
    torch.cuda.synchronize()
    names = [r["name"] for r in log if r["name"].startswith("norm_")]
    k, m = kind, _mapping(D)
    assert names == [f"norm_fwd<{k},{_DT[xdt]},{_DT[ydt]},{m}>", f"norm_bwd<{k},{_DT[xdt]},{_DT[ydt]},{m}>"], names
    assert got["y"].dtype == ydt and got["dx"].dtype == xdt
    tag = f"{kind} {R}x{D} {_DT[xdt]}->{_DT[ydt]} offset={offset:g} params={int(params)}"
    for out in ("y", "dx", "dscale", "dbias"):
        if want[out] is None:
            assert got[out] is None
            continue
        _check(f"{tag} {out}", got[out], want[out], ref32[out])


@pytest.mark.parametrize("kind,xdt,ydt,R,D", [("layer", F32, BF16, 257, 640), ("rms", BF16, BF16, 64, 4096),
                                              ("layer", BF16, F32, 1000, 512), ("rms", F32, F32, 5, 1032)])
def test_launch_record_names_the_kernel(hip, kind, xdt, ydt, R, D):
    """One forward and one backward launch, and nothing else from the library; the instance names
    spell the kind, the dtypes and the row mapping."""
    x, g, scale, bias = _inputs(R, D, 0.0, xdt, ydt, True, kind)
    with hip.launch_log() as log:
        _run_kernel(hip, x, g, scale, bias, kind, ydt)
    torch.cuda.synchronize()
    assert log.total == 2, [r["name"] for r in log]
    m = _mapping(D)
    assert [r["name"] for r in log] == [f"norm_fwd<{kind},{_DT[xdt]},{_DT[ydt]},{m}>",
                                        f"norm_bwd<{kind},{_DT[xdt]},{_DT[ydt]},{m}>"]
    assert log[0]["block"] == 256 and log[1]["block"] == (256 if m == "block" else 512)


@pytest.mark.parametrize("R,D", [(1000, 512), (257, 640), (64, 4096)])
def test_backward_is_deterministic(hip, R, D):
    x, g, scale, bias = _inputs(R, D, 0.0, BF16, BF16, True, "layer")
    a = _run_kernel(hip, x, g, scale, bias, "layer", BF16)
    b = _run_kernel(hip, x, g, scale, bias, "layer", BF16)
    torch.cuda.synchronize()
    for out in ("dx", "dscale", "dbias"):
        assert torch.equal(a[out], b[out]), out


def test_storage_order_without_a_copy(hip):
    """A seq-major [B][S][D] activation (a permuted view of a contiguous [S][B][D]) is processed in
    storage order: the kernel reads the tensor itself, y and dx take its strides, and the values
    are the contiguous run's bit for bit.  A tensor that is not dense (a column slice of a wider
    matrix) is made contiguous first and gives the contiguous run's values too."""
    B, S, D = 3, 40, 640
    gen = torch.Generator(device="cpu").manual_seed(3)
    base = torch.randn(S, B, D, generator=gen).to(BF16).to(dev)
    scale = (1.0 + 0.2 * torch.randn(D, generator=gen)).to(dev)
    bias = (0.2 * torch.randn(D, generator=gen)).to(dev)
    g = torch.randn(B, S, D, generator=gen).to(BF16).to(dev)
    wide = torch.randn(S, 2 * D, generator=gen).to(dev)
    for x, gx in ((base.permute(1, 0, 2), g), (wide[:, :D], g[0].float())):
        assert not x.is_contiguous()
        outs = []
        for xin in (x, x.contiguous()):
            xin = xin.detach().requires_grad_(True)
            y = hip.norm(xin, scale, bias, EPS, "layer", xin.dtype)
            saved = y.grad_fn.saved_tensors[0]
            (dx,) = torch.autograd.grad(y, xin, gx)
            outs.append((xin, y, dx, saved))
        (x0, y0, dx0, saved0), (x1, y1, dx1, _) = outs
        if x.dim() == 3:
            assert saved0.data_ptr() == x0.data_ptr() and saved0.stride() == x0.stride()   # no copy was made
            assert y0.stride() == x0.stride() and dx0.stride() == x0.stride()
        else:
            assert saved0.is_contiguous() and y0.is_contiguous()
        assert torch.equal(y0, y1) and torch.equal(dx0, dx1)


def test_graph_replay_rearms_the_tickets(hip):
    """Forward + backward captured once and replayed with new inputs: every replay equals the eager
    result for its input (a ticket left un-armed would skip the final reduction)."""
    R, D = 257, 640
    xs, gs = [], []
    for seed in (0, 1, 2):
        x, g, scale, bias = _inputs(R, D, 0.0, BF16, BF16, True, "layer", seed=seed)
        xs.append(x.to(dev))
        gs.append(g.to(dev))
    _, _, scale, bias = _inputs(R, D, 0.0, BF16, BF16, True, "layer", seed=0)
    scale, bias = scale.to(dev).requires_grad_(True), bias.to(dev).requires_grad_(True)
    sx, sg = xs[0].clone().requires_grad_(True), gs[0].clone()

    def step():
        y = hip.norm(sx, scale, bias, EPS, "layer", BF16)
        return (y.detach(),) + tuple(torch.autograd.grad(y, (sx, scale, bias), sg))

    eager = []
    for x, g in zip(xs, gs):
        with torch.no_grad():
            sx.copy_(x)
            sg.copy_(g)
        eager.append([t.clone() for t in step()])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.autograd.set_multithreading_enabled(False), torch.cuda.graph(graph, stream=side):
        static = step()
    for i in (1, 2):
        with torch.no_grad():
            sx.copy_(xs[i])
            sg.copy_(gs[i])
        graph.replay()
        torch.cuda.synchronize()
        for name, a, b in zip(("y", "dx", "dscale", "dbias"), static, eager[i]):
            assert torch.equal(a, b), (i, name)


@pytest.mark.parametrize("kind", ["layer", "rms"])
def test_skipped_outputs(hip, kind):
    """Only the gradients that are asked for come back, equal to the full run's."""
    x, g, scale, bias = _inputs(257, 640, 0.0, F32, BF16, True, kind)
    full = _run_kernel(hip, x, g, scale, bias, kind, BF16)
    only_p = _run_kernel(hip, x, g, scale, bias, kind, BF16, need_x=False)
    only_x = _run_kernel(hip, x, g, scale, bias, kind, BF16, need_p=False)
    torch.cuda.synchronize()
    assert only_p["dx"] is None and only_x["dscale"] is None and only_x["dbias"] is None
    assert torch.equal(only_p["dscale"], full["dscale"])
    if kind == "layer":
        assert torch.equal(only_p["dbias"], full["dbias"])
    assert torch.equal(only_x["dx"], full["dx"])


def test_unsupported_width_falls_back_with_one_warning(hip):
    """D = 100 on a GPU tensor: the torch formulation, one warning, no norm_* launch."""
    from learning_jax_sharding_amd.ops import kernels as K
    K._WARNED_NORM_D.discard(100)
    x, g, scale, bias = _inputs(33, 100, 0.0, F32, F32, True, "layer")
    want = _evaluate(x, g, scale, bias, "layer", torch.float64, "cpu")
    xs = x.to(dev).requires_grad_(True)
    sc, bi = scale.to(dev).requires_grad_(True), bias.to(dev).requires_grad_(True)
    with hip.launch_log() as log:
        with pytest.warns(UserWarning, match="100 features"):
            y = K.layer_norm(xs, sc, bi, EPS, "layer", F32)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            K.layer_norm(xs, sc, bi, EPS, "layer", F32)
        dx, ds, db = torch.autograd.grad(y, (xs, sc, bi), g.to(dev))
    torch.cuda.synchronize()
    assert not [r["name"] for r in log if r["name"].startswith("norm_")]
    # an f32 evaluation of sums of 100 (33 for the parameter gradients) terms of order 1: within
    # 64 f32 ulps of the largest value
    for name, got in (("y", y.detach()), ("dx", dx), ("dscale", ds), ("dbias", db)):
        err = (got.double().cpu() - want[name]).abs().max().item()
        assert err <= 64 * 2.0 ** -23 * want[name].abs().max().item(), (name, err)
