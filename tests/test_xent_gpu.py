"""Fused softmax cross-entropy HIP kernels (csrc/kernels/xent.hip) against a float64 oracle on
the CPU (run on a real MI355X: -m gpu).

The tolerance is the rule of tests/test_norm_gpu.py, measured against the reference, never against
the kernels: ``E_ref`` is the max-abs error of torch's own f32 evaluation of F.cross_entropy on the
GPU against the float64 oracle, per output.  An f32 output may be off by ``4 E_ref + 2^-23 max|f64|``,
a bf16 dx by one bf16 ulp of the rounded oracle (``2^-7 |rounded oracle|``) on top of that."""
import pytest
import torch
import torch.nn.functional as F

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


def _mapping(hip, V):
    return "wave" if V <= hip.XENT_WAVE_MAX_V else "block"


def _labels(R, V, gen, dtype=torch.int64):
    """Random labels with, on the first rows (as many as there are): column 0, column V - 1, an
    ignored row, and both sides of the boundary between two vocabulary shards."""
    lab = torch.randint(0, V, (R,), generator=gen)
    for i, v in enumerate((0, V - 1, -1, V // 2, max(V // 2 - 1, 0))[:R]):
        lab[i] = v
    return lab.to(dtype)


def _inputs(R, V, offset, std, dtype, seed=0, label_dtype=torch.int64):
    """Logits (in dtype), labels and the loss rows' cotangent (f32) on the CPU."""
    gen = torch.Generator(device="cpu").manual_seed(seed + 7 * R + V)
    x = (offset + std * torch.randn(R, V, generator=gen)).to(dtype)
    return x, _labels(R, V, gen, label_dtype), torch.randn(R, generator=gen)


def _evaluate(x, lab, g, dtype, device):
    """(loss rows, dx) of F.cross_entropy evaluated in ``dtype`` on ``device``, as f64 on the CPU."""
    xs = x.to(device=device, dtype=dtype).requires_grad_(True)
    loss = F.cross_entropy(xs, lab.long().to(device), reduction="none", ignore_index=-1)
    (dx,) = torch.autograd.grad(loss, xs, g.to(device=device, dtype=dtype))
    return {"loss": loss.detach().double().cpu(), "dx": dx.double().cpu()}


_REFS = {}


def _references(key, x, lab, g):
    """The float64 oracle and torch's f32 evaluation on the GPU for one input set: computed once,
    shared by the tests that use the set, never modified."""
    if key not in _REFS:
        _REFS[key] = (_evaluate(x, lab, g, torch.float64, "cpu"), _evaluate(x, lab, g, F32, dev))
    return _REFS[key]


def _run_kernel(hip, x, lab, g):
    xs = x.to(dev).requires_grad_(True)
    loss = hip.xent(xs, lab.to(dev))
    (dx,) = torch.autograd.grad(loss, xs, g.to(dev))
    return {"loss": loss.detach(), "dx": dx}


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
    worst = err.max().item()
    if worst == 0.0:
        frac = 0.0
    else:
        frac = torch.where(err > 0, err / allowed, torch.zeros_like(err)).max().item()
    ratio = worst / e_ref if e_ref > 0 else float("inf") if worst > 0 else 0.0
    print(f"xent-figures {name} dtype={_DT[got.dtype]} max_err={worst:.3e} E_ref={e_ref:.3e} "
          f"err/E_ref={ratio:.3f} worst_fraction_of_bound={frac:.3f}")
    assert torch.isfinite(got).all(), name
    assert frac <= 1.0, (name, worst, e_ref, frac)


def _shapes():
    from learning_jax_sharding_amd.ops import hip as H
    try:
        thr = int(H.XENT_WAVE_MAX_V)
    except (RuntimeError, OSError):   # no library (collection without a build): the tests skip anyway
        thr = 2048
    return [(1, 1), (3, 7), (130, 64), (257, 1000), (5, 1031), (3, 50257), (2, 262144), (6, thr), (6, thr + 8)]


SHAPES = _shapes()
DISTS = [(0.0, 1.5), (100.0, 1.5), (0.0, 8.0)]


@pytest.mark.parametrize("offset,std", DISTS, ids=["std1.5", "offset100", "std8"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("R,V", SHAPES, ids=[f"{R}x{V}" for R, V in SHAPES])
def test_xent_matches_float64_oracle(hip, R, V, dtype, offset, std):
    # int32 labels on the wide-spread inputs, int64 elsewhere: both instances run at every shape
    x, lab, g = _inputs(R, V, offset, std, dtype, label_dtype=torch.int32 if std == 8.0 else torch.int64)
    want, ref32 = _references((R, V, dtype, offset, std), x, lab, g)
    with hip.launch_log() as log:
        got = _run_kernel(hip, x, lab, g)
    torch.cuda.synchronize()
    names = [r["name"] for r in log if r["name"].startswith("xent_")]
    m = _mapping(hip, V)
    assert names == [f"xent_fwd<{_DT[dtype]},{m}>", f"xent_bwd<{_DT[dtype]},{m}>"], names
    assert log.total == 2, [r["name"] for r in log]
    assert got["loss"].dtype == F32 and got["dx"].dtype == dtype and got["dx"].is_contiguous()
    tag = f"{R}x{V} {_DT[dtype]} offset={offset:g} std={std:g}"
    for out in ("loss", "dx"):
        _check(f"{tag} {out}", got[out], want[out], ref32[out])
    ignored = (lab < 0).nonzero().flatten().tolist()
    for r in ignored:
        assert got["loss"][r].item() == 0.0 and not got["dx"][r].any()


def test_threshold_pair_takes_both_mappings(hip):
    thr = hip.XENT_WAVE_MAX_V
    assert (6, thr) in SHAPES and (6, thr + 8) in SHAPES
    assert _mapping(hip, thr) == "wave" and _mapping(hip, thr + 8) == "block" and (thr + 8) % 8 == 0


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_vocab_shard_statistics_merge_on_the_host(hip, dtype):
    """Columns 500..1499 of a 257 x 2000 problem as one shard (vocab_offset 500, row stride 2000, rows
    off the 16-byte grid), the rest as two more; the statistics merged as ops.core merges them match
    the whole-row oracle, loss and dx, under the same rule."""
    R, V = 257, 2000
    x, lab, g = _inputs(R, V, 0.0, 1.5, dtype, seed=5)
    lab[3], lab[4], lab[5], lab[6] = 499, 500, 1499, 1500
    want, ref32 = _references(("shard", dtype), x, lab, g)
    xs = x.to(dev).requires_grad_(True)
    labd = lab.to(dev)
    parts = [(0, 500), (500, 1500), (1500, 2000)]
    with hip.launch_log() as log:
        st = [hip.xent_stats(xs[:, lo:hi], labd, lo) for lo, hi in parts]
        m = torch.stack([s[0] for s in st])
        assert not m.requires_grad
        ls, t = torch.stack([s[1] for s in st]), torch.stack([s[2] for s in st])
        own = torch.stack([(labd >= lo) & (labd < hi) for lo, hi in parts]).float()
        rel = m - m.amax(0)
        loss = torch.log((ls.exp() * rel.exp()).sum(0)) - (own * (t + rel)).sum(0)
        loss = torch.where(labd >= 0, loss, torch.zeros_like(loss))
        (dx,) = torch.autograd.grad(loss, xs, g.to(dev))
    torch.cuda.synchronize()
    names = [r["name"] for r in log if r["name"].startswith("xent_")]
    assert sorted(names) == [f"xent_bwd<{_DT[dtype]},wave>"] * 3 + [f"xent_fwd<{_DT[dtype]},wave>"] * 3, names
    # each shard's t is zero exactly where it does not own the label
    for (lo, hi), s in zip(parts, st):
        assert not s[2][~((labd >= lo) & (labd < hi))].any()
    _check(f"shard 257x1000@500 {_DT[dtype]} loss", loss.detach(), want["loss"], ref32["loss"])
    # dx is the sum of three bf16 slices written separately: each element is one kernel's output
    _check(f"shard 257x1000@500 {_DT[dtype]} dx", dx, want["dx"], ref32["dx"])


def test_strided_rows_past_2_31(hip):
    """A [:, :1031] view of a [3, 2^30] bf16 allocation (never initialised, only the view is touched):
    row offsets of 2^30 and 2^31 elements.  Loss and dx are the contiguous copy's bit for bit, dx is
    a fresh contiguous tensor, and the columns right of the view keep their values."""
    R, V, LD = 3, 1031, 2 ** 30
    x, lab, g = _inputs(R, V, 0.0, 1.5, BF16, seed=9)
    big = torch.empty(R, LD, dtype=BF16, device=dev)
    guard = torch.full((R, 64), 3.0, dtype=BF16, device=dev)
    big[:, V:V + 64] = guard
    big[:, :V] = x.to(dev)
    view = big[:, :V]
    assert view.stride() == (LD, 1) and not view.is_contiguous()
    outs = []
    for xin in (view, view.contiguous()):
        xin = xin.detach().requires_grad_(True)
        loss = hip.xent(xin, lab.to(dev))
        (dx,) = torch.autograd.grad(loss, xin, g.to(dev))
        outs.append((loss.detach(), dx))
    torch.cuda.synchronize()
    (l0, d0), (l1, d1) = outs
    assert torch.equal(l0, l1) and torch.equal(d0, d1)
    assert d0.is_contiguous() and d0.shape == (R, V) and d0.data_ptr() != big.data_ptr()
    assert torch.equal(big[:, V:V + 64], guard) and torch.equal(big[:, :V], x.to(dev))
    want, ref32 = _references(("strided",), x, lab, g)
    _check("strided 3x1031 bf16 loss", l0, want["loss"], ref32["loss"])
    _check("strided 3x1031 bf16 dx", d0, want["dx"], ref32["dx"])
    del big
    torch.cuda.empty_cache()


@pytest.mark.parametrize("R,V,dtype", [(257, 1000, BF16), (3, 50257, F32)])
def test_runs_are_bit_identical(hip, R, V, dtype):
    x, lab, g = _inputs(R, V, 0.0, 1.5, dtype)
    a = _run_kernel(hip, x, lab, g)
    b = _run_kernel(hip, x, lab, g)
    torch.cuda.synchronize()
    assert torch.equal(a["loss"], b["loss"]) and torch.equal(a["dx"], b["dx"])


@pytest.mark.parametrize("R,V", [(257, 1000), (5, 4104)], ids=["wave", "block"])
def test_graph_replay_matches_eager(hip, R, V):
    """Forward + backward captured once and replayed twice with new values in the static inputs:
    every replay equals the eager result for its input bit for bit (nothing to re-arm)."""
    sets = [_inputs(R, V, 0.0, 1.5, BF16, seed=seed) for seed in (0, 1, 2)]
    sx = sets[0][0].to(dev).requires_grad_(True)
    sl, sg = sets[0][1].to(dev), sets[0][2].to(dev)

    def step():
        loss = hip.xent(sx, sl)
        return loss.detach(), torch.autograd.grad(loss, sx, sg)[0]

    def load(i):
        with torch.no_grad():
            sx.copy_(sets[i][0])
            sl.copy_(sets[i][1])
            sg.copy_(sets[i][2])

    eager = []
    for i in range(3):
        load(i)
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
        load(i)
        graph.replay()
        torch.cuda.synchronize()
        for name, a, b in zip(("loss", "dx"), static, eager[i]):
            assert torch.equal(a, b), (i, name)


def test_switch_off_takes_the_torch_formulation(hip, monkeypatch):
    """LJS_FUSED_XENT=0: no xent_ launch, results still within the rule."""
    from learning_jax_sharding_amd.ops import kernels as K
    R, V = 257, 1000
    x, lab, g = _inputs(R, V, 0.0, 1.5, F32)
    want, ref32 = _references((R, V, F32, 0.0, 1.5), x, lab, g)
    for flag, fused in (("0", False), ("1", True)):
        monkeypatch.setenv("LJS_FUSED_XENT", flag)
        xs = x.to(dev).requires_grad_(True)
        with hip.launch_log() as log:
            loss = K.softmax_xent(xs, lab.to(dev))
            (dx,) = torch.autograd.grad(loss, xs, g.to(dev))
        torch.cuda.synchronize()
        assert bool([r["name"] for r in log if r["name"].startswith("xent_")]) == fused
        _check(f"LJS_FUSED_XENT={flag} loss", loss.detach(), want["loss"], ref32["loss"])
        _check(f"LJS_FUSED_XENT={flag} dx", dx, want["dx"], ref32["dx"])
