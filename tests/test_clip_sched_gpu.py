"""The clipping / schedule kernels on a real MI355X (-m gpu): grad_sumsq against the float64 sum of
squares within the bound derived in tests/clip_oracle.py, its determinism under graph replay, the
dynamic Adam instance against the static one bit for bit, and step_hyper against the host
schedule objects."""
import math

import numpy as np
import pytest
import torch

import clip_oracle as CO

pytestmark = pytest.mark.gpu

dev = torch.device("cuda", 0)


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from learning_jax_sharding_amd.ops import hip as H
    H.lib()
    return H


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _check_sumsq(hip, name, sources, f32_grads):
    """One grad_sumsq call over ``sources`` against the float64 sum of squares of ``f32_grads`` (the
    f32 values the kernel squares), every launch's slot held to its own bound."""
    slots = hip.grad_sumsq(sources, dev).clone()
    torch.cuda.synchronize()
    assert slots.dtype == torch.float64 and slots.numel() == (len(sources) + 31) // 32
    worst = 0.0
    for k in range(slots.numel()):
        gs = f32_grads[32 * k:32 * k + 32]
        want = CO.sumsq64(gs)
        units = CO.sumsq_allowed_units([tuple(g.shape) for g in gs])
        err = abs(slots[k].item() - want)
        frac = err / (units * CO.U * want) if want > 0 else float(err != 0)
        worst = max(worst, frac)
        print(f"clip-figures grad_sumsq {name} launch={k} want={want:.9g} rel_err={err / max(want, 1e-300):.3e} "
              f"allowed={units:.2f}u worst_fraction_of_bound={frac:.3f}")
        assert err <= units * CO.U * want, (name, k, err, units * CO.U * want)
    return slots, worst


@pytest.mark.parametrize("shape", [(1,), (7,), (33, 65), (64, 64), (130, 192), (640, 512)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_grad_sumsq_plain(hip, shape, dtype):
    g = torch.randn(*shape, generator=_gen(1)).to(dtype).to(dev)
    with hip.launch_log() as log:
        _check_sumsq(hip, f"plain{shape}{dtype}", [(shape, g)], [g.float()])
    assert [r["name"] for r in log] == ["grad_sumsq"]
    tiles = CO.sumsq_tiles([shape])
    assert log[0]["blocks"] == tiles and log[0]["block"] == 256      # the grid is the tile count


def _slab_case(hip, S, dtype, ld_extra, r_off, c_off, R=130, C=192):
    """S slabs of a [R + 6][C + ld_extra] buffer; the gradient is the [R][C] block at (r_off, c_off).
    Returns (SlabGrad, the f32 gradient slab_reduce produces for that block)."""
    RT, LD = R + 6, C + ld_extra
    slabs = torch.randn(S, RT, LD, generator=_gen(2 + S)).to(dtype).to(dev)
    full = torch.empty(RT, LD, device=dev)
    hip.slab_reduce(slabs, full, LD, RT * LD)
    g = full[r_off:r_off + R, c_off:c_off + C].contiguous()
    return hip.SlabGrad(slabs, S, r_off * LD + c_off, LD, RT * LD, (R, C)), g


@pytest.mark.parametrize("S", [1, 3, 5, 9, 24])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_grad_sumsq_slabs(hip, S, dtype):
    """Split-K slabs with ld > C and a non-zero offset are summed in slab_reduce's order, then
    squared: 16-byte loads (aligned offset) and the scalar path (odd offset)."""
    for name, (r_off, c_off) in (("vec", (2, 8)), ("scalar", (3, 5))):
        sg, g = _slab_case(hip, S, dtype, 16, r_off, c_off)
        _check_sumsq(hip, f"slabs S={S} {dtype} {name}", [((130, 192), sg)], [g])


def test_grad_sumsq_const_and_mixed_two_launches(hip):
    """A constant gradient, and 40 tensors of every source form: two launches, two slots."""
    c = hip.ConstGrad(0.37, (70, 130))
    cg = torch.full((70, 130), 0.37, dtype=torch.float32)
    _check_sumsq(hip, "const", [((70, 130), c)], [cg])
    sources, grads = [], []
    shapes = [(1,), (7,), (33, 65), (64, 64), (96, 100), (128,), (200, 132), (64, 256)]
    for i in range(40):
        shape = shapes[i % len(shapes)]
        if i % 10 == 3:
            sg, g = _slab_case(hip, 3 + i % 4, torch.float32, 8, 1, 4, R=66, C=68)
            sources.append(((66, 68), sg)), grads.append(g)
        elif i % 10 == 7:
            sources.append((shape, hip.ConstGrad(-0.01 * i, shape))), grads.append(torch.full(shape, -0.01 * i))
        else:
            g = torch.randn(*shape, generator=_gen(100 + i)).to(torch.bfloat16 if i % 3 == 0 else torch.float32).to(dev)
            sources.append((shape, g)), grads.append(g.float())
    with hip.launch_log() as log:
        slots, _ = _check_sumsq(hip, "mixed40", sources, grads)
    assert [r["name"] for r in log] == ["grad_sumsq", "grad_sumsq"] and slots.numel() == 2


def test_grad_sumsq_deterministic_and_rearmed_under_replay(hip):
    """Two runs give equal bits; five replays of one captured launch give equal bits (the tickets
    are re-armed by the launch itself: no memset between replays)."""
    srcs = [((640, 512), torch.randn(640, 512, generator=_gen(5)).to(dev)),
            ((130, 192), torch.randn(130, 192, generator=_gen(6)).to(torch.bfloat16).to(dev))]
    a = hip.grad_sumsq(srcs, dev).clone()
    b = hip.grad_sumsq(srcs, dev).clone()
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    out = torch.zeros(1, dtype=torch.float64, device=dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out.copy_(hip.grad_sumsq(srcs, dev))
    got = []
    for _ in range(5):
        out.zero_()
        graph.replay()
        got.append(out.clone())
    torch.cuda.synchronize()
    for g in got:
        assert torch.equal(g.view(torch.int64), a.view(torch.int64))


# ---------------------------------------------------------------------------- dynamic Adam
LR, B1, B2, EPS, WD = 1e-3, 0.9, 0.999, 1e-8, 0.01


def _adam_case(hip, kind, scale):
    """(entries of the dynamic run, entries of the static run fed with ``scale`` x the gradient)."""
    from learning_jax_sharding_amd.ops import shadow
    shapes = [(640, 512), (200, 132), (70, 66), (640,)]
    gen = _gen(11)
    dyn, sta = [], []
    for shape in shapes:
        w = torch.randn(*shape, generator=gen).to(dev)
        m = (torch.randn(*shape, generator=gen) * 0.1).to(dev)
        v = (torch.rand(*shape, generator=gen) * 1e-3).to(dev)
        if kind == "slab" and len(shape) == 2:
            S, (R, C) = 5, shape
            slabs = torch.randn(S, R, C, generator=gen).to(dev)
            g1 = hip.SlabGrad(slabs, S, 0, C, R * C, shape)
            g2 = hip.SlabGrad(slabs * scale, S, 0, C, R * C, shape)
        elif kind == "const":
            g1, g2 = hip.ConstGrad(0.25, shape), hip.ConstGrad(0.25 * scale, shape)
        else:
            g = torch.randn(*shape, generator=gen).to(torch.bfloat16 if kind == "bf16" else torch.float32).to(dev)
            g1, g2 = g, g * scale
        a, b = (w.clone(), g1, m.clone(), v.clone()), (w.clone(), g2, m.clone(), v.clone())
        for t in (a[0], b[0]):
            if t.dim() == 2:
                shadow.get(t, "T")
                shadow.get(t, "N")
        dyn.append(a), sta.append(b)
    return dyn, sta


@pytest.mark.parametrize("rows", [16, 32, 64])
@pytest.mark.parametrize("kind", ["plain", "bf16", "slab", "const"])
@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_dynamic_adam_equals_static_bit_for_bit(hip, rows, kind, scale):
    """The dynamic instance with the record {scale, f32(lr)} == the static instance fed with the
    gradient (every slab) times scale (a power of two commutes with the f32 sums): p, m, v and both
    bf16 shadows, at every tile height."""
    from learning_jax_sharding_amd.ops import shadow
    dyn, sta = _adam_case(hip, kind, scale)
    rec = torch.tensor([scale, LR, 0.0, 0.0], dtype=torch.float32, device=dev)
    step = torch.full((), 3, dtype=torch.int32, device=dev)
    hip.set_adam_rows(rows)
    try:
        with hip.launch_log() as log:
            hip.adam_multi(dyn, step, 0.0, B1, B2, EPS, WD, hyper=rec)
        hip.adam_multi(sta, step, float(np.float32(LR)), B1, B2, EPS, WD)
    finally:
        hip.set_adam_rows(0)
    torch.cuda.synchronize()
    assert [r["name"] for r in log] == [f"adam_multi_dyn<{rows}>"]
    for a, b in zip(dyn, sta):
        for x, y, what in ((a[0], b[0], "p"), (a[2], b[2], "m"), (a[3], b[3], "v")):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (kind, tuple(x.shape), what)
        if a[0].dim() == 2:
            ea, eb = shadow.entry(a[0], create=False), shadow.entry(b[0], create=False)
            for k in ("T", "N"):
                assert torch.equal(ea.bufs[k].view(torch.int16), eb.bufs[k].view(torch.int16)), (kind, k)
            assert torch.equal(ea.bufs["N"], a[0].bfloat16())


# ---------------------------------------------------------------------------- step_hyper
WARMUP, DECAY = 5, 20
COUNTS = (0, 1, WARMUP - 1, WARMUP, WARMUP + 1, DECAY - 1, DECAY, DECAY + 17)


def _schedules():
    from learning_jax_sharding_amd import optim
    return {"constant": optim.constant_schedule(3e-4), "linear": optim.linear_schedule(1e-3, 1e-5, DECAY),
            "linear_begin": optim.linear_schedule(2e-3, 1e-4, DECAY - WARMUP, transition_begin=WARMUP),
            "linear_steps0": optim.linear_schedule(1e-3, 1e-5, 0),
            "cosine": optim.cosine_decay_schedule(1e-3, DECAY, alpha=0.1),
            "warmup_cosine": optim.warmup_cosine_decay_schedule(1e-5, 1e-3, WARMUP, DECAY, end_value=1e-4)}


def test_step_hyper_schedules_and_step_offset(hip):
    """lr == f32(schedule(count)) within 1 f32 ulp; the count is *step + step_offset - 1, so a
    pending offset of 0, 1 or 3 gives the value of the step being taken."""
    recs, want = [], []
    for name, s in _schedules().items():
        for c in COUNTS:
            for off in (0, 1, 3):
                step = torch.full((), c + 1 - off, dtype=torch.int32, device=dev)
                recs.append(hip.step_hyper(step, off, schedule=s))
                want.append((name, c, off, s(c)))
    with hip.launch_log() as log:
        recs.append(hip.step_hyper(torch.full((), 4, dtype=torch.int32, device=dev), 1, lr=2.5e-4))
        want.append(("float", 4, 1, 2.5e-4))
    assert [r["name"] for r in log] == ["step_hyper"] and log[0]["blocks"] == 1 and log[0]["block"] == 64
    got = torch.stack(recs).cpu()
    worst = 0.0
    for r, (name, c, off, w) in zip(got, want):
        u = CO.ulps32(r[1].item(), w)
        worst = max(worst, u)
        assert u <= 1.0, (name, c, off, r[1].item(), w)
        assert r[0].item() == 1.0 and r[2].item() == 0.0        # no clip: scale 1, no norm
    print(f"clip-figures step_hyper lr worst_ulps_f32={worst:.3f}")


@pytest.mark.parametrize("case", ["active", "inactive", "zero", "equal", "gathered"])
def test_step_hyper_norm_and_scale(hip, case):
    """sqrt of the slots (or the gathered per-device sums) added in index order in float64, rounded
    once: norm and grad_scale within 1 f32 ulp of the float64 oracle."""
    vals = {"active": [3.0, 1e-3, 250.5, 7.25], "inactive": [0.5, 0.25], "zero": [0.0, 0.0], "equal": [3600.0, 3625.0],
            "gathered": [1.5, 0.0, 2.25, 1e3]}[case]
    v = torch.tensor(vals, dtype=torch.float64, device=dev)
    total = 0.0
    for x in vals:
        total += x
    norm = math.sqrt(total)
    max_norm = {"active": 2.0, "inactive": 5.0, "zero": 1.0, "equal": 85.0, "gathered": 3.0}[case]
    step = torch.ones((), dtype=torch.int32, device=dev)
    if case == "gathered":
        junk = torch.full((3,), 1e30, dtype=torch.float64, device=dev)      # the slots are ignored
        rec = hip.step_hyper(step, 0, lr=1e-3, max_norm=max_norm, slots=junk, gathered=v)
        part = hip.sumsq_partial(v)
    else:
        rec = hip.step_hyper(step, 0, lr=1e-3, max_norm=max_norm, slots=v)
        part = hip.sumsq_partial(v)
    rec, part = rec.cpu(), part.cpu()
    assert part.item() == total                                  # index order, float64
    sc = CO.scale64(norm, max_norm)
    assert CO.ulps32(rec[2].item(), norm) <= 1.0 and CO.ulps32(rec[0].item(), sc) <= 1.0, (rec, norm, sc)
    assert (rec[0].item() < 1.0) == (case in ("active", "gathered"))
    assert rec[1].item() == float(np.float32(1e-3))
