"""The fused Adam kernels on a real MI355X (-m gpu), instance by instance against the float64 oracle
of tests/adam_oracle.py: p, m and v at every element within the bound derived there, the bf16 and
MX-fp8 shadows bit for bit against the kernel's own new p, the launch log for the instance and the
tile count the per-tensor heights imply, and a sentinel around every buffer the kernel writes."""
import numpy as np
import pytest
import torch

import adam_oracle as AO

pytestmark = pytest.mark.gpu

dev = torch.device("cuda", 0)
PAD = 64 * 64            # elements of padding on each side of every written buffer: one 64 x 64 tile
SENTINEL = 0x7B
CASES = AO.case_names()


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from learning_jax_sharding_amd.ops import hip as H
    H.lib()
    return H


class Padded:
    """``n`` elements of ``dtype`` inside a larger buffer of sentinel bytes, ``off`` elements past the
    aligned start."""

    def __init__(self, n, dtype, off=0, init=None):
        self.buf = torch.empty(n + 2 * PAD + off, dtype=dtype, device=dev)
        self.bytes = self.buf.view(torch.uint8)
        self.bytes.fill_(SENTINEL)
        self.lo, self.hi = (PAD + off) * self.buf.element_size(), (PAD + off + n) * self.buf.element_size()
        self.t = self.buf[PAD + off:PAD + off + n]
        if init is not None:
            self.t.copy_(torch.as_tensor(init).reshape(-1))

    def untouched(self):
        return bool((self.bytes[:self.lo] == SENTINEL).all()) and bool((self.bytes[self.hi:] == SENTINEL).all())


def spec(shape, src="f32", S=0, slab_off="aligned", shadows="", misaligned=False, const=0.37):
    shape = tuple(shape)
    R, C = (shape[0], shape[1]) if len(shape) == 2 else (1, int(np.prod(shape)))
    grad_vec = src in ("f32", "bf16", "const") or slab_off == "aligned"
    return dict(shape=shape, R=R, C=C, src=src, S=S if src.startswith("slab") else 0, slab_off=slab_off,
                shadows=shadows if len(shape) == 2 else "", misaligned=misaligned, const=const,
                mx="Q" in shadows, vec=(not misaligned) and C % 4 == 0 and grad_vec)


def build(hip, sp, case, seed):
    """One tensor of a launch: padded p / m / v (and shadows), its gradient source, and the f32
    gradient the kernel's moment updates see before any clipping scale."""
    from learning_jax_sharding_amd.ops import shadow
    R, C, shape = sp["R"], sp["C"], sp["shape"]
    n = R * C
    h, p0, g0, m0, v0 = AO.make_case(case, n, seed)
    off = 1 if sp["misaligned"] else 0
    bufs = {"p": Padded(n, torch.float32, off, p0), "m": Padded(n, torch.float32, 0, m0),
            "v": Padded(n, torch.float32, off, v0)}
    p, m, v = (bufs[k].t.view(shape) for k in "pmv")
    keep = []
    src = sp["src"]
    if src == "const":
        g_in, g_eff = hip.ConstGrad(sp["const"], shape), np.full(n, np.float32(sp["const"]), dtype=np.float32)
    elif src in ("f32", "bf16"):
        g_in = torch.as_tensor(g0).view(shape).to(torch.bfloat16 if src == "bf16" else torch.float32).to(dev)
        g_eff = AO.a32(g_in)
    else:
        # S slabs of a [R + 6][C + 16] buffer of noise; the gradient is the [R][C] block at an offset
        # that keeps 16-byte loads (2, 8) or forces the scalar path (3, 5).  Each slab of the block
        # is the case's gradient times a random weight, so the zero band sums to exactly 0.
        S, LD, RT = sp["S"], C + 16 + (-C) % 4, R + 6       # (slab_reduce, the reference, wants ld % 4 == 0)
        r_off, c_off = (2, 8) if sp["slab_off"] == "aligned" else (3, 5)
        rng = np.random.default_rng([seed, S, 77])
        slabs = (rng.standard_normal((S, RT, LD)) * np.abs(g0).max()).astype(np.float32)
        wts = (rng.random((S, R, C)) * (2.0 / S)).astype(np.float32)
        slabs[:, r_off:r_off + R, c_off:c_off + C] = g0.reshape(1, R, C) * wts
        slabs = torch.as_tensor(slabs).to(torch.bfloat16 if src == "slab_bf16" else torch.float32).to(dev)
        full = torch.empty(RT, LD, device=dev)
        hip.slab_reduce(slabs, full, LD, RT * LD)
        g_eff = AO.a32(full[r_off:r_off + R, c_off:c_off + C].contiguous())
        g_in = hip.SlabGrad(slabs, S, r_off * LD + c_off, LD, RT * LD, shape)
        keep.append(slabs)
    if sp["shadows"]:
        e = shadow.entry(p)
        for kind in sp["shadows"]:
            if kind in "NT":
                bufs[kind] = Padded(n, torch.bfloat16)
                e.bufs[kind] = bufs[kind].t.view((R, C) if kind == "N" else (C, R))
                e.versions[kind] = -1
            elif kind == "Q":
                for k, qs in (("QN", (R, C)), ("QT", (C, R))):
                    bufs[k] = Padded(n, torch.uint8)
                    bufs[k + "s"] = Padded(n // 32, torch.uint8)
                    e.bufs[k], e.bufs[k + "s"] = bufs[k].t.view(qs), bufs[k + "s"].t.view(qs[0], qs[1] // 32)
                    e.versions[k] = e.versions[k + "s"] = -1
    return dict(sp=sp, h=h, p=p, m=m, v=v, g_in=g_in, g_eff=g_eff, bufs=bufs, keep=keep,
                p0=p0.copy(), m0=m0.copy(), v0=v0.copy())


def forget(tensors):
    from learning_jax_sharding_amd.ops import shadow
    for t in tensors:
        shadow._REG.pop(shadow._key(t["p"]), None)


def expected_launches(specs, rows, dyn, cast_n=0):
    """[(instance name, blocks)] of the launches of one adam_multi call (32 tensors each)."""
    out = []
    for i in range(0, len(specs), 32):
        launch_rows, _, tiles = AO.launch_tiles(specs[i:i + 32], rows)
        if i + 32 >= len(specs) and cast_n > 0:
            tiles += min(2048, -(-cast_n // 2048))
        out.append((f"adam_multi{'_dyn' if dyn else ''}<{launch_rows}>", tiles))
    return out


def verify(hip, fig, label, tensors, h, scale=None):
    """p, m, v of every tensor against the oracle at every element (one figure per output over the
    launch), the shadows against the kernel's own new p, every buffer's padding."""
    from learning_jax_sharding_amd.ops import fp8 as F
    torch.cuda.synchronize()
    got, want, allowed = ([], [], []), ([], [], []), ([], [], [])
    for i, t in enumerate(tensors):
        g = t["g_eff"] if scale is None else AO.scaled(t["g_eff"], scale)
        w, a = AO.oracle(t["p0"], g, t["m0"], t["v0"], h), AO.bound(t["p0"], g, t["m0"], t["v0"], h)
        for k, out in enumerate("pmv"):
            got[k].append(AO.a64(t[out])), want[k].append(w[k]), allowed[k].append(a[k])
        sp, bufs, p = t["sp"], t["bufs"], t["p"]
        what = f"{label} tensor {i} {sp['shape']} {sp['src']}"
        if "N" in bufs:
            fig.equal(f"{what} shadow N", torch.equal(bufs["N"].t.view(torch.int16), p.bfloat16().view(-1).view(torch.int16)))
        if "T" in bufs:
            fig.equal(f"{what} shadow T", torch.equal(bufs["T"].t.view(torch.int16),
                                                      p.bfloat16().t().contiguous().view(-1).view(torch.int16)))
        if "QN" in bufs:
            pc = p.clone()
            (qn, sn), (qt, st) = F.quant_rows(pc), F.quant_cols(pc)
            for k, ref in (("QN", qn), ("QNs", sn), ("QT", qt), ("QTs", st)):
                fig.equal(f"{what} shadow {k}", torch.equal(bufs[k].t, ref.reshape(-1)))
        for k, b in bufs.items():
            fig.equal(f"{what} padding of {k}", b.untouched(), "(a write outside the tensor)")
    for k, out in enumerate("pmv"):
        fig.check(f"{label} {out}", got[k], want[k], allowed[k])


def run(hip, fig, label, specs, case, rows=0, dyn=None, offset=None, seed=0, cast_n=0):
    """One adam_multi call over ``specs`` in hyperparameter case ``case``, launched and verified.
    ``dyn``: (grad_scale, lr) of the record of the dynamic instance; ``offset``: a pending count
    offset given through ``taken=``.  Returns the tensors (for bit comparisons between runs)."""
    tensors = [build(hip, sp, case, seed + 17 * i) for i, sp in enumerate(specs)]
    h = tensors[0]["h"]
    try:
        step = torch.full((), h.t - (offset or 0), dtype=torch.int32, device=dev)
        entries = [(t["p"], t["g_in"], t["m"], t["v"]) for t in tensors]
        kw = {} if offset is None else {"taken": (offset, None)}
        hip.set_adam_rows(rows)
        try:
            with hip.launch_log() as log:
                if dyn is not None:
                    rec = torch.tensor([dyn[0], dyn[1], 0.0, 0.0], dtype=torch.float32, device=dev)
                    hip.adam_multi(entries, step, 7.0, h.b1, h.b2, h.eps, h.wd, hyper=rec, **kw)   # (lr = 7: ignored)
                    h = h._replace(lr=dyn[1])
                else:
                    hip.adam_multi(entries, step, h.lr, h.b1, h.b2, h.eps, h.wd, **kw)
        finally:
            hip.set_adam_rows(0)
        names = [(r["name"], r["blocks"]) for r in log if r["name"].startswith("adam_multi")]
        assert names == expected_launches(specs, rows, dyn is not None, cast_n), (label, names)
        assert all(r["block"] == 256 for r in log)
        assert int(step) == h.t - (offset or 0)                      # no increment asked for: none made
        verify(hip, fig, label, tensors, h, None if dyn is None else dyn[0])
    finally:
        forget(tensors)
    return tensors


# ---------------------------------------------------------------------------- adam_f32
@pytest.mark.parametrize("case", CASES)
def test_adam_f32(hip, case):
    """hip.adam: one element, a scalar tail only, one 4-wide group, several blocks with a tail; f32
    and bf16 gradients; out of place (the inputs keep their bits); the count as an int64 tensor."""
    fig = AO.Figures()
    for n in (1, 3, 4, 4099):
        for gd in (torch.float32, torch.bfloat16):
            h, p0, g0, m0, v0 = AO.make_case(case, n, seed=n)
            p, m, v = (torch.as_tensor(a).to(dev) for a in (p0, m0, v0))
            g = torch.as_tensor(g0).to(gd).to(dev)
            step = torch.full((), h.t, dtype=torch.int64 if n == 3 else torch.int32, device=dev)
            inplace = n == 4099 and gd == torch.float32
            with hip.launch_log() as log:
                po, mo, vo = hip.adam(p, g, m, v, step, h.lr, h.b1, h.b2, h.eps, h.wd, inplace=inplace)
            torch.cuda.synchronize()
            assert [(r["name"], r["blocks"], r["block"]) for r in log] == [("adam_f32", -(-n // 1024), 256)]
            if inplace:
                assert po.data_ptr() == p.data_ptr() and mo.data_ptr() == m.data_ptr() and vo.data_ptr() == v.data_ptr()
            else:
                for a, b in ((p, p0), (m, m0), (v, v0)):
                    assert np.array_equal(AO.a32(a).view(np.int32), b.view(np.int32))
            ge = AO.a32(g)
            want, allowed = AO.oracle(p0, ge, m0, v0, h), AO.bound(p0, ge, m0, v0, h)
            for k, (out, x) in enumerate(zip("pmv", (po, mo, vo))):
                fig.check(f"adam_f32 {case} n={n} g={str(gd)[6:]} {out}", x, want[k], allowed[k])
    fig.finish()


# ---------------------------------------------------------------------------- adam_multi, static
def _edge_specs(shadows):
    return [spec((128, 128), shadows=shadows),                   # full 4-wide tiles, several per tensor
            spec((70, 128), shadows=shadows),                    # ragged rows, R % 4 != 0: the transposed shadow's scalar stores
            spec((96, 100), shadows=shadows),                    # a 4-wide tensor whose last column tile takes the scalar path
            spec((33, 7), shadows=shadows),                      # scalar path (C % 4 != 0)
            spec((1,)), spec((640,)),                            # one-dimensional: one row of C columns
            spec((64, 64), shadows=shadows, misaligned=True)]    # p and v one element into their buffers: scalar path


@pytest.mark.parametrize("rows", [0, 16, 32, 64])
@pytest.mark.parametrize("shadows", ["", "N", "T", "NT"])
def test_static_shapes_heights_and_shadows(hip, rows, shadows):
    """Every tile path of the static instances at every height, with and without each bf16 shadow,
    and no write outside any tensor or shadow (the ragged, column-tail and misaligned shapes have a
    tile that overhangs), in every hyperparameter case."""
    fig = AO.Figures()
    for case in CASES:
        run(hip, fig, f"static rows={rows} shadows={shadows or '-'} {case}", _edge_specs(shadows), case, rows=rows,
            seed=len(shadows))
    fig.finish()


@pytest.mark.parametrize("rows", [0, 64])
def test_mx_and_plain_tensors_in_one_launch(hip, rows):
    """MX-fp8 shadows make the launch 64 rows high; the plain 4-wide tensors beside them keep 32-row
    tiles (automatic height only), the scalar one takes the launch's."""
    fig = AO.Figures()
    specs = [spec((64, 64), shadows="Q"), spec((128, 64), shadows="QNT"), spec((128, 128), shadows="NT"),
             spec((70, 128), src="bf16", shadows="T"), spec((33, 7), shadows="N")]
    launch_rows, heights, _ = AO.launch_tiles(specs, rows)
    assert launch_rows == 64 and heights == ([64, 64, 32, 32, 64] if rows == 0 else [64] * 5)
    for case in ("warm/wd=0.1", "large_count/wd=0", "eps/wd=0.1"):
        run(hip, fig, f"mx+plain rows={rows} {case}", specs, case, rows=rows)
    fig.finish()


# ---------------------------------------------------------------------------- gradient sources
def _source_specs(kind, shape=(70, 128)):
    if kind.startswith("slab"):
        # ld = C + 16; an offset that keeps the 16-byte loads, and an odd one (scalar path)
        return [spec(shape, src=kind, S=S, slab_off=o) for S in (1, 2, 4, 5, 9) for o in ("aligned", "odd")]
    return [spec(shape, src=kind), spec((96, 100), src=kind), spec((33, 7), src=kind), spec((640,), src=kind)]


@pytest.mark.parametrize("rows", [0, 16, 32, 64])
@pytest.mark.parametrize("kind", ["f32", "bf16", "slab_f32", "slab_bf16", "const"])
def test_gradient_sources(hip, rows, kind):
    """Plain f32 / bf16 gradients, f32 / bf16 split-K slabs (1, 2, 4, 5, 9 of them: no group of four,
    one group, a group and a remainder, two groups) with ld > C and a non-zero offset, and a constant
    gradient, at every height, in every hyperparameter case."""
    fig = AO.Figures()
    for case in CASES:
        run(hip, fig, f"source {kind} rows={rows} {case}", _source_specs(kind), case, rows=rows, seed=3)
    fig.finish()


@pytest.mark.parametrize("rows", [0, 64])
def test_slab_counts_choose_heights_per_tensor(hip, rows):
    """S = 2, 4, 8 slab gradients in one launch: at a forced 64-row launch the tensors get 64-, 32-
    and 16-row tiles (32, 16, 16 at the automatic 32), proved by the launch's block count."""
    fig = AO.Figures()
    specs = [spec((128, 64), src="slab_f32", S=2), spec((128, 64), src="slab_bf16", S=4),
             spec((128, 128), src="slab_f32", S=8, shadows="NT"), spec((70, 128), src="slab_f32", S=8, slab_off="odd")]
    launch_rows, heights, tiles = AO.launch_tiles(specs, rows)
    assert (launch_rows, heights) == ((64, [64, 32, 16, 64]) if rows == 64 else (32, [32, 16, 16, 32]))
    for case in ("warm/wd=0.1", "small_p/wd=0"):
        run(hip, fig, f"slab heights rows={rows} {case}", specs, case, rows=rows)
    fig.finish()


def test_forty_tensors_two_launches(hip):
    """40 tensors of every source kind: two launches, each with its own tile plan."""
    fig = AO.Figures()
    shapes = [(64, 64), (33, 7), (70, 128), (96, 100), (640,)]
    kinds = ["f32", "bf16", "const", "slab_f32", "slab_bf16"]
    specs = []
    for i in range(40):
        sh, kind = shapes[i % 5], kinds[(i // 5) % 5]
        if kind.startswith("slab") and len(sh) == 1:
            kind = "f32"
        specs.append(spec(sh, src=kind, S=1 + i % 4, slab_off="odd" if i % 3 == 0 else "aligned",
                          shadows="NT" if i % 2 else "", const=0.01 * (i - 20)))
    assert len(expected_launches(specs, 0, False)) == 2
    run(hip, fig, "forty warm/wd=0.1", specs, "warm/wd=0.1")
    fig.finish()


# ---------------------------------------------------------------------------- dynamic instance
@pytest.mark.parametrize("rows", [16, 32, 64])
@pytest.mark.parametrize("scale", [0.3, 1.0])
def test_dynamic_instance(hip, rows, scale):
    """The record's grad_scale (0.3: not a power of two, so f32(g * scale) rounds) and learning rate
    (not the ignored lr argument), over every source kind and tile path."""
    fig = AO.Figures()
    specs = (_edge_specs("NT")[:4] + [spec((640,), src="bf16"), spec((70, 128), src="bf16", shadows="T"),
                                       spec((70, 128), src="const"), spec((33, 7), src="const", const=-1e-4)]
             + [spec((70, 128), src=k, S=S, slab_off=o) for k, S, o in (("slab_f32", 5, "aligned"), ("slab_bf16", 9, "odd"),
                                                                        ("slab_bf16", 2, "aligned"))])
    for case in CASES:
        run(hip, fig, f"dyn rows={rows} scale={scale} {case}", specs, case, rows=rows, dyn=(scale, 2.5e-4), seed=5)
    fig.finish()


# ---------------------------------------------------------------------------- count plumbing
@pytest.mark.parametrize("dyn", [False, True])
def test_increment_step_three_calls(hip, dyn):
    """increment_step from a non-zero start: every call uses the count after its own increment and
    is held to the oracle at that t from the kernel's own state of the call before."""
    fig = AO.Figures()
    start, case = 6, "warm/wd=0.1"
    specs = [spec((70, 128), shadows="NT"), spec((33, 7)), spec((640,), src="bf16")]
    tensors = [build(hip, sp, case, 9 + i) for i, sp in enumerate(specs)]
    try:
        step = torch.full((), start, dtype=torch.int32, device=dev)
        rec = torch.tensor([0.3, 2.5e-4, 0.0, 0.0], dtype=torch.float32, device=dev)
        entries = [(t["p"], t["g_in"], t["m"], t["v"]) for t in tensors]
        for call in range(3):
            h = tensors[0]["h"]._replace(t=start + call + 1)
            if dyn:
                hip.adam_multi(entries, step, 7.0, h.b1, h.b2, h.eps, h.wd, increment_step=True, hyper=rec)
                h = h._replace(lr=2.5e-4)
            else:
                hip.adam_multi(entries, step, h.lr, h.b1, h.b2, h.eps, h.wd, increment_step=True)
            assert int(step) == start + call + 1
            verify(hip, fig, f"increment dyn={dyn} call={call} t={h.t}", tensors, h, 0.3 if dyn else None)
            for t in tensors:
                t["p0"], t["m0"], t["v0"] = (AO.a32(t[k]).copy() for k in "pmv")
    finally:
        forget(tensors)
    fig.finish()


@pytest.mark.parametrize("offset", [0, 1, 3])
def test_taken_offset(hip, offset):
    """A pending offset given through ``taken=``: the kernel uses *step + offset, the count stays."""
    fig = AO.Figures()
    specs = [spec((70, 128)), spec((33, 7), src="bf16"), spec((1,))]
    for case in ("warm/wd=0", "large_count/wd=0.1"):
        run(hip, fig, f"taken offset={offset} static {case}", specs, case, offset=offset)
        run(hip, fig, f"taken offset={offset} dyn {case}", specs, case, offset=offset, dyn=(0.3, 2.5e-4))
    fig.finish()


# ---------------------------------------------------------------------------- the cast job
@pytest.mark.parametrize("dyn", [None, (0.3, 2.5e-4)])
def test_cast_job_rides_the_last_launch(hip, monkeypatch, dyn):
    """The launch's extra blocks cast the next step's input: the destination equals src.bfloat16()
    bit for bit, nothing around it is written, and p / m / v are bit-identical to the same call
    without the cast.  Lengths: whole chunks with a tail, a tail alone, several grid-stride passes
    (more than 2048 blocks' worth), none."""
    from learning_jax_sharding_amd.ops import linear
    fig = AO.Figures()
    specs = [spec((70, 128), shadows="NT"), spec((33, 7)), spec((128, 64), src="slab_f32", S=5)]
    case = "warm/wd=0.1"
    base = None
    for n in (0, 8 * 2048 * 2 + 5, 5, 2048 * 2048 * 2 + 8 * 3 + 5):
        taken, committed = [], []
        if n:
            src = torch.randn(n, generator=torch.Generator().manual_seed(n)).to(dev)
            dst = Padded(n, torch.bfloat16)

            def take(device, src=src, dst=dst):
                taken.append(device)
                return (src, dst.t, src) if len(taken) == 1 else None
            monkeypatch.setattr(linear, "take_optimizer_precast", take)
            monkeypatch.setattr(linear, "commit_optimizer_precast", committed.append)
        else:
            monkeypatch.setattr(linear, "take_optimizer_precast", lambda device: None)
        tensors = run(hip, fig, f"cast n={n} dyn={dyn is not None}", specs, case, dyn=dyn, cast_n=n)
        if n:
            assert len(taken) == 1 and len(committed) == 1
            fig.equal(f"cast n={n} destination", torch.equal(dst.t.view(torch.int16), src.bfloat16().view(torch.int16)))
            fig.equal(f"cast n={n} padding", dst.untouched(), "(a write outside the destination)")
        bits = [AO.a32(t[k]).view(np.int32).copy() for t in tensors for k in "pmv"]
        if base is None:
            base = bits
        for a, b in zip(bits, base):
            fig.equal(f"cast n={n} adam outputs vs no cast", np.array_equal(a, b))
    fig.finish()


# ---------------------------------------------------------------------------- every instance
def test_every_instance_is_reached(hip):
    """adam_f32 and the six adam_multi instances each appear in the launch log."""
    fig = AO.Figures()
    seen = []
    with hip.launch_log() as log:
        p = torch.zeros(8, device=dev)
        hip.adam(p, torch.ones(8, device=dev), p.clone(), p.clone(), torch.ones((), dtype=torch.int32, device=dev),
                 1e-3, 0.9, 0.999, 1e-8, 0.0, inplace=False)
    seen += [r["name"] for r in log]
    for rows in (16, 32, 64):
        for dyn in (None, (1.0, 1e-3)):
            with hip.launch_log() as log:
                run(hip, fig, f"instances rows={rows} dyn={dyn is not None} fresh/wd=0.1", [spec((70, 128)), spec((33, 7))],
                    "fresh/wd=0.1", rows=rows, dyn=dyn)
            seen += [r["name"] for r in log if r["name"].startswith("adam")]
    assert seen == ["adam_f32", "adam_multi<16>", "adam_multi_dyn<16>", "adam_multi<32>", "adam_multi_dyn<32>",
                    "adam_multi<64>", "adam_multi_dyn<64>"], seen
    fig.finish()
