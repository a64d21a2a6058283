"""Time the SwiGLU activation on one MI355X, forward and forward + backward: the fused HIP kernels
(csrc/kernels/swiglu.hip) against the torch composite ``F.silu(g) * u`` with its autograd, same GPU.

    python scripts/swiglu_probe.py [--shape 16384x2560] [--replays 20] [--json out.json] [--launches out.txt]
                                   [--figures out.txt] [--no-timing]

g and u are the two column blocks of a fused bf16 [T][2F] projection buffer, as the gate / up dense
hands them over.  Each pass is captured into a HIP graph that runs it once over each of several input
sets (enough sets that one sweep moves ~600 MB, so a replay does not find its inputs in the 256 MB
Infinity Cache; capped at 16 sets).  A timing is HIP events around ``--replays`` replays after warm-up,
divided by replays x sets; the two paths alternate three times and the median is reported.  The byte
floor is the bytes a pass must move (forward: g and u read, h written, 3 arrays; backward: g, u and
dh read, dg and du written, 5 arrays) at 6.3 TB/s.  ``--launches`` writes the launch log of one
GatedFeedForward training step (the bench layer's 16384 x 640 -> 2560): which GEMM instances the gate /
up dense's backward runs behind the kernel's [dg|du] buffer, and behind the two tensors of the torch
formulation.  ``--figures`` writes the worst error figures of the kernels on 2.2M samples against the float64
oracle of tests/swiglu_oracle.py.  Fails without a GPU.
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_BPS = 6.3e12
SHAPES = [(16384, 2560), (2048, 2560)]   # tokens x ff_dim of the benchmark's layer


class Pass:
    """Forward and forward + backward graphs of one path over ``nset`` input sets."""

    def __init__(self, T, F, fused, nset):
        from learning_jax_sharding_amd.ops import hip
        from learning_jax_sharding_amd.ops import kernels as K
        gen = torch.Generator().manual_seed(0)
        self.sets = []
        for _ in range(nset):
            buf = torch.randn(T, 2 * F, generator=gen).to(torch.bfloat16).cuda()
            # leaves that are the column blocks themselves: the backward's result is their gradient
            # as it is, with no scatter into a buffer-shaped gradient on either path
            g, u = (buf[:, i * F:(i + 1) * F].detach().requires_grad_(True) for i in (0, 1))
            dh = torch.randn(T, F, generator=gen).to(torch.bfloat16).cuda()
            self.sets.append((g, u, dh))

        def act(g, u):
            return K.swiglu(g, u) if fused else torch.nn.functional.silu(g) * u

        def fwd():
            return [act(g, u) for g, u, _ in self.sets]

        def fwd_bwd():
            return [torch.autograd.grad(act(g, u), [g, u], dh) for g, u, dh in self.sets]

        # everything on ONE side stream: autograd issues a backward node on its forward's stream
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        self.graphs = {}
        with torch.cuda.stream(side):
            with hip.launch_log() as log:
                fwd()
            launches = [r["name"] for r in log if r["name"].startswith("swiglu")]
            if fused != bool(launches):
                raise RuntimeError(f"expected the {'fused' if fused else 'composite'} path, saw {launches}")
            for name, fn in (("fwd", fwd), ("fwd+bwd", fwd_bwd)):
                for _ in range(2):
                    fn()
                side.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.autograd.set_multithreading_enabled(False), \
                        torch.cuda.graph(graph, stream=side, capture_error_mode="relaxed"):
                    keep = fn()
                self.graphs[name] = (graph, keep)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.nset = nset

    def time_us(self, name, replays):
        graph, _ = self.graphs[name]
        for _ in range(3):
            graph.replay()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(replays):
            graph.replay()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / (replays * self.nset)


def ff_step_launches(path):
    """The launch log of one GatedFeedForward training step on one GPU device, in issue order: with the
    fused kernels ([dg|du] one buffer) and with LJS_FUSED_SWIGLU=0 (dg and du two tensors)."""
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd import nn
    from learning_jax_sharding_amd.ops import hip
    model = nn.GatedFeedForward(2560)
    x = ljs.random.normal(ljs.random.PRNGKey(0), (64, 256, 640))
    params = model.init(ljs.random.PRNGKey(1), x)["params"]

    def loss(p, xs):   # a cotangent that is a real [T][d] matrix, as inside a model (not the row of y.sum())
        y = model.apply({"params": p}, xs, residual=xs).astype(ljs.numpy.float32)
        return (y * y).sum()

    step = ljs.value_and_grad(loss, argnums=(0, 1))
    keys = ("name", "grid", "block", "resolved_tile", "splitk", "variant")
    out = []
    # which branch of ops/linear.py _wgrads each weight gradient took: _dw_slabs with its column count
    # (2 F: the batched launch over adjacent cotangents) or _dw_slabs_wmajor (separate cotangents)
    from learning_jax_sharding_amd.ops import linear
    branches, real = [], (linear._dw_slabs, linear._dw_slabs_wmajor)
    linear._dw_slabs = lambda *a, **k: (branches.append(f"_dw_slabs(columns={a[5]})"), real[0](*a, **k))[1]
    linear._dw_slabs_wmajor = lambda *a, **k: (branches.append("_dw_slabs_wmajor"), real[1](*a, **k))[1]
    try:
        for fused in ("1", "0"):
            os.environ["LJS_FUSED_SWIGLU"] = fused
            step(params, x)
            del branches[:]
            with hip.launch_log() as log:
                step(params, x)
            torch.cuda.synchronize()
            out.append(f"GatedFeedForward(2560) step, x (64, 256, 640), LJS_FUSED_SWIGLU={fused}: {log.total} "
                       "launches of the library (torch's own kernels are not in this log)")
            out += [" ".join(f"{k}={r.get(k)}" for k in keys if r.get(k) is not None) for r in log]
            out.append("weight-gradient branches, in order: " + ", ".join(branches))
    finally:
        linear._dw_slabs, linear._dw_slabs_wmajor = real
        os.environ.pop("LJS_FUSED_SWIGLU", None)
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")
    print("\n".join(out))


def figures(path, n=2_000_000):
    """Worst error figures of the kernels (and of the torch formulation on the host) against the float64
    oracle of tests/swiglu_oracle.py on n + 200000 samples: g ~ 4 N(0,1) clamped to +-80 plus linspaces
    over [-80, 80] and [-1.4, -1.1], u ~ 2 N(0,1), dh ~ N(0,1), |u| and |dh| kept in [2^-10, 8]."""
    import contextlib
    import io
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import swiglu_oracle as O
    from learning_jax_sharding_amd.ops import hip
    from learning_jax_sharding_amd.ops import kernels as K
    gen = torch.Generator().manual_seed(0)
    g = torch.cat([(4 * torch.randn(n, generator=gen)).clamp(-80, 80), torch.linspace(-80, 80, 100000),
                   torch.linspace(-1.4, -1.1, 100000)])

    def mag(scale):
        t = scale * torch.randn(g.numel(), generator=gen)
        return torch.where(t < 0, -1.0, 1.0) * t.abs().clamp(2.0 ** -10, 8.0)

    u, dh = mag(2.0), mag(1.0)
    g, u, dh = (t.view(1, -1, 8) for t in (g, u, dh))
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        for where in ("gpu", "host"):
            for idt in (torch.float32, torch.bfloat16):
                for odt in (torch.float32, torch.bfloat16):
                    dev = "cuda" if where == "gpu" else "cpu"
                    gs, us = (t.to(idt).to(dev).requires_grad_(True) for t in (g, u))
                    ds = dh.to(odt).to(dev)
                    with hip.launch_log() as log:
                        h = K.swiglu(gs, us, odt)
                        dg, du = torch.autograd.grad(h, [gs, us], ds)
                    ran = [r["name"] for r in log if r["name"].startswith("swiglu")]
                    if (len(ran) == 2) != (where == "gpu"):
                        raise RuntimeError(f"{where}: saw the launches {ran}")
                    tag = f"{where} {str(idt)[6:]}->{str(odt)[6:]} n={g.numel()}"
                    dg64, mdg, du64, mdu = O.backward64(gs, us, ds)
                    O.check(f"{tag} h", h, *O.forward64(gs, us), O.U_H)
                    O.check(f"{tag} dg", dg, dg64, mdg, O.U_DG)
                    O.check(f"{tag} du", du, du64, mdu, O.U_DU)
    with open(path, "w") as f:
        f.write(buf.getvalue())
    print(buf.getvalue(), end="")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--shape", default="", help="TxF: this shape only (default: 16384x2560 and 2048x2560)")
    ap.add_argument("--json", default="")
    ap.add_argument("--launches", default="", help="write the launch log of one GatedFeedForward step here")
    ap.add_argument("--figures", default="", help="write the kernels' worst error figures against the oracle here")
    ap.add_argument("--no-timing", action="store_true", help="skip the timing table")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("swiglu_probe: no GPU; a timing needs one")
    os.environ.setdefault("LJS_PLATFORM", "gpu")
    os.environ.setdefault("LJS_NUM_DEVICES", "1")
    rows = []
    print(f"{'shape':>12} {'pass':>8} {'fused us':>9} {'GB/s':>7} {'composite us':>12} {'GB/s':>7} {'ratio':>6} "
          f"{'floor us':>8} {'fused/floor':>11}")
    shapes = [tuple(int(v) for v in a.shape.split("x"))] if a.shape else SHAPES
    for T, F in ([] if a.no_timing else shapes):
        arr = T * F * 2                                     # one bf16 [T][F] array
        nbytes = {"fwd": 3 * arr, "fwd+bwd": 8 * arr}
        nset = max(2, min(16, math.ceil(600e6 / (3 * arr))))
        t = {(p, f): [] for p in nbytes for f in (True, False)}
        passes = {f: Pass(T, F, f, nset) for f in (True, False)}
        for _ in range(3):                                  # the two paths alternate
            for f in (True, False):
                for p in nbytes:
                    t[(p, f)].append(passes[f].time_us(p, a.replays))
        del passes
        torch.cuda.empty_cache()
        for p in nbytes:
            fu, co = statistics.median(t[(p, True)]), statistics.median(t[(p, False)])
            floor = nbytes[p] / PEAK_BPS * 1e6
            row = {"T": T, "F": F, "pass": p, "sets": nset, "fused_us": fu, "composite_us": co,
                   "fused_all": t[(p, True)], "composite_all": t[(p, False)], "bytes": nbytes[p],
                   "fused_gbps": nbytes[p] / fu * 1e-3, "composite_gbps": nbytes[p] / co * 1e-3, "ratio": co / fu,
                   "floor_us": floor}
            rows.append(row)
            print(f"{f'{T}x{F}':>12} {p:>8} {fu:9.2f} {row['fused_gbps']:7.0f} {co:12.2f} "
                  f"{row['composite_gbps']:7.0f} {co / fu:6.1f} {floor:8.2f} {fu / floor:11.1f}", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)
    if a.launches:
        ff_step_launches(a.launches)
    if a.figures:
        figures(a.figures)


if __name__ == "__main__":
    main()
