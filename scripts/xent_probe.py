"""Time the fused softmax cross-entropy kernels (csrc/kernels/xent.hip, through ops.hip.xent)
against torch's F.cross_entropy on the same MI355X, forward and forward + backward.

    python scripts/xent_probe.py [--shape 16384x32768:bf16] [--replays 10] [--json out.json]

Each pass is captured into a HIP graph that runs it once over each of several input sets (enough
sets that one sweep reads ~600 MB of logits, so a replay does not find its inputs in the 256 MB
Infinity Cache; at least 2).  A timing is HIP events around ``--replays`` replays after warm-up,
divided by replays x sets; the two paths alternate three times and the median is reported.
TB/s counts the bytes a pass must move: the forward reads the logits once (R V esize), the backward
reads them and writes dx once each, so forward + backward is 3 R V esize; the floor is those bytes
at 6.3 TB/s.  torch is given the logits in their own dtype (for bf16 that is its cheapest form:
no f32 copy of the logits is made first).  Fails without a GPU.
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_BPS = 6.3e12
SHAPES = [(16384, 32768, "bf16"), (16384, 50257, "f32"), (2048, 32768, "bf16")]
_DT = {"f32": torch.float32, "bf16": torch.bfloat16}


class Pass:
    """Forward and forward + backward graphs of one path over ``nset`` input sets."""

    def __init__(self, R, V, dtype, fused, nset):
        from learning_jax_sharding_amd.ops import hip
        dev = torch.device("cuda", 0)
        gen = torch.Generator(device=dev).manual_seed(0)
        self.sets = []
        for _ in range(nset):
            x = (1.5 * torch.randn(R, V, generator=gen, device=dev)).to(dtype).requires_grad_(True)
            lab = torch.randint(0, V, (R,), generator=gen, device=dev)
            lab[::97] = -1
            g = torch.randn(R, generator=gen, device=dev)
            self.sets.append((x, lab, g))
        if fused:
            fn = hip.xent
        else:
            def fn(x, lab):
                return F.cross_entropy(x, lab, reduction="none", ignore_index=-1)

        def fwd():
            with torch.no_grad():
                return [fn(x, lab) for x, lab, _ in self.sets]

        def fwd_bwd():
            out = []
            for x, lab, g in self.sets:
                loss = fn(x, lab)
                out.append(torch.autograd.grad(loss, x, g.to(loss.dtype)))
            return out

        # everything on ONE side stream: autograd issues a backward node on the stream its forward
        # ran on, and a launch on another stream while a capture is open is not part of it
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        self.graphs = {}
        with torch.cuda.stream(side):
            with hip.launch_log() as log:
                fwd_bwd()
            ran = [r["name"] for r in log if r["name"].startswith("xent_")]
            if fused != bool(ran):
                raise RuntimeError(f"expected the {'fused' if fused else 'torch'} path, saw {ran}")
            self.launches = sorted(set(ran))
            for name, f in (("fwd", fwd), ("fwd+bwd", fwd_bwd)):
                f()
                side.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.autograd.set_multithreading_enabled(False), \
                        torch.cuda.graph(graph, stream=side, capture_error_mode="relaxed"):
                    keep = f()
                self.graphs[name] = (graph, keep)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.nset = nset

    def time_us(self, name, replays):
        graph, _ = self.graphs[name]
        for _ in range(2):
            graph.replay()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(replays):
            graph.replay()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / (replays * self.nset)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=10)
    ap.add_argument("--shape", default="", help="RxV:dtype, this shape only (default: the three of the docstring)")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("xent_probe: no GPU; a timing needs one")
    shapes = SHAPES
    if a.shape:
        rv, dt = a.shape.split(":")
        shapes = [tuple(int(v) for v in rv.split("x")) + (dt,)]
    rows = []
    print(f"{'shape':>14} {'dtype':>5} {'pass':>8} {'fused us':>9} {'TB/s':>6} {'torch us':>9} {'TB/s':>6} {'ratio':>6} "
          f"{'floor us':>8} {'fused/floor':>11}")
    for R, V, dt in shapes:
        esize = 2 if dt == "bf16" else 4
        nbytes = {"fwd": R * V * esize, "fwd+bwd": 3 * R * V * esize}
        nset = max(2, math.ceil(600e6 / nbytes["fwd"]))
        t = {(p, f): [] for p in nbytes for f in (True, False)}
        passes = {f: Pass(R, V, _DT[dt], f, nset) for f in (True, False)}
        for _ in range(3):                  # the two paths alternate
            for f in (True, False):
                for p in nbytes:
                    t[(p, f)].append(passes[f].time_us(p, a.replays))
        launches = passes[True].launches
        del passes
        torch.cuda.empty_cache()
        for p in nbytes:
            fu, to = statistics.median(t[(p, True)]), statistics.median(t[(p, False)])
            floor = nbytes[p] / PEAK_BPS * 1e6
            row = {"R": R, "V": V, "dtype": dt, "pass": p, "sets": nset, "fused_us": fu, "torch_us": to,
                   "fused_all": t[(p, True)], "torch_all": t[(p, False)], "bytes": nbytes[p],
                   "fused_tbps": nbytes[p] / fu * 1e-6, "torch_tbps": nbytes[p] / to * 1e-6, "ratio": to / fu,
                   "floor_us": floor, "launches": launches}
            rows.append(row)
            print(f"{f'{R}x{V}':>14} {dt:>5} {p:>8} {fu:9.1f} {row['fused_tbps']:6.2f} {to:9.1f} {row['torch_tbps']:6.2f} "
                  f"{to / fu:6.2f} {floor:8.1f} {fu / floor:11.2f}", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
