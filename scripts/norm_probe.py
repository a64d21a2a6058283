"""Time nn.LayerNorm / nn.RMSNorm forward and backward on one MI355X: the fused HIP kernels
against the composite of elementwise / reduction ops (LJS_FUSED_NORM=0, same build).

    python scripts/norm_probe.py [--kind layer] [--shape 2048x640] [--replays 20] [--json out.json]

Each pass is captured into a HIP graph that runs it once over each of several input sets (enough
sets that one sweep moves ~600 MB, so a replay does not find its inputs in the 256 MB Infinity
Cache; capped at 16 sets, which the small shape's 8 MB passes still fit into - as they would
behind their producer).  A timing is HIP events around ``--replays`` replays after warm-up,
divided by replays x sets; the two paths alternate three times and the median is reported.
GB/s counts the bytes a pass must move (forward x + y; backward x + g + dx) and the floor is
those bytes at 6.3 TB/s.  Fails without a GPU.
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
SHAPES = [(16384, 640), (2048, 640)]
DTYPES = [(torch.float32, torch.bfloat16), (torch.bfloat16, torch.bfloat16)]
_NAME = {torch.float32: "f32", torch.bfloat16: "bf16"}


def _leaf(a):
    from learning_jax_sharding_amd.array import ShardedArray
    return ShardedArray(a.shape, a.dtype, a.sharding, {d: t.detach().clone().requires_grad_(True)
                                                       for d, t in a.local.items()})


def _local(a):
    return next(iter(a.local.values()))


class Pass:
    """Forward and backward graphs of one layer on one path over ``nset`` input sets."""

    def __init__(self, kind, R, D, xdt, ydt, fused, nset):
        import learning_jax_sharding_amd as ljs
        from learning_jax_sharding_amd import nn
        os.environ["LJS_FUSED_NORM"] = "1" if fused else "0"
        model = (nn.LayerNorm if kind == "layer" else nn.RMSNorm)(dtype=ydt)
        gen = torch.Generator().manual_seed(0)
        self.sets = []
        params = {"scale": _leaf(ljs.device_put((1.0 + 0.1 * torch.randn(D, generator=gen)).numpy()))}
        if kind == "layer":
            params["bias"] = _leaf(ljs.device_put((0.1 * torch.randn(D, generator=gen)).numpy()))
        for _ in range(nset):
            x = _leaf(ljs.device_put(torch.randn(R, D, generator=gen).numpy()).astype(xdt))
            g = torch.randn(R, D, generator=gen).to(ydt).cuda()
            self.sets.append((x, g))
        self.wrt_p = [_local(p) for p in params.values()]

        def fwd():
            return [model.apply({"params": params}, x) for x, _ in self.sets]

        # everything runs on ONE side stream: autograd issues a backward node on the stream its
        # forward ran on, and a launch on another stream while a capture is open is not part of it
        # (a first version, whose forward ran on the default stream, crashed inside the capture)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        self.graphs = {}
        from learning_jax_sharding_amd.ops import hip
        with torch.cuda.stream(side):
            with hip.launch_log() as log:
                ys = fwd()
            self.fwd_launches = [r["name"] for r in log if r["name"].startswith("norm_")]
            if fused != bool(self.fwd_launches):
                raise RuntimeError(f"expected the {'fused' if fused else 'composite'} path, saw {self.fwd_launches}")
            ylocs = [_local(y) for y in ys]

            def bwd():
                return [torch.autograd.grad(y, [_local(x)] + self.wrt_p, g, retain_graph=True)
                        for y, (x, g) in zip(ylocs, self.sets)]

            for name, fn in (("fwd", fwd), ("bwd", bwd)):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", default="layer", choices=["layer", "rms"])
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--shape", default="", help="RxD: this shape only (default: 16384x640 and 2048x640)")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("norm_probe: no GPU; a timing needs one")
    os.environ.setdefault("LJS_PLATFORM", "gpu")
    os.environ["LJS_NUM_DEVICES"] = "1"
    rows = []
    print(f"{'shape':>12} {'dtypes':>10} {'pass':>4} {'fused us':>9} {'GB/s':>7} {'composite us':>12} {'GB/s':>7} "
          f"{'ratio':>6} {'floor us':>8} {'fused/floor':>11}")
    shapes = [tuple(int(v) for v in a.shape.split("x"))] if a.shape else SHAPES
    for R, D in shapes:
        for xdt, ydt in DTYPES:
            bx, by = (2 if xdt == torch.bfloat16 else 4), (2 if ydt == torch.bfloat16 else 4)
            nbytes = {"fwd": R * D * (bx + by), "bwd": R * D * (bx + by + bx)}
            nset = max(2, min(16, math.ceil(600e6 / nbytes["bwd"])))
            t = {(p, f): [] for p in ("fwd", "bwd") for f in (True, False)}
            passes = {f: Pass(a.kind, R, D, xdt, ydt, f, nset) for f in (True, False)}
            for _ in range(3):              # the two paths alternate
                for f in (True, False):
                    for p in ("fwd", "bwd"):
                        t[(p, f)].append(passes[f].time_us(p, a.replays))
            del passes
            torch.cuda.empty_cache()
            for p in ("fwd", "bwd"):
                fu, co = statistics.median(t[(p, True)]), statistics.median(t[(p, False)])
                floor = nbytes[p] / PEAK_BPS * 1e6
                row = {"kind": a.kind, "R": R, "D": D, "x": _NAME[xdt], "y": _NAME[ydt], "pass": p, "sets": nset,
                       "fused_us": fu, "composite_us": co, "fused_all": t[(p, True)], "composite_all": t[(p, False)],
                       "bytes": nbytes[p], "fused_gbps": nbytes[p] / fu * 1e-3, "composite_gbps": nbytes[p] / co * 1e-3,
                       "ratio": co / fu, "floor_us": floor}
                rows.append(row)
                print(f"{f'{R}x{D}':>12} {_NAME[xdt] + '>' + _NAME[ydt]:>10} {p:>4} {fu:9.2f} {row['fused_gbps']:7.0f} "
                      f"{co:12.2f} {row['composite_gbps']:7.0f} {co / fu:6.1f} {floor:8.2f} {fu / floor:11.1f}",
                      flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
