"""Time the rotary embedding of Q and K on one MI355X, forward and forward + backward: the fused HIP
kernel (csrc/kernels/rope.hip) against the torch composite (ops/kernels.py rope_reference,
LJS_FUSED_ROPE=0, same build, same GPU).

    python scripts/rope_probe.py [--shape 32x512x8x64] [--replays 20] [--json out.json]

Q and K are column blocks 0 and 1 of a fused bf16 [B, S, 3, H, D] projection buffer, as a RoPE layer
hands them over.  Each pass is captured into a HIP graph that runs it once over each of several
input sets (enough sets that one sweep moves ~600 MB, so a replay does not find its inputs in the
256 MB Infinity Cache; capped at 16 sets).  A timing is HIP events around ``--replays`` replays after
warm-up, divided by replays x sets; the two paths alternate three times and the median is reported.
The byte floor is the bytes a pass must move (forward: Q and K read, Q' and K' written; the backward
the same again for the cotangents) at 6.3 TB/s.  Fails without a GPU.
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
SHAPES = [(32, 512, 8, 64), (4, 512, 8, 64)]   # B S = 16384 and 2048 tokens
THETA = 10000.0


class Pass:
    """Forward and forward + backward graphs of one path over ``nset`` input sets."""

    def __init__(self, B, S, H, D, fused, nset):
        from learning_jax_sharding_amd.ops import hip
        from learning_jax_sharding_amd.ops import kernels as K
        os.environ["LJS_FUSED_ROPE"] = "1" if fused else "0"
        gen = torch.Generator().manual_seed(0)
        self.sets = []
        for _ in range(nset):
            qkv = torch.randn(B, S, 3, H, D, generator=gen).to(torch.bfloat16).cuda()
            # leaves that are the column blocks themselves: the backward's result is their gradient
            # as it is, with no scatter into a buffer-shaped gradient on either path
            q, k = (qkv[:, :, i].detach().requires_grad_(True) for i in (0, 1))
            gq = torch.randn(B, S, H, D, generator=gen).to(torch.bfloat16).cuda()
            gk = torch.randn(B, S, H, D, generator=gen).to(torch.bfloat16).cuda()
            self.sets.append((q, k, gq, gk))

        def fwd():
            return [K.rope(q, k, 0, THETA) for q, k, _, _ in self.sets]

        def fwd_bwd():
            return [torch.autograd.grad(list(K.rope(q, k, 0, THETA)), [q, k], [gq, gk])
                    for q, k, gq, gk in self.sets]

        # everything on ONE side stream: autograd issues a backward node on its forward's stream
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        self.graphs = {}
        with torch.cuda.stream(side):
            with hip.launch_log() as log:
                fwd()
            launches = [r["name"] for r in log if r["name"].startswith("rope<")]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--shape", default="", help="BxSxHxD: this shape only (default: 32x512x8x64 and 4x512x8x64)")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rope_probe: no GPU; a timing needs one")
    rows = []
    print(f"{'shape':>14} {'pass':>8} {'fused us':>9} {'GB/s':>7} {'composite us':>12} {'GB/s':>7} {'ratio':>6} "
          f"{'floor us':>8} {'fused/floor':>11}")
    shapes = [tuple(int(v) for v in a.shape.split("x"))] if a.shape else SHAPES
    for B, S, H, D in shapes:
        one = 2 * 2 * B * S * H * D * 2                    # Q and K, read and written, bf16
        nbytes = {"fwd": one, "fwd+bwd": 2 * one}
        nset = max(2, min(16, math.ceil(600e6 / one)))
        t = {(p, f): [] for p in nbytes for f in (True, False)}
        passes = {f: Pass(B, S, H, D, f, nset) for f in (True, False)}
        for _ in range(3):                                 # the two paths alternate
            for f in (True, False):
                for p in nbytes:
                    t[(p, f)].append(passes[f].time_us(p, a.replays))
        del passes
        torch.cuda.empty_cache()
        for p in nbytes:
            fu, co = statistics.median(t[(p, True)]), statistics.median(t[(p, False)])
            floor = nbytes[p] / PEAK_BPS * 1e6
            row = {"B": B, "S": S, "H": H, "D": D, "pass": p, "sets": nset, "fused_us": fu, "composite_us": co,
                   "fused_all": t[(p, True)], "composite_all": t[(p, False)], "bytes": nbytes[p],
                   "fused_gbps": nbytes[p] / fu * 1e-3, "composite_gbps": nbytes[p] / co * 1e-3, "ratio": co / fu,
                   "floor_us": floor}
            rows.append(row)
            print(f"{f'{B}x{S}x{H}x{D}':>14} {p:>8} {fu:9.2f} {row['fused_gbps']:7.0f} {co:12.2f} "
                  f"{row['composite_gbps']:7.0f} {co / fu:6.1f} {floor:8.2f} {fu / floor:11.1f}", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
