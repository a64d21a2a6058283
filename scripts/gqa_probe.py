"""Time grouped-query attention on one MI355X, forward and forward + backward, in bf16 with head dim
64: the kernels' K/V head lookup plus ``gqa_reduce`` (csrc/kernels/attention.hip, gqa.hip) against

  * the multi-head kernels at ``kv_heads = heads`` (what the narrower K / V cost or save), and
  * the ``LJS_GQA_KERNELS=0`` composite: torch expands K / V to one head per query head, the multi-head
    kernels run, and autograd sums dK / dV over each group (same build, same GPU).

    python scripts/gqa_probe.py [--shape 64x256x8x2] [--replays 20] [--no-causal] [--json out.json]

A shape is batch x sequence x heads x kv_heads.  Each pass is captured into a HIP graph that runs it
once over each of several input sets (enough sets that one sweep moves ~600 MB, so a replay does not
find its inputs in the 256 MB Infinity Cache; capped at 16 sets).  A timing is HIP events around
``--replays`` replays after warm-up, divided by replays x sets; the three versions alternate five
times and the median is reported with the min..max spread.  The last column times ``gqa_reduce``
alone over the bytes it must move (dKx and dVx read, dK and dV written).  Fails without a GPU.
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

SHAPES = [(64, 256, 8, 2), (8, 256, 8, 2), (4, 4096, 8, 2), (64, 256, 8, 1)]
VERSIONS = ("gqa", "mha", "composite")
ROUNDS = 5


def _capture(fn, side):
    for _ in range(2):
        fn()
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.autograd.set_multithreading_enabled(False), \
            torch.cuda.graph(graph, stream=side, capture_error_mode="relaxed"):
        keep = fn()
    return graph, keep


class Pass:
    """Forward and forward + backward graphs of one version over ``nset`` input sets."""

    def __init__(self, B, S, H, Hkv, version, causal, nset):
        from learning_jax_sharding_amd.ops import hip
        os.environ["LJS_GQA_KERNELS"] = "0" if version == "composite" else "1"
        hk = H if version == "mha" else Hkv
        scale = 0.125
        gen = torch.Generator().manual_seed(0)

        def rnd(*shape):
            return torch.randn(*shape, generator=gen).to(torch.bfloat16).cuda()

        self.sets = [(rnd(B, S, H, 64).requires_grad_(True), rnd(B, S, hk, 64).requires_grad_(True),
                      rnd(B, S, hk, 64).requires_grad_(True), rnd(B, S, H, 64)) for _ in range(nset)]

        def fwd():
            return [hip.attention(q, k, v, scale, causal, 0) for q, k, v, _ in self.sets]

        def fwd_bwd():
            return [torch.autograd.grad(hip.attention(q, k, v, scale, causal, 0), [q, k, v], do)
                    for q, k, v, do in self.sets]

        # everything on ONE side stream: autograd issues a backward node on its forward's stream
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        self.graphs = {}
        with torch.cuda.stream(side):
            with hip.launch_log() as log:
                torch.autograd.grad(hip.attention(*self.sets[0][:3], scale, causal, 0), list(self.sets[0][:3]),
                                    self.sets[0][3])
            self.launches = [r["name"] for r in log]
            if (version == "gqa") != ("gqa_reduce" in self.launches):
                raise RuntimeError(f"version {version}: unexpected launches {self.launches}")
            for name, fn in (("fwd", fwd), ("fwd+bwd", fwd_bwd)):
                self.graphs[name] = _capture(fn, side)
            if version == "gqa":
                xs = [(rnd(B, S, H, 64), rnd(B, S, H, 64), torch.empty(B, S, Hkv, 64, dtype=torch.bfloat16, device="cuda"),
                       torch.empty(B, S, Hkv, 64, dtype=torch.bfloat16, device="cuda")) for _ in range(nset)]
                # (kept on the object: the graph holds the addresses, not the tensors, and a later
                # capture empties the allocator's cache of whatever was freed)
                self.reduce_sets = xs
                self.graphs["reduce"] = _capture(lambda: [hip.gqa_reduce(*x) for x in xs], side)
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


def _fmt(ts):
    return f"{statistics.median(ts):8.2f} ({min(ts):.2f}..{max(ts):.2f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--shape", default="", help="BxSxHxHkv: this shape only")
    ap.add_argument("--no-causal", action="store_true")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gqa_probe: no GPU; a timing needs one")
    causal = not a.no_causal
    shapes = [tuple(int(v) for v in a.shape.split("x"))] if a.shape else SHAPES
    rows = []
    print(f"times in us per pass, median (min..max) of {ROUNDS} alternated rounds; causal={causal}")
    print(f"{'shape':>14} {'pass':>8} {'gqa':>24} {'mha (kv=heads)':>24} {'composite':>24} {'comp/gqa':>8} "
          f"{'reduce us':>22} {'GB/s':>6}")
    for B, S, H, Hkv in shapes:
        per_set = 6 * B * S * H * 64 * 2
        nset = max(2, min(16, math.ceil(600e6 / per_set)))
        passes = {v: Pass(B, S, H, Hkv, v, causal, nset) for v in VERSIONS}
        t = {(p, v): [] for p in ("fwd", "fwd+bwd") for v in VERSIONS}
        red = []
        for _ in range(ROUNDS):                        # the versions alternate
            for v in VERSIONS:
                for p in ("fwd", "fwd+bwd"):
                    t[(p, v)].append(passes[v].time_us(p, a.replays))
            red.append(passes["gqa"].time_us("reduce", a.replays))
        launches = {v: passes[v].launches for v in VERSIONS}
        del passes
        torch.cuda.empty_cache()
        rbytes = 2 * B * S * (H + Hkv) * 64 * 2
        for p in ("fwd", "fwd+bwd"):
            med = {v: statistics.median(t[(p, v)]) for v in VERSIONS}
            rows.append({"B": B, "S": S, "H": H, "Hkv": Hkv, "pass": p, "sets": nset, "causal": causal,
                         **{f"{v}_us": med[v] for v in VERSIONS}, **{f"{v}_all": t[(p, v)] for v in VERSIONS},
                         "reduce_us": statistics.median(red), "reduce_all": red, "reduce_bytes": rbytes,
                         "launches": launches})
            tail = f"{_fmt(red):>22} {rbytes / statistics.median(red) * 1e-3:6.0f}" if p == "fwd+bwd" else ""
            print(f"{f'{B}x{S}x{H}/{Hkv}':>14} {p:>8} {_fmt(t[(p, 'gqa')]):>24} {_fmt(t[(p, 'mha')]):>24} "
                  f"{_fmt(t[(p, 'composite')]):>24} {med['composite'] / med['gqa']:8.2f} {tail}", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
