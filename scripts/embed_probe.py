"""Time the fused embedding kernels (csrc/kernels/embed.hip, through ops.hip) against torch's
F.embedding + .to(bf16) and its backward on the same MI355X, in the same process.

    python scripts/embed_probe.py [--shape 16384x50257x640] [--replays 20] [--json out.json] [--index-sweep]

Table f32, output and dY bf16, ids int64, uniform and Zipf(1.0) from a fixed seed.  Each timed piece
is captured into a HIP graph (a piece torch cannot capture is timed eagerly and marked ``*``); a
timing is HIP events around ``--replays`` replays after warm-up, the paths alternate three times
and the median is reported.  The launch log is checked: the fused pieces ran the embed_ kernels,
the torch pieces none.  Backward pieces of the fused path: ``index`` (embed_rank + embed_scan +
embed_fill, or the torch.sort route above EMBED_ALLPAIRS_MAX_TOKENS), ``sum`` (embed_bwd and, when a
list can be longer than EMBED_CHUNK, embed_combine).  The floor is the bytes a pass must move at
6.3 TB/s: forward T D (4 + 2), backward T D 2 + V D 4.  ``--index-sweep`` times the all-pairs index
against the torch.sort route at several token counts (the choice of the cap).  Fails without a GPU.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_BPS = 6.3e12
SHAPES = [(16384, 50257, 640), (16384, 32768, 640), (2048, 50257, 640)]
BF16 = torch.bfloat16


def make_ids(T, V, dist, dev):
    gen = torch.Generator().manual_seed(1234)
    if dist == "uniform":
        ids = torch.randint(0, V, (T,), generator=gen)
    else:   # Zipf(1.0): p(rank r) ~ 1 / r, ranks dealt to ids by a fixed permutation
        p = 1.0 / torch.arange(1, V + 1, dtype=torch.float64)
        ranks = torch.multinomial(p / p.sum(), T, replacement=True, generator=gen)
        ids = torch.randperm(V, generator=gen)[ranks]
    return ids.to(dev)


class Piece:
    """One timed callable: captured into a graph on a side stream if torch allows, else eager."""

    def __init__(self, fn, fused, hip):
        self.fn, self.graph, self.keep = fn, None, None
        self.side = torch.cuda.Stream()
        self.side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self.side):
            with hip.launch_log() as log:
                fn()
            ran = [r["name"] for r in log if r["name"].startswith("embed_")]
            if fused != bool(ran):
                raise RuntimeError(f"expected the {'fused' if fused else 'torch'} path, saw {ran}")
            self.launches = ran
            fn()
            self.side.synchronize()
            try:
                graph = torch.cuda.CUDAGraph()
                with torch.autograd.set_multithreading_enabled(False), \
                        torch.cuda.graph(graph, stream=self.side, capture_error_mode="relaxed"):
                    self.keep = fn()
                self.graph = graph
            except Exception as e:   # a torch op that synchronises or allocates outside the pool
                self.why = str(e).splitlines()[0]
                torch.cuda.synchronize()
        torch.cuda.current_stream().wait_stream(self.side)
        torch.cuda.synchronize()

    def time_us(self, replays):
        run = self.graph.replay if self.graph is not None else self.fn
        with torch.cuda.stream(self.side):
            for _ in range(2):
                run()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(replays):
                run()
            b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / replays


def median_times(pieces, replays):
    t = {k: [] for k in pieces}
    for _ in range(3):   # the paths alternate
        for k, p in pieces.items():
            t[k].append(p.time_us(replays))
    return {k: statistics.median(v) for k, v in t.items()}


def probe_shape(hip, T, V, D, dist, replays):
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    table = torch.randn(V, D, generator=gen, device=dev).requires_grad_(True)
    dy = torch.randn(T, D, generator=gen, device=dev).to(BF16)
    ids = make_ids(T, V, dist, dev)
    counts = torch.bincount(ids, minlength=V)
    start, lst, work, cap = hip._embed_index(ids, 0, V)
    partial = torch.empty((max(cap, 1), D), dtype=torch.float32, device=dev)
    out = torch.empty((V, D), dtype=torch.float32, device=dev)

    def fused_sum():
        hip._ck(hip.lib().ljs_embed_bwd(hip._p(dy), 1, T, D, V, hip._p(start), hip._p(lst), hip._p(work), cap,
                                        hip._p(partial), hip._p(out), hip._stream(dy)), "embed_bwd")

    def torch_fwd():
        with torch.no_grad():
            return F.embedding(ids, table).to(BF16)

    def torch_fwd_bwd():
        return torch.autograd.grad(F.embedding(ids, table).to(BF16), table, dy)

    def fused_fwd():
        with torch.no_grad():
            return hip.embed(table, ids, 0, BF16)

    pieces = {
        "fused fwd": Piece(fused_fwd, True, hip),
        "torch fwd": Piece(torch_fwd, False, hip),
        "fused bwd": Piece(lambda: hip.embed_grad(dy, ids, V), True, hip),
        "fused bwd index": Piece(lambda: hip._embed_index(ids, 0, V), True, hip),
        "fused bwd sum": Piece(fused_sum, True, hip),
        "torch bwd": Piece(lambda: torch.ops.aten.embedding_dense_backward(dy.float(), ids, V, -1, False), False, hip),
        "torch fwd+bwd": Piece(torch_fwd_bwd, False, hip),
    }
    us = median_times(pieces, replays)
    eager = sorted(k for k, p in pieces.items() if p.graph is None)
    floor = {"fwd": T * D * (4 + 2) / PEAK_BPS * 1e6, "bwd": (T * D * 2 + V * D * 4) / PEAK_BPS * 1e6}
    return {"T": T, "V": V, "D": D, "ids": dist, "us": us, "eager": eager, "floor_us": floor,
            "max_list": int(counts.max()), "rows_chosen": int((counts > 0).sum()), "work_cap": cap,
            "chunk": hip.EMBED_CHUNK, "launches": pieces["fused bwd"].launches}


def index_sweep(hip, replays):
    """The all-pairs index (forced) against the torch.sort route (forced) at several token counts."""
    dev = torch.device("cuda", 0)
    V, rows = 50257, []
    L = hip.lib()
    real = L.ljs_embed_allpairs_max_tokens
    for T in (4096, 8192, 16384, 32768, 65536):
        ids = make_ids(T, V, "zipf", dev)
        row = {"T": T}
        for route, cap_tokens in (("all-pairs", 1 << 30), ("torch.sort", 0)):
            L.ljs_embed_allpairs_max_tokens = lambda c=cap_tokens: c
            try:
                p = Piece(lambda: hip._embed_index(ids, 0, V), True, hip)
                row[route] = statistics.median(p.time_us(replays) for _ in range(3))
                row[route + " eager"] = p.graph is None
            finally:
                L.ljs_embed_allpairs_max_tokens = real
        rows.append(row)
        print(f"index T={T:6d}  all-pairs {row['all-pairs']:8.1f} us   torch.sort route {row['torch.sort']:8.1f} us"
              f"{' *' if row['torch.sort eager'] else ''}", flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--shape", default="", help="TxVxD, this shape only (default: the three of SHAPES)")
    ap.add_argument("--json", default="")
    ap.add_argument("--index-sweep", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("embed_probe: no GPU; a timing needs one")
    from learning_jax_sharding_amd.ops import hip
    hip.lib()
    shapes = [tuple(int(v) for v in a.shape.split("x"))] if a.shape else SHAPES
    print(f"EMBED_CHUNK={hip.EMBED_CHUNK} EMBED_ALLPAIRS_MAX_TOKENS={hip.EMBED_ALLPAIRS_MAX_TOKENS}")
    rows = []
    for T, V, D in shapes:
        per = {}
        for dist in ("uniform", "zipf"):
            r = per[dist] = probe_shape(hip, T, V, D, dist, a.replays)
            rows.append(r)
            u, fl = r["us"], r["floor_us"]
            star = {k: ("*" if k in r["eager"] else "") for k in u}
            print(f"{T}x{V}x{D} {dist:8s} max list {r['max_list']:5d}, {r['rows_chosen']:5d} rows chosen\n"
                  f"   fwd   fused {u['fused fwd']:8.1f} us   torch {u['torch fwd']:8.1f}{star['torch fwd']} us   "
                  f"torch/fused {u['torch fwd'] / u['fused fwd']:5.2f}   floor {fl['fwd']:6.1f} us\n"
                  f"   bwd   fused {u['fused bwd']:8.1f} us (index {u['fused bwd index']:.1f} + sum "
                  f"{u['fused bwd sum']:.1f})   torch {u['torch bwd']:8.1f}{star['torch bwd']} us (fwd+bwd "
                  f"{u['torch fwd+bwd']:.1f}{star['torch fwd+bwd']})   torch/fused "
                  f"{u['torch bwd'] / u['fused bwd']:5.2f}   floor {fl['bwd']:6.1f} us", flush=True)
        print(f"   skewed / uniform: fused bwd {per['zipf']['us']['fused bwd'] / per['uniform']['us']['fused bwd']:.2f}, "
              f"sum pass {per['zipf']['us']['fused bwd sum'] / per['uniform']['us']['fused bwd sum']:.2f}, "
              f"torch bwd {per['zipf']['us']['torch bwd'] / per['uniform']['us']['torch bwd']:.2f}", flush=True)
        torch.cuda.empty_cache()
    out = {"shapes": rows}
    if a.index_sweep:
        out["index_sweep"] = index_sweep(hip, a.replays)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
