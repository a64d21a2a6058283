"""Time head_dim 128 attention on one MI355X, forward and forward + backward, bf16 and causal: the
HIP kernels of csrc/kernels/attention128.hip (``LJS_ATTN_D128=1``) against

  * ``torch``: the torch formulation the same ``kernels.attention`` call takes with the switch off,
  * ``sdpa``: ``F.scaled_dot_product_attention`` where this torch build runs it for bf16 on the GPU, and
  * ``d64``: the head_dim 64 kernels at equal heads x head_dim and tokens (twice the heads), the
    project's own yardstick; TFLOPS count 4 S^2 D (forward) and 10 S^2 D (backward) per head, halved
    under causal.

    python scripts/attn128_probe.py [--shape 8x2048x8x2] [--replays 10] [--json out.json]

A shape is batch x sequence x heads x kv_heads.  Each pass is captured into a HIP graph; a timing is
HIP events around ``--replays`` replays after warm-up; the versions alternate three times and the
median is reported with the min..max spread.  Fails without a GPU.
"""
import argparse
import json
import os
import statistics
import sys
import warnings

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = [(64, 256, 8, 8), (64, 256, 8, 2), (8, 2048, 8, 8), (8, 2048, 8, 2), (2, 8192, 8, 8), (2, 8192, 8, 2)]
VERSIONS = ("hip128", "torch", "sdpa", "d64")
ROUNDS = 3


class Pass:
    """Forward and forward + backward graphs of one version."""

    def __init__(self, B, S, H, Hkv, version):
        from learning_jax_sharding_amd.ops import hip, kernels
        os.environ["LJS_ATTN_D128"] = "1" if version == "hip128" else "0"
        D, mul = (64, 2) if version == "d64" else (128, 1)
        scale = D ** -0.5
        gen = torch.Generator().manual_seed(0)

        def rnd(h):
            return torch.randn(B, S, h, D, generator=gen).to(torch.bfloat16).cuda()

        q, k, v = (rnd(h).requires_grad_(True) for h in (mul * H, mul * Hkv, mul * Hkv))
        do = rnd(mul * H)
        if version == "sdpa":
            def attn():
                return F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2),
                                                      is_causal=True, scale=scale, enable_gqa=H != Hkv).transpose(1, 2)
        else:
            def attn():
                return kernels.attention(q, k, v, scale, True, 0)
        self.keep = (q, k, v, do)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        self.graphs = {}
        with torch.cuda.stream(side), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            with hip.launch_log() as log:
                torch.autograd.grad(attn(), [q, k, v], do)
            self.launches = [r["name"] for r in log]
            if (version == "hip128") != any(n.startswith("attn128") for n in self.launches):
                raise RuntimeError(f"version {version}: unexpected launches {self.launches}")
            for name, fn in (("fwd", attn), ("fwd+bwd", lambda: torch.autograd.grad(attn(), [q, k, v], do))):
                for _ in range(2):
                    fn()
                side.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.autograd.set_multithreading_enabled(False), \
                        torch.cuda.graph(graph, stream=side, capture_error_mode="relaxed"):
                    out = fn()
                self.graphs[name] = (graph, out)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()

    def time_ms(self, name, replays):
        graph, _ = self.graphs[name]
        graph.replay()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(replays):
            graph.replay()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / replays


def probe(shape, replays):
    B, S, H, Hkv = shape
    passes = {}
    for ver in VERSIONS:
        try:
            passes[ver] = Pass(B, S, H, Hkv, ver)
        except Exception as e:   # (sdpa: not every build runs it for these operands)
            print(f"# {shape} {ver}: not run ({type(e).__name__}: {str(e)[:100]})")
    times = {(ver, n): [] for ver in passes for n in ("fwd", "fwd+bwd")}
    for _ in range(ROUNDS):
        for ver, p in passes.items():
            for n in ("fwd", "fwd+bwd"):
                times[(ver, n)].append(p.time_ms(n, replays))
    row = {"shape": "x".join(map(str, shape))}
    flops = {"fwd": 4.0, "fwd+bwd": 14.0}
    for (ver, n), ts in times.items():
        med = statistics.median(ts)
        row[f"{ver} {n} ms"] = f"{med:.4f} ({min(ts):.4f}..{max(ts):.4f})"
        if ver in ("hip128", "d64"):
            row[f"{ver} {n} TFLOPS"] = round(flops[n] * B * H * S * S * 128 / 2 / (med * 1e-3) / 1e12, 1)
    for n in ("fwd", "fwd+bwd"):
        for base in ("torch", "sdpa"):
            if (base, n) in times and ("hip128", n) in times:
                row[f"{base}/hip128 {n}"] = round(statistics.median(times[(base, n)]) /
                                                  statistics.median(times[("hip128", n)]), 2)
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shape", action="append", help="BxSxHxHkv (repeatable); default: the six probed shapes")
    ap.add_argument("--replays", type=int, default=10)
    ap.add_argument("--json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("attn128_probe: no GPU")
    shapes = [tuple(int(t) for t in s.split("x")) for s in args.shape] if args.shape else SHAPES
    rows = [probe(s, args.replays) for s in shapes]
    for r in rows:
        print("| " + " | ".join(f"{k}: {v}" for k, v in r.items()) + " |")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
