"""Time the chunked-prefill attention kernel on one MI355X, head dim 64 or 128.

    python scripts/chunk_probe.py [--quick] [--out-dir profiles/chunk]
    python scripts/chunk_probe.py --dim 128 [--quick] [--max-l 4096] [--out-dir profiles/chunk128]

``attn_chunk`` (and ``attn_chunk_q8`` on the same shapes) on T new positions over a cache already filled to L rows, against
the two things a caller could do without it, on the same GPU and the same build:

  (a) ``ceil(T / 64)`` ``attn_extend`` launches (each with its merge launch where the plan splits the key axis);
  (b) ``attn_fwd_lse(causal=True, q_offset=L)`` on the cache slice ``[:, :L + T]`` -- possible because the probe's lengths
      are uniform: the same FLOPs by the training kernel.

Shapes: heads / kv_heads 8/2 and 8/8, batch 1 / 8 / 64, T = 128 / 512 / 2048, L = 0 / 4096 / 32768; the capacity is L + T.
Each version is a HIP graph of one call, HIP events around enough replays to fill about 50 ms after a warm-up; the
versions alternate three times and the median is reported with its min..max.  Fails without a GPU.

``--dim 128`` (prefill128.hip; the probe sets ``LJS_ATTN_D128=1``) adds two comparisons: (c) what ran before the kernel,
``attn_chunk_reference`` on the GPU (where its S x cap f32 scores stay under 2^30 elements), and (d) the 64 kernel at equal
tokens and equal heads x head_dim (twice the heads), as TFLOP/s of live keys.  ``--max-l`` drops the longer caches.
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ROUNDS = 3
BF16 = torch.bfloat16


def _graph(fn, side):
    fn()
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side, capture_error_mode="relaxed"):
        keep = fn()
    return g, keep


def _once(g):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    g.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _time(graphs):
    """us per replay: median (min, max) of ROUNDS alternated windows of about 50 ms each."""
    reps = {}
    for n, g in graphs.items():
        _once(g)                                           # warm-up
        reps[n] = max(2, min(200, int(50.0 / max(_once(g), 1e-3))))
    res = {n: [] for n in graphs}
    for _ in range(ROUNDS):
        for n, g in graphs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps[n]):
                g.replay()
            b.record()
            b.synchronize()
            res[n].append(a.elapsed_time(b) * 1e3 / reps[n])
    return {n: (statistics.median(v), min(v), max(v)) for n, v in res.items()}


def _fmt(t):
    return f"{t[0]:.1f} ({t[1]:.1f}..{t[2]:.1f})"


def _ratio(x, base):
    r = x[0] / base[0]
    return f"**{r:.2f}**" if r > 1.0 else f"{r:.2f}"       # bold: attn_chunk is the slower one


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="B = 8 and T = 512 only")
    ap.add_argument("--out-dir", default=None)
    ap.add_argument("--dim", type=int, default=64, choices=(64, 128))
    ap.add_argument("--max-l", type=int, default=32768, help="skip caches already filled beyond this many rows")
    args = ap.parse_args()
    D, SCALE = args.dim, args.dim ** -0.5
    if D == 128:
        os.environ["LJS_ATTN_D128"] = "1"
    if not torch.cuda.is_available():
        raise SystemExit("chunk_probe needs a GPU")
    from learning_jax_sharding_amd.ops import hip, kernels
    side = torch.cuda.Stream()
    gen = torch.Generator(device="cuda").manual_seed(0)
    out = ["| H/Hkv | B | T | L | tile | attn_chunk us | TFLOP/s | (a) extend x ceil(T/64) us | chunk / (a) | (b) attn_fwd us | "
           "chunk / (b) | attn_chunk_q8 us | q8 / (a, mx8) | q8 / chunk |" + (" (c) reference us | chunk / (c) | (d) attn_chunk at 64, "
           "2H heads, us | its TFLOP/s |" if D == 128 else ""),
           "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|" + ("---|---|---|---|" if D == 128 else "")]
    for H, Hkv in ((8, 2), (8, 8)):
        for B in ((8,) if args.quick else (1, 8, 64)):
            for T in ((512,) if args.quick else (128, 512, 2048)):
                for L in (l for l in (0, 4096, 32768) if l <= args.max_l):
                    cap = L + T
                    q = torch.randn(B, T, H, D, device="cuda", generator=gen).to(BF16)
                    k = torch.randn(B, cap, Hkv, D, device="cuda", generator=gen).to(BF16)
                    v = torch.randn(B, cap, Hkv, D, device="cuda", generator=gen).to(BF16)
                    q8 = tuple(torch.empty(B, cap, Hkv, d, dtype=torch.uint8, device="cuda") for d in (D, D, D // 32, D // 32))
                    hip.kv_append_q8(k, v, *q8)                                         # (kc, vc, kcs, vcs): rows 0 .. cap - 1
                    lens = torch.full((B,), L, dtype=torch.int32).cuda()
                    starts = list(range(0, T, 64))
                    lens_c = [lens + c0 for c0 in starts]
                    ext = lambda f, bufs: [f(q[:, c0:c0 + 64], *bufs, lc, SCALE)        # noqa: E731
                                           for c0, lc in zip(starts, lens_c)]
                    with torch.cuda.stream(side):
                        graphs = {"chunk": _graph(lambda: hip.attn_chunk(q, k, v, lens, SCALE), side),
                                  "extend": _graph(lambda: ext(hip.attn_extend, (k, v)), side),
                                  "fwd": _graph(lambda: hip.attn_fwd_lse(q, k, v, SCALE, True, L), side),
                                  "chunk8": _graph(lambda: hip.attn_chunk_q8(q, *q8, lens, SCALE), side),
                                  "extend8": _graph(lambda: ext(hip.attn_extend_q8, q8), side)}
                        if D == 128:
                            # (d): the same tokens and the same heads x head_dim at 64 -- the buffers reinterpreted
                            q64, k64, v64 = (x.view(*x.shape[:2], -1, 64) for x in (q, k, v))
                            graphs["chunk64"] = _graph(lambda: hip.attn_chunk(q64, k64, v64, lens, 0.125), side)
                            if B * H * T * cap <= 2 ** 30:
                                graphs["ref"] = _graph(lambda: kernels.attn_chunk_reference(q, k, v, lens, SCALE), side)
                    t = _time({m: g[0] for m, g in graphs.items()})
                    flops = 4.0 * D * B * H * (T * L + T * (T + 1) / 2)                 # QK^T and PV over the live keys
                    rows = hip.plan_chunk(B, T, H, Hkv)[0]
                    out.append(f"| {H}/{Hkv} | {B} | {T} | {L} | R{rows} | {_fmt(t['chunk'])} | "
                               f"{flops / t['chunk'][0] * 1e-6:.1f} | {_fmt(t['extend'])} | {_ratio(t['chunk'], t['extend'])} | "
                               f"{_fmt(t['fwd'])} | {_ratio(t['chunk'], t['fwd'])} | {_fmt(t['chunk8'])} | "
                               f"{_ratio(t['chunk8'], t['extend8'])} | {t['chunk8'][0] / t['chunk'][0]:.2f} |")
                    if D == 128:
                        ref = f" {_fmt(t['ref'])} | {_ratio(t['chunk'], t['ref'])} |" if "ref" in t else " - | - |"
                        out[-1] += f"{ref} {_fmt(t['chunk64'])} | {flops / t['chunk64'][0] * 1e-6:.1f} |"
                    print(out[-1], flush=True)
                    del graphs, q, k, v, q8
                    torch.cuda.empty_cache()
    text = "\n".join(out) + "\n"
    if args.out_dir:
        os.makedirs(args.out_dir, exist_ok=True)
        with open(os.path.join(args.out_dir, "chunk_probe_quick.md" if args.quick else "chunk_probe.md"), "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
