"""Time the W8A16 tile GEMM of csrc/kernels/gemm_w8.hip on one MI355X against the bf16 tile GEMMs of the same build.

    python scripts/gemm_w8_probe.py [--part shapes|generate|all] [--ms 64,512,4096,16384] [--out profiles/gemm_w8/probe.md]

``shapes``: M = 64 / 512 / 4096 / 16384 rows times (K -> N) = 640 -> 1536, 1792 -> 640, 640 -> 32768, 4096 -> 4096, 4096 ->
28672, 14336 -> 4096.  ``hip.gemm_w8`` on the "QT" quantisation of a weight against
  (a) ``hip.gemm`` on the bf16 weight at ``tile=1282``, the same tile geometry;
  (b) ``hip.gemm`` at its own ``pick_tile``, what runs today;
  (c) a dequantise-to-bf16 pass (torch: the e4m3 cast times the block scale) followed by (b), what a user without the
      kernel would do to get fp8-weight semantics.
Timed as ``skinny_mx_probe.py`` times its arms: HIP graphs (at least 8 calls per graph), HIP events around ``--replays``
replays, the arms alternated three times, median (min..max).  Ratios are gemm_w8 time over the arm's time.

``generate``: the decode model of ``skinny_mx_probe.py``, B = 8, 128 + 128 tokens, captured, with ``weight_quant`` None,
"mxfp8" and "mxfp8-all", alternating.

Run under ``timeout``.  Fails without a GPU."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import skinny_probe as SP  # noqa: E402

BF16 = torch.bfloat16
SHAPES = [(640, 1536), (1792, 640), (640, 32768), (4096, 4096), (4096, 28672), (14336, 4096)]


def shapes_part(args, out):
    from learning_jax_sharding_amd.ops import fp8, hip
    side = torch.cuda.Stream()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    out.append(f"gemm_w8 against the bf16 tile GEMMs of the same build, us per call, median (min..max) of {SP.ROUNDS} "
               f"alternated rounds, {cus} CUs; ratios: gemm_w8 over the arm (**bold**: gemm_w8 slower than (b))")
    out.append("")
    out.append("| K -> N | M | rows x blocks | gemm_w8 us | (a) tile 1282 us | (b) pick_tile us | (c) dequant + (b) us | /(a) | /(b) "
               "| /(c) |")
    out.append("|---|---|---|---|---|---|---|---|---|---|")
    gen = torch.Generator().manual_seed(0)
    for K, N in SHAPES:
        w = (torch.randn(N, K, generator=gen) * 0.05).to(BF16).cuda()
        q, s = fp8.quant_rows(w)                         # blocks along K of the [N][K] operand: the "QT" layout
        wd = torch.empty_like(w)
        for M in args.ms:
            reps = max(8, min(64, (1 << 33) // (M * N * K)))
            x = torch.randn(M, K, generator=gen).to(BF16).cuda()
            o = {n: torch.empty(M, N, dtype=BF16, device="cuda") for n in ("w8", "a", "b", "c")}

            def dequant():
                sc = (s.to(torch.int32) << 23).view(torch.float32).to(BF16)
                torch.mul(q.view(torch.float8_e4m3fn).to(BF16).view(N, K // 32, 32), sc[:, :, None], out=wd.view(N, K // 32, 32))

            arms = {
                "w8": lambda: [hip.gemm_w8(x, q, s, o["w8"], M, N, K, K, N) for _ in range(reps)],
                "a": lambda: [hip.gemm(x, w, o["a"], M, N, K, K, K, N, True, True, tile=1282) for _ in range(reps)],
                "b": lambda: [hip.gemm(x, w, o["b"], M, N, K, K, K, N, True, True) for _ in range(reps)],
                "c": lambda: [(dequant(), hip.gemm(x, wd, o["c"], M, N, K, K, K, N, True, True)) for _ in range(reps)],
            }
            with torch.cuda.stream(side), torch.no_grad():
                graphs = {n: SP._graph(f, side) for n, f in arms.items()}
            torch.cuda.synchronize()
            assert torch.equal(o["w8"], o["c"]) or float((o["w8"].float() - o["c"].float()).abs().max()) < 2.0 ** -6 * float(
                o["c"].float().abs().max()), (K, N, M)
            t = SP._time(graphs, args.replays, reps)
            r = {n: t["w8"][0] / t[n][0] for n in "abc"}
            rb = f"**{r['b']:.3f}**" if r["b"] > 1.0 else f"{r['b']:.3f}"
            pl = hip.gemm_w8_plan(M, N, K, cus)
            out.append(f"| {K} -> {N} | {M} | {pl[0]} x {pl[1]} | {SP._fmt(t['w8'])} | {SP._fmt(t['a'])} | {SP._fmt(t['b'])} | "
                       f"{SP._fmt(t['c'])} | {r['a']:.3f} | {rb} | {r['c']:.3f} |")
            print(out[-1], flush=True)
            del graphs, o
        del w, q, s, wd
        torch.cuda.empty_cache()


def generate_part(args, out):
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd.models import TransformerLM, generate
    B, P, N = 8, 128, 128
    model = TransformerLM(vocab_size=32768, dim=640, layers=4, heads=8, kv_heads=2, dim_head=64, norm="rms",
                          ff="swiglu", rope_theta=10000.0, causal=True)
    tok = torch.randint(0, 32768, (B, P), generator=torch.Generator().manual_seed(0))
    ids = ljs.device_put(tok.numpy())
    params = model.init(ljs.random.PRNGKey(1), ids)["params"]
    arms = {"bf16": None, "mxfp8": "mxfp8", "mxfp8-all": "mxfp8-all"}
    toks, ts = {}, {n: [] for n in arms}
    for n, wq in arms.items():                       # (shadows, captures' warm-up)
        toks[n] = generate(model, params, ids, N, capture=True, weight_quant=wq)
    torch.cuda.synchronize()
    for _ in range(SP.ROUNDS):
        for n, wq in arms.items():
            t0 = time.perf_counter()
            generate(model, params, ids, N, capture=True, weight_quant=wq)
            torch.cuda.synchronize()
            ts[n].append((time.perf_counter() - t0) * 1e3)
    out.append("")
    for n in arms:
        v = ts[n]
        out.append(f"generate B = {B}, {P} + {N} tokens, captured, weights {n}: {statistics.median(v):.1f} ms "
                   f"({min(v):.1f}..{max(v):.1f})")
        print(out[-1], flush=True)
    out.append(f"first tokens of mxfp8 equal bf16's: {bool(torch.equal(toks['bf16'][:, 0], toks['mxfp8'][:, 0]))}; fraction of "
               f"all tokens equal, mxfp8-all against mxfp8: {float((toks['mxfp8-all'] == toks['mxfp8']).float().mean()):.3f}")
    print(out[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="shapes", choices=("shapes", "generate", "all"))
    ap.add_argument("--ms", default="64,512,4096,16384", type=lambda v: [int(m) for m in v.split(",")])
    ap.add_argument("--replays", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    os.environ.setdefault("LJS_PLATFORM", "gpu")
    os.environ.setdefault("LJS_NUM_DEVICES", "1")
    if not torch.cuda.is_available():
        raise SystemExit("gemm_w8_probe needs a GPU")
    out = []
    try:
        if args.part in ("generate", "all"):
            generate_part(args, out)
        if args.part in ("shapes", "all"):
            shapes_part(args, out)
    finally:
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
