"""Time the MX-fp8 skinny GEMM of csrc/kernels/skinny_mx.hip on one MI355X against the bf16 skinny GEMM of the same
build on the same call.

    python scripts/skinny_mx_probe.py [--part shapes|generate|parent|all] [--parent TREE] [--out skinny_mx_probe.md]

``shapes``, at M = 1, 8 and 16 rows: the six projections of the decode model of ``decode_probe.py --part generate`` (dim
640, 8/2 heads, SwiGLU 1792, vocab 32768) and four byte-bound shapes a larger model would have (4096 -> 4096, 4096 ->
2 x 14336, 14336 -> 4096, 4096 -> 128256).  ``hip.skinny_mx`` on the MX quantisation of a weight against ``hip.skinny`` on
that weight, each with its own plan, timed as ``skinny_probe.py`` times its arms: HIP graphs over several operand sets
(a sweep moves ~600 MB of bf16 weight, at most 16 sets, at least 64 calls per graph), HIP events around ``--replays``
replays, the arms alternated three times, median (min..max).  Ratio: fp8 time over bf16 time; the byte ratio is (1 +
1/32) / 2 = 0.516.  TB/s: the bytes of weight each arm reads over its time.

``generate``: the decode model, B = 8, 128 + 128 tokens, captured, with and without ``weight_quant="mxfp8"``, alternating.

``parent`` (needs ``--parent``, the parent commit's tree built beside this one): the default paths, ``skinny_probe.py``'s
``generate`` and ``bench`` parts (default captured ``generate`` and ``python bench.py`` in both trees, alternating).

The ``shapes`` and ``generate`` parts run in this process: run them under ``timeout``.  Fails without a GPU."""
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
SHAPES = SP.SHAPES + [("4096->4096", 4096, 4096, 1, False), ("4096->2x14336", 4096, 14336, 2, False),
                      ("14336->4096 +res", 14336, 4096, 1, True), ("4096->128256", 4096, 128256, 1, False)]


def shapes_part(args, out):
    from learning_jax_sharding_amd.ops import fp8, hip
    from learning_jax_sharding_amd.ops.kernels import skinny_mx_reference
    side = torch.cuda.Stream()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    out.append(f"skinny_mx against skinny (bf16) of the same build, us per call, median (min..max) of {SP.ROUNDS} alternated "
               f"rounds, {cus} CUs")
    out.append("")
    out.append("| shape | M | plan mx / bf16 (waves x blocks) | skinny_mx us | skinny us | ratio | mx TB/s | bf16 TB/s | verdict |")
    out.append("|---|---|---|---|---|---|---|---|---|")
    for name, K, N, nw, has_res in SHAPES:
        NN = nw * N
        wbytes = NN * K * 2
        qbytes = NN * K + NN * K // 32
        nset = max(1, min(16, -(-600_000_000 // wbytes)))
        reps = max(1, -(-64 // nset))
        gen = torch.Generator().manual_seed(0)
        ws, qs, ss = [], [], []
        for _ in range(nset):
            w = (torch.randn(NN, K, generator=gen) * 0.05).to(BF16).cuda()
            q, s = fp8.quant_rows(w)                     # blocks along K of the [N][K] operand: the "QT" layout
            ws.append(w), qs.append(q), ss.append(s)
        for M in (1, 8, 16):
            xs = [torch.randn(M, K, generator=gen).to(BF16).cuda() for _ in range(nset)]
            rs = [torch.randn(M, N, generator=gen).to(BF16).cuda() if has_res else None for _ in range(nset)]
            o_q = [torch.empty(M, NN, dtype=BF16, device="cuda") for _ in range(nset)]
            o_b = [torch.empty(M, NN, dtype=BF16, device="cuda") for _ in range(nset)]

            def mx():
                for _ in range(reps):
                    for x, q, s, r, o in zip(xs, qs, ss, rs, o_q):
                        hip.skinny_mx(x, q, s, o, M, NN, K, K, NN, res=r, res_ld=N)

            def bf():
                for _ in range(reps):
                    for x, w, r, o in zip(xs, ws, rs, o_b):
                        hip.skinny(x, w, o, M, NN, K, K, NN, res=r, res_ld=N)

            with torch.cuda.stream(side), torch.no_grad():
                graphs = {"mx": SP._graph(mx, side), "bf16": SP._graph(bf, side)}
            torch.cuda.synchronize()
            if NN * K <= (1 << 24):      # the kernel against its torch statement on the first set (another summation order)
                want = skinny_mx_reference(xs[0], qs[0], ss[0], None, False, rs[0]).float()
                worst = float((o_q[0].float() - want).abs().max() / want.abs().max().clamp_min(1e-6))
                assert worst < 2.0 ** -6, (name, M, worst)
            t = SP._time(graphs, args.replays, nset * reps)
            a, b = t["mx"], t["bf16"]
            verdict = "faster" if a[2] < b[1] else ("SLOWER" if a[1] > b[2] else "ranges overlap")
            pm, pb = hip.skinny_mx_plan(M, NN, K, cus), hip.skinny_plan(M, NN, K, cus)
            out.append(f"| {name} | {M} | {pm[0]} x {pm[1]} / {pb[0]} x {pb[1]} | {SP._fmt(a)} | {SP._fmt(b)} | {a[0] / b[0]:.3f} | "
                       f"{qbytes / a[0] / 1e6:.2f} | {wbytes / b[0] / 1e6:.2f} | {verdict} |")
            print(out[-1], flush=True)
            del graphs
        del ws, qs, ss
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
    arms = {"bf16": None, "mxfp8": "mxfp8"}
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
                   f"({min(v):.1f}..{max(v):.1f}), {statistics.median(v) * 1e3 / N:.0f} us per token")
        print(out[-1], flush=True)
    out.append(f"first tokens equal: {bool(torch.equal(toks['bf16'][:, 0], toks['mxfp8'][:, 0]))}; fraction of all tokens "
               f"equal: {float((toks['bf16'] == toks['mxfp8']).float().mean()):.3f}")
    print(out[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="shapes", choices=("shapes", "generate", "parent", "all"))
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    os.environ.setdefault("LJS_PLATFORM", "gpu")
    os.environ.setdefault("LJS_NUM_DEVICES", "1")
    out = []
    try:
        # (the child processes first: this process opens the GPU only for its own parts)
        if args.part in ("parent", "all"):
            SP.generate_part(args, out)
            SP.bench_part(args, out)
        if args.part != "parent" and not torch.cuda.is_available():
            raise SystemExit("skinny_mx_probe needs a GPU")
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
