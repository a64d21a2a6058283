"""Time the skinny GEMM of csrc/kernels/skinny.hip on one MI355X against what the dense layers launched
before it, bf16.

    python scripts/skinny_probe.py [--part shapes|generate|bench|all] [--parent TREE] [--out skinny_probe.md]

``shapes``: the projections of the decode model of ``decode_probe.py --part generate`` (dim 640, 8/2 heads,
SwiGLU 1792, vocab 32768) at M = 1, 8 and 16 rows:

    640 -> 512 (Q), 640 -> 2 x 128 fused (K | V), 512 -> 640 + residual (out), 640 -> 2 x 1792 fused (gate | up),
    1792 -> 640 + residual (down), 640 -> 32768 (head)

``hip.skinny`` with its own plan against ``hip.gemm`` with the launcher's own pick on the same operands (the
call ``ops.linear`` makes with grad enabled, and made for every decode step before; at M = 1 that call is
timed on one row, without the padded copies the dense layer used to make around it).  Every timing is a
HIP graph that runs the call over each of several operand sets (enough that a sweep moves ~600 MB,
capped at 16: a 42 MB head weight comes from HBM every time, a 0.3-4.6 MB projection from the 256 MB
Infinity Cache at best, as in a decode step whose whole model is 76 MB), at least 64 calls per graph, HIP
events around ``--replays`` replays, divided by the calls; the arms alternate three times and the median is
reported with its min..max.  A call's time includes its kernel boundary.  Floor: the weight bytes over
8 TB/s (the HBM peak in MI355X_MICROARCH.md); TB/s: the weight bytes over the skinny call's time.

``generate`` (needs ``--parent``, the parent commit's tree built beside this one): ``decode_probe.py --part
generate`` in this tree and in the parent's, alternating, three pairs, one process each under its own time
limit: ms per captured call, us per token, launches per step.

``bench`` (needs ``--parent``): ``python bench.py`` and ``--batch-per-gpu 8`` in both trees, alternating, three
pairs.

The ``generate`` and ``bench`` parts run every GPU step as a child process under its own time limit.  The
``shapes`` part runs in this process and has none of its own: run it under ``timeout`` (a few minutes are
ample).  Fails without a GPU."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12
ROUNDS = 3
BF16 = torch.bfloat16
# (name, K, N per weight, weights, residual)
SHAPES = [("Q 640->512", 640, 512, 1, False), ("K|V 640->2x128", 640, 128, 2, False),
          ("out 512->640 +res", 512, 640, 1, True), ("gate|up 640->2x1792", 640, 1792, 2, False),
          ("down 1792->640 +res", 1792, 640, 1, True), ("head 640->32768", 640, 32768, 1, False)]


def _graph(fn, side):
    for _ in range(2):
        fn()
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side, capture_error_mode="relaxed"):
        fn()
    return g


def _time(graphs, replays, per):
    """{name: (median, min, max) us per call} of graphs {name: graph}, alternated ROUNDS times."""
    res = {n: [] for n in graphs}
    for g in graphs.values():
        g.replay()
    torch.cuda.synchronize()
    for _ in range(ROUNDS):
        for n, g in graphs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(replays):
                g.replay()
            b.record()
            b.synchronize()
            res[n].append(a.elapsed_time(b) * 1e3 / (replays * per))
    return {n: (statistics.median(v), min(v), max(v)) for n, v in res.items()}


def _fmt(t):
    return f"{t[0]:.2f} ({t[1]:.2f}..{t[2]:.2f})"


def shapes_part(args, out):
    from learning_jax_sharding_amd.ops import hip
    side = torch.cuda.Stream()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    out.append(f"skinny against the tile GEMM the launcher picks, bf16, us per call, median (min..max) of {ROUNDS} "
               f"alternated rounds, {cus} CUs; floor: weight bytes over {HBM_BYTES_PER_S / 1e12:.0f} TB/s")
    out.append("")
    out.append("| shape | M | plan (waves x blocks) | skinny us | tile GEMM us | tile kernel | floor us | skinny TB/s | "
               "verdict |")
    out.append("|---|---|---|---|---|---|---|---|---|")
    for name, K, N, nw, has_res in SHAPES:
        wbytes = nw * N * K * 2
        nset = max(1, min(16, -(-600_000_000 // wbytes)))
        reps = max(1, -(-64 // nset))
        gen = torch.Generator().manual_seed(0)
        ws = [(torch.randn(nw * N, K, generator=gen) * 0.05).to(BF16).cuda() for _ in range(nset)]
        for M in (1, 8, 16):
            xs = [torch.randn(M, K, generator=gen).to(BF16).cuda() for _ in range(nset)]
            rs = [torch.randn(M, N, generator=gen).to(BF16).cuda() if has_res else None for _ in range(nset)]
            o_s = [torch.empty(M, nw * N, dtype=BF16, device="cuda") for _ in range(nset)]
            o_g = [torch.empty(M, nw * N, dtype=BF16, device="cuda") for _ in range(nset)]

            def skinny():
                for _ in range(reps):
                    for x, w, r, o in zip(xs, ws, rs, o_s):
                        hip.skinny(x, w, o, M, nw * N, K, K, nw * N, res=r, res_ld=N)

            def tile():
                for _ in range(reps):
                    for x, w, r, o in zip(xs, ws, rs, o_g):
                        hip.gemm(x, w, o, M, N, K, K, K, nw * N, True, True, batch=nw, sA=0, sB=N * K if nw > 1 else 0,
                                 sC=N, res=r, res_ld=N)

            with torch.cuda.stream(side), torch.no_grad():
                with hip.launch_log() as log:
                    tile()
                tile_name = log[-1]["name"]
                graphs = {"skinny": _graph(skinny, side), "tile": _graph(tile, side)}
            torch.cuda.synchronize()
            # the two arms computed the same thing (another summation order: bf16 outputs within 2 ulp of each other's size)
            worst = max(float((a.float() - b.float()).abs().max() / b.float().abs().max().clamp_min(1e-6))
                        for a, b in zip(o_s, o_g))
            assert worst < 2.0 ** -6, (name, M, worst)
            t = _time(graphs, args.replays, nset * reps)
            s, g = t["skinny"], t["tile"]
            verdict = "faster" if s[2] < g[1] else ("slower" if s[1] > g[2] else "ranges overlap")
            floor = wbytes / HBM_BYTES_PER_S * 1e6
            waves, blocks = hip.skinny_plan(M, nw * N, K, cus)
            out.append(f"| {name} | {M} | {waves} x {blocks} | {_fmt(s)} | {_fmt(g)} | `{tile_name}` | {floor:.2f} | "
                       f"{wbytes / s[0] / 1e6:.2f} | {verdict} |")
            print(out[-1], flush=True)
            del graphs
        del ws
        torch.cuda.empty_cache()


def _run(cmd, cwd, limit, env=None):
    """One child process under its own time limit; anything but a clean exit ends the probe."""
    e = dict(os.environ, **(env or {}))
    e.pop("LJS_KERNELS_LIB", None)
    r = subprocess.run(cmd, cwd=cwd, env=e, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)} in {cwd} exited {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return r.stdout


def _trees(args):
    if not args.parent or not os.path.isdir(args.parent):
        raise SystemExit("this part needs --parent: the parent commit's tree, built")
    return (("this", ROOT), ("parent", os.path.abspath(args.parent)))


def generate_part(args, out):
    trees = _trees(args)
    res = {n: [] for n, _ in trees}
    launches = {}
    out.append("")
    for rnd in range(ROUNDS):
        for name, tree in trees:
            text = _run([sys.executable, "scripts/decode_probe.py", "--part", "generate"], tree, 420)
            m = re.search(r"captured ([0-9.]+) \(([0-9.]+)\.\.([0-9.]+)\)", text)
            n = re.search(r"one decode step records (\d+) launches", text)
            res[name].append(tuple(float(v) for v in m.groups()))
            launches[name] = int(n.group(1))
            out.append(f"generate round={rnd + 1} tree={name} captured_ms={m.group(1)} ({m.group(2)}..{m.group(3)}) "
                       f"launches_per_step={n.group(1)}")
            print(out[-1], flush=True)
            if rnd == 0:
                out.append(f"  {name}: " + text[text.index("one decode step records"):].strip().splitlines()[0])
    out.append("")
    out.append("| tree | captured generate ms (median of the processes' medians, min..max over all) | us per token | "
               "launches per step |")
    out.append("|---|---|---|---|")
    for name, _ in trees:
        med = statistics.median(v[0] for v in res[name])
        lo, hi = min(v[1] for v in res[name]), max(v[2] for v in res[name])
        out.append(f"| {name} | {med:.1f} ({lo:.1f}..{hi:.1f}) | {med * 1e3 / 128:.0f} | {launches[name]} |")
        print(out[-1], flush=True)


def bench_part(args, out):
    trees = _trees(args)
    out.append("")
    res = {}
    for rnd in range(ROUNDS):
        for extra in ((), ("--batch-per-gpu", "8")):
            for name, tree in trees:
                text = _run([sys.executable, "bench.py", *extra], tree, 300)
                line = [l for l in text.splitlines() if l.startswith("{")][-1]
                rec = json.loads(line)
                ms = rec.get("ms_per_step", rec.get("step_ms"))
                res.setdefault((name, extra), []).append(ms)
                out.append(f"bench round={rnd + 1} tree={name} args='{' '.join(extra)}' ms_per_step={ms}")
                print(out[-1], flush=True)
    out.append("")
    for extra in ((), ("--batch-per-gpu", "8")):
        a, b = res[("this", extra)], res[("parent", extra)]
        overlap = min(a) <= max(b) and min(b) <= max(a)
        out.append(f"bench.py {' '.join(extra) or '(default)'}: this {min(a)}-{max(a)} ms, parent {min(b)}-{max(b)} ms, "
                   f"ranges {'overlap' if overlap else 'DO NOT overlap'}")
        print(out[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="shapes", choices=("shapes", "generate", "bench", "all"))
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    os.environ.setdefault("LJS_PLATFORM", "gpu")
    os.environ.setdefault("LJS_NUM_DEVICES", "1")
    out = []
    try:
        # (the child processes first: this process opens the GPU only for the shapes part)
        if args.part in ("generate", "all"):
            generate_part(args, out)
        if args.part in ("bench", "all"):
            bench_part(args, out)
        if args.part in ("shapes", "all"):
            if not torch.cuda.is_available():
                raise SystemExit("skinny_probe needs a GPU")
            shapes_part(args, out)
    finally:
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
