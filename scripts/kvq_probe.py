"""Time the MX-fp8 KV cache against the bf16 cache of the same build on one MI355X, head dim 64.

    python scripts/kvq_probe.py [--part attn|append|generate|long|all] [--quick] [--out-dir profiles/kvq]

``attn``: ``attn_decode<..,mx8>`` against ``attn_decode`` at heads / kv_heads = 8/2 and 8/8, batch 1 / 8 / 64, 256 / 4096 /
32768 keys (the capacity is the length: the plan depends on the capacity): us per call and TB/s of the live bytes
(K + V rows, and their scales for the fp8 cache).

``append``: ``kv_append<rot,q,mx8>`` against ``kv_append<rot,q>``, 32 calls per graph.

``generate``: ``models.generate`` for dim 640, 4 layers, 8/2 heads, vocab 32768, batch 8, 128 prompt + 128 new tokens,
captured, with and without ``cache_quant="mxfp8"``; the fraction of equal tokens.

``long``: the same model at batch 64 on a cache of 4096 rows filled to 4000: captured decode steps, ms per step.

Kernel timings are HIP graphs that run the call once over each of several input sets (enough sets that a sweep moves
~600 MB, capped at 16), HIP events around ``--replays`` replays after a warm-up; the versions alternate three times and
the median is reported with its min..max.  ``--part all`` runs every part as a fresh child process under a time limit
of its own and stops at the first one that fails; this process never opens the GPU.  Fails without a GPU.
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ROUNDS = 3
SCALE = 0.125
PARTS = {"attn": 420, "append": 120, "generate": 300, "long": 300}     # seconds a part may take
BF16, U8 = torch.bfloat16, torch.uint8


def _graph(fn, side):
    for _ in range(2):
        fn()
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side, capture_error_mode="relaxed"):
        keep = fn()
    return g, keep


def _time(graphs, replays, per):
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
    return f"{t[0]:.1f} ({t[1]:.1f}..{t[2]:.1f})"


def _q8_cache(B, n, Hkv, gen):
    """Random finite e4m3 bytes and scales around 2^-4 (the time does not depend on the values)."""
    c = torch.randint(0, 256, (B, n, Hkv, 64), dtype=U8, device="cuda", generator=gen)
    c = torch.where((c & 0x7F) == 0x7F, c - 1, c)
    s = torch.randint(120, 126, (B, n, Hkv, 2), dtype=U8, device="cuda", generator=gen)
    return c, s


def attn_part(args, out):
    from learning_jax_sharding_amd.ops import hip
    side = torch.cuda.Stream()
    out.append("| H/Hkv | B | keys | plan | bf16 us | mx8 us | mx8 / bf16 | bf16 TB/s | mx8 TB/s |")
    out.append("|---|---|---|---|---|---|---|---|---|")
    gen = torch.Generator(device="cuda").manual_seed(0)
    for H, Hkv in ((8, 2), (8, 8)):
        for B in (1, 8, 64):
            for n in ([256, 4096] if args.quick else [256, 4096, 32768]):
                live = 2 * B * n * Hkv * 64 * 2                       # K + V bytes of the live bf16 rows
                live8 = 2 * B * n * Hkv * 66
                nset = max(1, min(16, -(-600_000_000 // live8)))
                sets, sets8 = [], []
                for _ in range(nset):
                    q = torch.randn(B, 1, H, 64, device="cuda", generator=gen).to(BF16)
                    k = torch.randn(B, n, Hkv, 64, device="cuda", generator=gen).to(BF16)
                    v = torch.randn(B, n, Hkv, 64, device="cuda", generator=gen).to(BF16)
                    sets.append((q, k, v))
                    kc, ks = _q8_cache(B, n, Hkv, gen)
                    vc, vs = _q8_cache(B, n, Hkv, gen)
                    sets8.append((q, kc, vc, ks, vs))
                lens = torch.full((B,), n - 1, dtype=torch.int32).cuda()
                hip.attn_decode(*sets[0], lens, SCALE, 1)             # (the workspace, outside any capture)
                with torch.cuda.stream(side):
                    graphs = {"bf16": _graph(lambda: [hip.attn_decode(*s, lens, SCALE, 1) for s in sets], side),
                              "mx8": _graph(lambda: [hip.attn_decode_q8(*s, lens, SCALE, 1) for s in sets8], side)}
                t = _time({m: g[0] for m, g in graphs.items()}, args.replays, nset)
                out.append(f"| {H}/{Hkv} | {B} | {n} | {'x'.join(map(str, hip.plan_decode(B, Hkv, n)))} | {_fmt(t['bf16'])} | "
                           f"{_fmt(t['mx8'])} | {t['mx8'][0] / t['bf16'][0]:.3f} | {live / t['bf16'][0] / 1e6:.2f} | "
                           f"{live8 / t['mx8'][0] / 1e6:.2f} |")
                print(out[-1], flush=True)
                del graphs, sets, sets8
                torch.cuda.empty_cache()


def append_part(args, out):
    from learning_jax_sharding_amd.ops import hip
    side = torch.cuda.Stream()
    out.append("| B | H/Hkv | cap | kv_append<rot,q> us | kv_append<rot,q,mx8> us |")
    out.append("|---|---|---|---|---|")
    theta, cap, pos = 10000.0, 4096, 1000
    for B, H, Hkv in ((8, 8, 2), (64, 8, 2), (64, 8, 8)):
        gen = torch.Generator().manual_seed(0)
        mk = lambda h: torch.randn(B, 1, h, 64, generator=gen).to(BF16).cuda()   # noqa: E731
        q, k, v = mk(H), mk(Hkv), mk(Hkv)
        kc = torch.zeros(B, cap, Hkv, 64, dtype=BF16).cuda()
        vc = torch.zeros_like(kc)
        k8, v8 = torch.zeros(B, cap, Hkv, 64, dtype=U8).cuda(), torch.zeros(B, cap, Hkv, 64, dtype=U8).cuda()
        ks, vs = torch.zeros(B, cap, Hkv, 2, dtype=U8).cuda(), torch.zeros(B, cap, Hkv, 2, dtype=U8).cuda()
        lens = torch.full((B,), pos, dtype=torch.int32).cuda()
        hip.rope(q, None, pos_offset=pos, theta=theta)                # (the table, outside any capture)
        reps = 32       # calls per graph: one replay's own cost is spread over them
        with torch.cuda.stream(side), torch.no_grad():
            graphs = {"bf16": _graph(lambda: [hip.kv_append(k, v, kc, vc, lens, q=q, theta=theta)
                                              for _ in range(reps)], side),
                      "mx8": _graph(lambda: [hip.kv_append_q8(k, v, k8, v8, ks, vs, lens, q=q, theta=theta)
                                             for _ in range(reps)], side)}
        t = _time({m: g[0] for m, g in graphs.items()}, args.replays, reps)
        out.append(f"| {B} | {H}/{Hkv} | {cap} | {_fmt(t['bf16'])} | {_fmt(t['mx8'])} |")
        print(out[-1], flush=True)


def _model():
    from learning_jax_sharding_amd.models import TransformerLM
    return TransformerLM(vocab_size=32768, dim=640, layers=4, heads=8, kv_heads=2, dim_head=64, norm="rms",
                         ff="swiglu", rope_theta=10000.0, causal=True)


def generate_part(args, out):
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd.models import generate
    B, P, N = 8, 128, 32 if args.quick else 128
    model = _model()
    tok = torch.randint(0, 32768, (B, P), generator=torch.Generator().manual_seed(0))
    ids = ljs.device_put(tok.numpy())
    params = model.init(ljs.random.PRNGKey(1), ids)["params"]
    runs = {"bf16": lambda: generate(model, params, ids, N, capture=True),
            "mx8": lambda: generate(model, params, ids, N, capture=True, cache_quant="mxfp8")}
    toks, ts = {}, {n: [] for n in runs}
    for n, fn in runs.items():
        toks[n] = fn()
    torch.cuda.synchronize()
    for _ in range(ROUNDS):
        for n, fn in runs.items():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[n].append((time.perf_counter() - t0) * 1e3)
    t = {n: (statistics.median(v), min(v), max(v)) for n, v in ts.items()}
    same = float((toks["bf16"] == toks["mx8"]).float().mean())
    out.append(f"generate: dim 640, 4 layers, 8/2 heads, vocab 32768, B = {B}, {P} prompt + {N} new tokens, captured (ms, "
               f"median (min..max) of {ROUNDS}, alternated): bf16 cache {_fmt(t['bf16'])}, mxfp8 cache {_fmt(t['mx8'])}; "
               f"fraction of tokens equal between the two (random weights): {same:.3f}")
    print(out[-1], flush=True)


def long_part(args, out):
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd.ops import core
    B, cap, filled, steps = 64, 4096, 4000, 32
    model = _model()
    one = ljs.device_put(torch.randint(0, 32768, (B, 1), generator=torch.Generator().manual_seed(0)).numpy())
    params = model.init(ljs.random.PRNGKey(1), one)["params"]
    res = {"bf16": [], "mx8": []}
    state = {}
    for name, quant in (("bf16", None), ("mx8", "mxfp8")):
        cache = model.init_cache(B, cap, quant=quant)
        gen = torch.Generator(device="cuda").manual_seed(1)
        for arrs in (cache.k, cache.v):                   # a pre-filled cache: the values do not matter to the time
            for a in arrs:
                for t in a.local.values():
                    if quant:
                        t.copy_(_q8_cache(*t.shape[:3], gen)[0])
                    else:
                        t.copy_(torch.randn(t.shape, device="cuda", generator=gen).to(BF16))
        for arrs in (cache.k_scale, cache.v_scale):
            for a in arrs:
                for t in a.local.values():
                    t.fill_(123)
        step = ljs.jit(lambda p, x, c: model.apply({"params": p}, x, cache=c), donate_argnums=(2,), capture=True)
        state[name] = (cache, step)
    with torch.no_grad():
        for r in range(ROUNDS + 1):                       # round 0: the warm-up and the captures
            for name, (cache, step) in list(state.items()):
                core.cache_set_lens(cache.lens, filled)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    _, cache = step(params, one, cache)
                torch.cuda.synchronize()
                state[name] = (cache, step)               # (donated: the returned cache is the one to pass on)
                if r:
                    res[name].append((time.perf_counter() - t0) * 1e3 / steps)
    t = {n: (statistics.median(v), min(v), max(v)) for n, v in res.items()}
    fm = lambda x: f"{x[0]:.3f} ({x[1]:.3f}..{x[2]:.3f})"   # noqa: E731
    out.append(f"long context: the same model, B = {B}, a cache of {cap} rows filled to {filled}, {steps} captured decode "
               f"steps (ms per step, median (min..max) of {ROUNDS}, alternated): bf16 cache {fm(t['bf16'])}, mxfp8 cache "
               f"{fm(t['mx8'])}")
    print(out[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=tuple(PARTS) + ("all",))
    ap.add_argument("--replays", type=int, default=10)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out-dir", default=None)
    args = ap.parse_args()
    if args.part == "all":                # every part a fresh process under its own time limit; stop at a failure
        for part, limit in PARTS.items():
            cmd = [sys.executable, os.path.abspath(__file__), "--part", part, "--replays", str(args.replays)]
            cmd += ["--quick"] if args.quick else []
            cmd += ["--out-dir", args.out_dir] if args.out_dir else []
            rc = subprocess.run(cmd, timeout=limit + 30).returncode
            if rc != 0:
                raise SystemExit(f"kvq_probe: part {part} ended with {rc}; the later parts were not started")
        return
    if not torch.cuda.is_available():
        raise SystemExit("kvq_probe needs a GPU")
    os.environ.setdefault("LJS_PLATFORM", "gpu")
    os.environ.setdefault("LJS_NUM_DEVICES", "1")
    out = []
    {"attn": attn_part, "append": append_part, "generate": generate_part, "long": long_part}[args.part](args, out)
    text = "\n".join(out) + "\n"
    if args.out_dir:
        os.makedirs(args.out_dir, exist_ok=True)
        with open(os.path.join(args.out_dir, f"kvq_probe_{args.part}.md"), "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
