"""Time multi-token cached steps and greedy speculative decoding on one MI355X, head dim 64.

    python scripts/extend_probe.py [--part attn|step|generate|all] [--quick] [--new 128] [--out-dir profiles/extend]

``attn``: ``attn_extend`` at T = 2, 4, 8 against T ``attn_decode`` launches and against one, at the decode tables' shapes
(heads / kv_heads = 8/2 and 8/8, batch 1 / 8 / 64, 256 / 4096 keys; the capacity is the length plus T: the plan depends
on the capacity): us per call.

``step``: a captured cached call of the tests' model (dim 128, 2 layers, 4/2 heads, vocab 257, batch 2) on T = 4
positions (``extend=True``) against the single-token step, us per call; the same for the probe model (dim 640, 4
layers, 8/2 heads, vocab 32768).

``generate``: ``models.generate`` of the probe model at batch 2, 128 prompt + ``--new`` new tokens, captured (a call
includes its prefills, its eager warm-up call and its capture, so two lengths separate them from the rate): plain, with the
target as its own draft (every draft token accepted: the fewest rounds there can be, at twice the model cost per
round) and with a one-layer draft of random weights (acceptance near zero: the floor); 3 draft tokens, so a target
call has 2 x 4 = 8 rows.  Acceptance on random weights says nothing about trained models.

Kernel timings are HIP graphs that run the call once over each of several input sets, HIP events around
``--replays`` replays after a warm-up; the versions alternate three times and the median is reported with its
min..max.  ``--part all`` runs every part as a fresh child process under a time limit of its own and stops at the
first one that fails; this process never opens the GPU.  Fails without a GPU.
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
PARTS = {"attn": 420, "step": 240, "generate": 420}     # seconds a part may take
BF16 = torch.bfloat16


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


def attn_part(args, out):
    from learning_jax_sharding_amd.ops import hip
    side = torch.cuda.Stream()
    out.append("| H/Hkv | B | keys | T | plan | 1 x attn_decode us | T x attn_decode us | attn_extend us | extend / T decodes "
               "| extend / 1 decode |")
    out.append("|---|---|---|---|---|---|---|---|---|---|")
    gen = torch.Generator(device="cuda").manual_seed(0)
    for H, Hkv in ((8, 2), (8, 8)):
        for B in (1, 8, 64):
            for n in (256, 4096):
                for T in ((4,) if args.quick else (2, 4, 8)):
                    cap = n + T
                    nset = max(1, min(16, -(-600_000_000 // (2 * B * cap * Hkv * 128))))
                    sets = []
                    for _ in range(nset):
                        q = torch.randn(B, T, H, 64, device="cuda", generator=gen).to(BF16)
                        k = torch.randn(B, cap, Hkv, 64, device="cuda", generator=gen).to(BF16)
                        v = torch.randn(B, cap, Hkv, 64, device="cuda", generator=gen).to(BF16)
                        sets.append((q, k, v))
                    lens = torch.full((B,), n, dtype=torch.int32).cuda()
                    hip.attn_extend(*sets[0], lens, SCALE)            # (the workspace, outside any capture)
                    one = lambda s: hip.attn_decode(s[0][:, :1], s[1], s[2], lens, SCALE, 1)          # noqa: E731
                    many = lambda s: [hip.attn_decode(s[0][:, t:t + 1], s[1], s[2], lens, SCALE, t + 1)   # noqa: E731
                                      for t in range(T)]
                    with torch.cuda.stream(side):
                        graphs = {"one": _graph(lambda: [one(s) for s in sets], side),
                                  "many": _graph(lambda: [many(s) for s in sets], side),
                                  "extend": _graph(lambda: [hip.attn_extend(*s, lens, SCALE) for s in sets], side)}
                    t = _time({m: g[0] for m, g in graphs.items()}, args.replays, nset)
                    out.append(f"| {H}/{Hkv} | {B} | {n} | {T} | {'x'.join(map(str, hip.plan_decode(B, Hkv, cap)))} | "
                               f"{_fmt(t['one'])} | {_fmt(t['many'])} | {_fmt(t['extend'])} | "
                               f"{t['extend'][0] / t['many'][0]:.3f} | {t['extend'][0] / t['one'][0]:.3f} |")
                    print(out[-1], flush=True)
                    del graphs, sets
                    torch.cuda.empty_cache()


def _model(small=False, layers=None):
    from learning_jax_sharding_amd.models import TransformerLM
    if small:
        return TransformerLM(vocab_size=257, dim=128, layers=2, heads=4, kv_heads=2, dim_head=64, norm="rms",
                             ff="swiglu", rope_theta=10000.0, causal=True)
    return TransformerLM(vocab_size=32768, dim=640, layers=layers or 4, heads=8, kv_heads=2, dim_head=64, norm="rms",
                         ff="swiglu", rope_theta=10000.0, causal=True)


def step_part(args, out):
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd.ops import core
    B, cap, filled, T, steps = 2, 512, 128, 4, 64
    for name, model in (("tests' model (dim 128, 2 layers, 4/2 heads, vocab 257)", _model(small=True)),
                        ("probe model (dim 640, 4 layers, 8/2 heads, vocab 32768)", _model())):
        gen = torch.Generator().manual_seed(0)
        xs = {1: ljs.device_put(torch.randint(0, 257, (B, 1), generator=gen).numpy()),
              T: ljs.device_put(torch.randint(0, 257, (B, T), generator=gen).numpy())}
        params = model.init(ljs.random.PRNGKey(1), xs[T])["params"]
        state = {}
        for n in xs:
            fn = (lambda p, x, c: model.apply({"params": p}, x, cache=c, extend=True)) if n > 1 else \
                (lambda p, x, c: model.apply({"params": p}, x, cache=c))
            state[n] = (model.init_cache(B, cap), ljs.jit(fn, donate_argnums=(2,), capture=True))
        res = {n: [] for n in xs}
        with torch.no_grad():
            for r in range(ROUNDS + 1):                   # round 0: the warm-up and the captures
                for n, (cache, step) in list(state.items()):
                    core.cache_set_lens(cache.lens, filled)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(steps):
                        _, cache = step(params, xs[n], cache)
                    torch.cuda.synchronize()
                    state[n] = (cache, step)
                    if r:
                        res[n].append((time.perf_counter() - t0) * 1e6 / steps)
        t = {n: (statistics.median(v), min(v), max(v)) for n, v in res.items()}
        out.append(f"captured cached call, {name}, B = {B}, cache of {cap} rows from {filled} (us per call, median "
                   f"(min..max) of {ROUNDS}, alternated): 1 position {_fmt(t[1])}, {T} positions (extend) {_fmt(t[T])}: "
                   f"{t[T][0] / t[1][0]:.3f} of a single step's time for {T} positions")
        print(out[-1], flush=True)


def generate_part(args, out):
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd.models import generate
    B, P, N, k = 2, 128, 32 if args.quick else args.new, 3
    model, small = _model(), _model(layers=1)
    tok = torch.randint(0, 32768, (B, P), generator=torch.Generator().manual_seed(0))
    ids = ljs.device_put(tok.numpy())
    params = model.init(ljs.random.PRNGKey(1), ids)["params"]
    dparams = small.init(ljs.random.PRNGKey(2), ids)["params"]
    spec = dict(capture=True, draft_tokens=k, return_lens=True, stop_poll=4)
    runs = {"plain": lambda: (generate(model, params, ids, N, capture=True), None, 1.0),
            "self": lambda: generate(model, params, ids, N, draft=(model, params), **spec),
            "random": lambda: generate(model, params, ids, N, draft=(small, dparams), **spec)}
    first, ts = {}, {n: [] for n in runs}
    for n, fn in runs.items():
        first[n] = fn()
    torch.cuda.synchronize()
    for _ in range(ROUNDS):
        for n, fn in runs.items():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[n].append((time.perf_counter() - t0) * 1e3)
    t = {n: (statistics.median(v), min(v), max(v)) for n, v in ts.items()}
    same = {n: bool(torch.equal(first[n][0], first["plain"][0])) for n in runs}
    out.append(f"generate: dim 640, 4 layers, 8/2 heads, vocab 32768, B = {B}, {P} prompt + {N} new tokens, captured, {k} draft "
               f"tokens, counts read every 4 rounds (ms, median (min..max) of {ROUNDS}, alternated; a call includes its "
               f"prefills and its capture): plain {_fmt(t['plain'])}; the target as its own draft {_fmt(t['self'])} "
               f"({first['self'][2]:.2f} tokens per round, tokens equal plain's: {same['self']}); a one-layer draft of random "
               f"weights {_fmt(t['random'])} ({first['random'][2]:.2f} tokens per round, tokens equal plain's: "
               f"{same['random']})")
    print(out[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=tuple(PARTS) + ("all",))
    ap.add_argument("--replays", type=int, default=10)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--new", type=int, default=128, help="generate: new tokens per sequence")
    ap.add_argument("--out-dir", default=None)
    args = ap.parse_args()
    if args.part == "all":                # every part a fresh process under its own time limit; stop at a failure
        for part, limit in PARTS.items():
            cmd = [sys.executable, os.path.abspath(__file__), "--part", part, "--replays", str(args.replays)]
            cmd += ["--quick"] if args.quick else []
            cmd += ["--new", str(args.new)]
            cmd += ["--out-dir", args.out_dir] if args.out_dir else []
            rc = subprocess.run(cmd, timeout=limit + 30).returncode
            if rc != 0:
                raise SystemExit(f"extend_probe: part {part} ended with {rc}; the later parts were not started")
        return
    if not torch.cuda.is_available():
        raise SystemExit("extend_probe needs a GPU")
    os.environ.setdefault("LJS_PLATFORM", "gpu")
    os.environ.setdefault("LJS_NUM_DEVICES", "1")
    out = []
    {"attn": attn_part, "step": step_part, "generate": generate_part}[args.part](args, out)
    text = "\n".join(out) + "\n"
    if args.out_dir:
        os.makedirs(args.out_dir, exist_ok=True)
        with open(os.path.join(args.out_dir, f"extend_probe_{args.part}.md"), "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
