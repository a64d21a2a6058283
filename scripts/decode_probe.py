"""Time the decode kernels of csrc/kernels/decode.hip on one MI355X, bf16, head dim 64.

    python scripts/decode_probe.py [--part attn|append|generate|all] [--quick] [--out decode_probe.md]

``attn``: ``attn_decode`` alone at heads / kv_heads = 8/8 and 8/2, batch 1 / 8 / 64, length 256 / 4096 / 32768
(the cache capacity is the length: the plan depends on the capacity) against

  * what the code had before: ``attn_fwd_lse`` on one query with ``causal`` and ``q_offset`` (one block per
    (batch, query head), walking all keys),
  * torch SDPA on K / V already expanded to one head per query head (the expansion is not timed),
  * the byte floor: the K + V bytes of the live rows over 8 TB/s (the HBM peak in MI355X_MICROARCH.md).

``append``: ``kv_append`` (rotate q and k at the device position, copy v, one launch) against ``rope`` + two
``copy_`` into the cache rows at a HOST position (what a step without the kernel would launch), 32 calls
per graph.

``generate``: ``models.generate`` for dim 640, 4 layers, 8/2 heads, vocab 32768, batch 8, 128 prompt + 128
new tokens: captured, eager, and the uncached loop that re-runs the whole prefix for every token; and the
launch list of one decode step.

Every kernel timing is a HIP graph that runs the call once over each of several input sets (enough
sets that a sweep moves ~600 MB, so a replay does not find its inputs in the 256 MB Infinity Cache;
capped at 16), HIP events around ``--replays`` replays after a warm-up, divided by replays x sets; the
versions alternate three times and the median is reported with its min..max.  Fails without a GPU.
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12
ROUNDS = 3
SCALE = 0.125


def _graph(fn, side):
    for _ in range(2):
        fn()
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side, capture_error_mode="relaxed"):
        keep = fn()
    return g, keep


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
    return f"{t[0]:.1f} ({t[1]:.1f}..{t[2]:.1f})"


def attn_part(args, out):
    from learning_jax_sharding_amd.ops import hip
    side = torch.cuda.Stream()
    out.append("| H/Hkv | B | length | plan | attn_decode us | attn_fwd_lse (1 query) us | SDPA (expanded K/V) us | "
               "byte floor us | decode GB/s |")
    out.append("|---|---|---|---|---|---|---|---|---|")
    lengths = [256, 4096] if args.quick else [256, 4096, 32768]
    for H, Hkv in ((8, 8), (8, 2)):
        for B in (1, 8, 64):
            for n in lengths:
                live = 2 * B * n * Hkv * 64 * 2                       # K + V bytes of the live rows
                nset = max(1, min(16, -(-600_000_000 // live)))
                gen = torch.Generator().manual_seed(0)
                sets = []
                for _ in range(nset):
                    q = torch.randn(B, 1, H, 64, generator=gen).to(torch.bfloat16).cuda()
                    k = torch.randn(B, n, Hkv, 64, generator=gen).to(torch.bfloat16).cuda()
                    v = torch.randn(B, n, Hkv, 64, generator=gen).to(torch.bfloat16).cuda()
                    sets.append((q, k, v))
                lens = torch.full((B,), n - 1, dtype=torch.int32).cuda()
                G = H // Hkv
                hip.attn_decode(*sets[0], lens, SCALE, 1)             # (the workspace, outside any capture)
                graphs = {}
                with torch.cuda.stream(side):
                    graphs["decode"] = _graph(lambda: [hip.attn_decode(q, k, v, lens, SCALE, 1) for q, k, v in sets],
                                              side)
                    graphs["fwd"] = _graph(lambda: [hip.attn_fwd_lse(q, k, v, SCALE, True, n - 1) for q, k, v in sets],
                                           side)
                    ex = [(q.transpose(1, 2), k.repeat_interleave(G, 2).transpose(1, 2),
                           v.repeat_interleave(G, 2).transpose(1, 2)) for q, k, v in sets]
                    graphs["sdpa"] = _graph(lambda: [torch.nn.functional.scaled_dot_product_attention(
                        a, b, c, scale=SCALE) for a, b, c in ex], side)
                t = _time({m: g[0] for m, g in graphs.items()}, args.replays, nset)
                floor = live / HBM_BYTES_PER_S * 1e6
                out.append(f"| {H}/{Hkv} | {B} | {n} | {'x'.join(map(str, hip.plan_decode(B, Hkv, n)))} | "
                           f"{_fmt(t['decode'])} | {_fmt(t['fwd'])} | {_fmt(t['sdpa'])} | {floor:.2f} | "
                           f"{live / t['decode'][0] / 1e3:.0f} |")
                print(out[-1], flush=True)
                del graphs, sets, ex
                torch.cuda.empty_cache()


def append_part(args, out):
    from learning_jax_sharding_amd.ops import hip
    side = torch.cuda.Stream()
    out.append("")
    out.append("| B | H/Hkv | cap | kv_append us | rope + 2 copy_ us |")
    out.append("|---|---|---|---|---|")
    theta, cap, pos = 10000.0, 4096, 1000
    for B, H, Hkv in ((8, 8, 2), (64, 8, 2), (64, 8, 8)):
        gen = torch.Generator().manual_seed(0)
        mk = lambda h: torch.randn(B, 1, h, 64, generator=gen).to(torch.bfloat16).cuda()   # noqa: E731
        q, k, v = mk(H), mk(Hkv), mk(Hkv)
        kc = torch.zeros(B, cap, Hkv, 64, dtype=torch.bfloat16).cuda()
        vc = torch.zeros_like(kc)
        lens = torch.full((B,), pos, dtype=torch.int32).cuda()
        hip.rope(q, None, pos_offset=pos, theta=theta)

        def composite():
            qr, _ = hip.rope(q, None, pos_offset=pos, theta=theta)
            kr, _ = hip.rope(k, None, pos_offset=pos, theta=theta)
            kc[:, pos:pos + 1].copy_(kr)
            vc[:, pos:pos + 1].copy_(v)
            return qr

        reps = 32       # calls per graph: one replay's own cost is spread over them
        with torch.cuda.stream(side), torch.no_grad():
            graphs = {"append": _graph(lambda: [hip.kv_append(k, v, kc, vc, lens, q=q, theta=theta)
                                                for _ in range(reps)], side),
                      "composite": _graph(lambda: [composite() for _ in range(reps)], side)}
        t = _time({m: g[0] for m, g in graphs.items()}, args.replays, reps)
        out.append(f"| {B} | {H}/{Hkv} | {cap} | {_fmt(t['append'])} | {_fmt(t['composite'])} |")
        print(out[-1], flush=True)


def generate_part(args, out):
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd.models import TransformerLM, generate
    from learning_jax_sharding_amd.ops import hip
    B, P, N = 8, 128, 32 if args.quick else 128
    model = TransformerLM(vocab_size=32768, dim=640, layers=4, heads=8, kv_heads=2, dim_head=64, norm="rms",
                          ff="swiglu", rope_theta=10000.0, causal=True)
    tok = torch.randint(0, 32768, (B, P), generator=torch.Generator().manual_seed(0))
    ids = ljs.device_put(tok.numpy())
    params = model.init(ljs.random.PRNGKey(1), ids)["params"]

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(ROUNDS):
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return res, (statistics.median(ts), min(ts), max(ts))

    cap_toks, t_cap = timed(lambda: generate(model, params, ids, N, capture=True))
    eag_toks, t_eag = timed(lambda: generate(model, params, ids, N, capture=False))

    try:
        ref_toks, t_ref = timed(lambda: _reforward_host(model, params, tok, N, ljs))
    except Exception as e:      # (reported, not hidden)
        ref_toks, t_ref = None, None
        out.append(f"uncached loop failed: {e!r}")
    same = bool(torch.equal(cap_toks, eag_toks))
    agree = None if ref_toks is None else float((ref_toks == eag_toks).float().mean())
    out.append("")
    out.append(f"generate: dim 640, 4 layers, 8/2 heads, vocab 32768, B = {B}, {P} prompt + {N} new tokens (ms, median "
               f"(min..max) of {ROUNDS}): captured {_fmt(t_cap)}, eager {_fmt(t_eag)}, uncached re-forward loop "
               f"{'failed' if t_ref is None else _fmt(t_ref)}; captured == eager tokens: {same}; fraction of tokens "
               f"equal to the uncached loop's: {agree}")
    print(out[-1], flush=True)
    cache = model.init_cache(B, P + 8)
    with torch.no_grad():
        _, cache = model.apply({"params": params}, ids, cache=cache)
        one = ljs.device_put(tok[:, :1].numpy())
        model.apply({"params": params}, one, cache=cache)
        n0 = hip.lib().ljs_launch_count()
        with hip.launch_log() as log:
            model.apply({"params": params}, one, cache=cache)
    names = [r["name"] for r in log]
    out.append(f"one decode step records {hip.lib().ljs_launch_count() - n0} launches of the library; the last "
               f"{len(names)}: {', '.join(names)}")
    print(out[-1], flush=True)


def _reforward_host(model, params, tok, N, ljs):
    cur = tok.clone()
    with torch.no_grad():
        for _ in range(N):
            logits = model.apply({"params": params}, ljs.device_put(cur.numpy())).local_tensors()[0]
            cur = torch.cat([cur, logits[:, -1].float().argmax(-1, keepdim=True).cpu()], dim=1)
    return cur[:, tok.shape[1]:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=("attn", "append", "generate", "all"))
    ap.add_argument("--replays", type=int, default=10)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("decode_probe needs a GPU")
    os.environ.setdefault("LJS_PLATFORM", "gpu")
    os.environ.setdefault("LJS_NUM_DEVICES", "1")
    out = []
    if args.part in ("attn", "all"):
        attn_part(args, out)
    if args.part in ("append", "all"):
        append_part(args, out)
    if args.part in ("generate", "all"):
        generate_part(args, out)
    text = "\n".join(out) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
