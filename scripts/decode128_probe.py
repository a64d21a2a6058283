"""Time the head dim 128 cache kernels of csrc/kernels/decode.hip on one MI355X (bf16 and MX-fp8 caches).

    python scripts/decode128_probe.py [--part attn|append|extend|generate|all] [--quick] [--out decode128_probe.md]

``attn``: ``attn_decode`` at head dim 128 (``attn_decode128<..>`` and its ``mx8`` instance) at heads / kv_heads = 8/2 and
8/8, batch 1 / 8 / 64, length 256 / 4096 / 32768 (the capacity is the length) against ``attn_decode_reference`` on the same
GPU (what a 128-wide cache ran before; skipped above 1 GB of live K + V, where its f32 copies no longer fit a sweep of
input sets) and against the 64 kernel at equal live K + V bytes: the same batch and heads at head dim 64 and twice the keys.
``append``: ``kv_append128`` against ``rope`` + two ``copy_`` at a host position.  ``extend``: ``attn_extend128`` at T = 2 / 4
/ 8 against T single ``attn_decode`` launches.  ``generate``: dim 1024, 8 heads of 128, 2 kv heads, captured, against
``LJS_FUSED_DECODE=0``.

The timing is scripts/decode_probe.py's: a HIP graph over several input sets (a sweep moves ~600 MB), HIP events around
``--replays`` replays, versions alternated three times, the median with its min..max.  Fails without a GPU.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)
from decode_probe import _fmt, _graph, _time  # noqa: E402

BF16, U8 = torch.bfloat16, torch.uint8
SCALE = 128 ** -0.5


def _sets(B, n, H, Hkv, D, nset, mx8):
    """``nset`` (q, cache) pairs of full caches; MX-fp8 ones are random e4m3 bytes below NaN with scales near 1."""
    gen = torch.Generator().manual_seed(0)
    out = []
    for _ in range(nset):
        q = torch.randn(B, 1, H, D, generator=gen).to(BF16).cuda()
        if mx8:
            kv = [torch.randint(0, 0x78, (B, n, Hkv, D), generator=gen, dtype=U8).cuda() for _ in range(2)]
            kv += [torch.randint(124, 128, (B, n, Hkv, D // 32), generator=gen, dtype=U8).cuda() for _ in range(2)]
        else:
            kv = [torch.randn(B, n, Hkv, D, generator=gen).to(BF16).cuda() for _ in range(2)]
        out.append((q, kv))
    return out


def attn_part(args, out):
    from learning_jax_sharding_amd.ops import hip, kernels as K
    side = torch.cuda.Stream()
    out.append("| H/Hkv | B | length | decode128 us | decode128 mx8 us | reference us | decode64 (2 x length) us | 128 / 64 per byte | "
               "decode128 GB/s |")
    out.append("|---|---|---|---|---|---|---|---|---|")
    for H, Hkv in ((8, 2), (8, 8)):
        for B in (1, 8, 64):
            for n in ([256, 4096] if args.quick else [256, 4096, 32768]):
                live = 2 * B * n * Hkv * 128 * 2
                nset = max(1, min(16, -(-600_000_000 // live)))
                lens, lens2 = (torch.full((B,), m - 1, dtype=torch.int32).cuda() for m in (n, 2 * n))
                forms = {"d128": (hip.attn_decode, _sets(B, n, H, Hkv, 128, nset, False), lens),
                         "mx8": (hip.attn_decode_q8, _sets(B, n, H, Hkv, 128, nset, True), lens),
                         "d64": (hip.attn_decode, _sets(B, 2 * n, H, Hkv, 64, nset, False), lens2)}
                if live <= 1 << 30:
                    forms["ref"] = (K.attn_decode_reference, forms["d128"][1], lens)
                graphs = {}
                with torch.cuda.stream(side), torch.no_grad():
                    for name, (fn, sets, lt) in forms.items():
                        sc = 0.125 if name == "d64" else SCALE
                        fn(sets[0][0], *sets[0][1], lt, sc, 1)              # (the workspace, outside any capture)
                        graphs[name] = _graph(lambda fn=fn, sets=sets, lt=lt, sc=sc: [fn(q, *kv, lt, sc, 1) for q, kv in sets], side)
                t = _time({m: g[0] for m, g in graphs.items()}, args.replays, nset)
                out.append(f"| {H}/{Hkv} | {B} | {n} | {_fmt(t['d128'])} | {_fmt(t['mx8'])} | "
                           f"{_fmt(t['ref']) if 'ref' in t else '-'} | {_fmt(t['d64'])} | {t['d128'][0] / t['d64'][0]:.2f} | "
                           f"{live / t['d128'][0] / 1e3:.0f} |")
                print(out[-1], flush=True)
                del graphs, forms
                torch.cuda.empty_cache()


def append_part(args, out):
    from learning_jax_sharding_amd.ops import hip
    side = torch.cuda.Stream()
    out += ["", "| B | H/Hkv | cap | kv_append128 us | rope + 2 copy_ us |", "|---|---|---|---|---|"]
    theta, cap, pos, reps = 10000.0, 4096, 1000, 32
    for B, H, Hkv in ((8, 8, 2), (64, 8, 2), (64, 8, 8)):
        gen = torch.Generator().manual_seed(0)
        q, k, v = (torch.randn(B, 1, h, 128, generator=gen).to(BF16).cuda() for h in (H, Hkv, Hkv))
        kc = torch.zeros(B, cap, Hkv, 128, dtype=BF16).cuda()
        vc = torch.zeros_like(kc)
        lens = torch.full((B,), pos, dtype=torch.int32).cuda()

        def composite():
            qr, _ = hip.rope(q, None, pos_offset=pos, theta=theta)
            kr, _ = hip.rope(k, None, pos_offset=pos, theta=theta)
            kc[:, pos:pos + 1].copy_(kr)
            vc[:, pos:pos + 1].copy_(v)
            return qr

        composite()
        with torch.cuda.stream(side), torch.no_grad():
            graphs = {"append": _graph(lambda: [hip.kv_append(k, v, kc, vc, lens, q=q, theta=theta) for _ in range(reps)], side),
                      "composite": _graph(lambda: [composite() for _ in range(reps)], side)}
        t = _time({m: g[0] for m, g in graphs.items()}, args.replays, reps)
        out.append(f"| {B} | {H}/{Hkv} | {cap} | {_fmt(t['append'])} | {_fmt(t['composite'])} |")
        print(out[-1], flush=True)


def extend_part(args, out):
    from learning_jax_sharding_amd.ops import hip
    side = torch.cuda.Stream()
    out += ["", "| B | H/Hkv | length | T | attn_extend128 us | T x attn_decode128 us |", "|---|---|---|---|---|---|"]
    B, H, Hkv, n = 8, 8, 2, 4096
    gen = torch.Generator().manual_seed(0)
    kc, vc = (torch.randn(B, n, Hkv, 128, generator=gen).to(BF16).cuda() for _ in range(2))
    lens = torch.full((B,), n - 16, dtype=torch.int32).cuda()
    for T in (2, 4, 8):
        q = torch.randn(B, T, H, 128, generator=gen).to(BF16).cuda()
        hip.attn_extend(q, kc, vc, lens, SCALE)
        with torch.cuda.stream(side), torch.no_grad():
            graphs = {"extend": _graph(lambda: hip.attn_extend(q, kc, vc, lens, SCALE), side),
                      "steps": _graph(lambda: [hip.attn_decode(q[:, t:t + 1], kc, vc, lens, SCALE, t + 1) for t in range(T)], side)}
        t = _time({m: g[0] for m, g in graphs.items()}, args.replays, 1)
        out.append(f"| {B} | {H}/{Hkv} | {n} | {T} | {_fmt(t['extend'])} | {_fmt(t['steps'])} |")
        print(out[-1], flush=True)


def generate_part(args, out):
    import statistics
    import time
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd.models import TransformerLM, generate
    B, P, N = 8, 128, 32 if args.quick else 128
    model = TransformerLM(vocab_size=512, dim=1024, layers=2, heads=8, kv_heads=2, dim_head=128, norm="rms", ff="swiglu",
                          rope_theta=10000.0, causal=True)
    tok = torch.randint(0, 512, (B, P), generator=torch.Generator().manual_seed(0))
    ids = ljs.device_put(tok.numpy())
    params = model.init(ljs.random.PRNGKey(1), ids)["params"]
    res = {}
    for fused in ("1", "0", "1", "0", "1", "0"):
        os.environ["LJS_FUSED_DECODE"] = fused
        generate(model, params, ids, N, capture=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        generate(model, params, ids, N, capture=True)
        torch.cuda.synchronize()
        res.setdefault(fused, []).append((time.perf_counter() - t0) * 1e3)
    os.environ.pop("LJS_FUSED_DECODE")
    f = lambda v: (statistics.median(v), min(v), max(v))   # noqa: E731
    out += ["", f"generate: dim 1024, 2 layers, 8/2 heads of 128, B = {B}, {P} prompt + {N} new tokens, captured (ms, median "
                f"(min..max) of 3, alternated): kernels {_fmt(f(res['1']))}, LJS_FUSED_DECODE=0 {_fmt(f(res['0']))}"]
    print(out[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=("attn", "append", "extend", "generate", "all"))
    ap.add_argument("--replays", type=int, default=10)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("decode128_probe needs a GPU")
    os.environ.setdefault("LJS_PLATFORM", "gpu")
    os.environ.setdefault("LJS_NUM_DEVICES", "1")
    os.environ.setdefault("LJS_ATTN_D128", "1")      # (the prompt's own prefill attention in the generate part)
    out = []
    for name, fn in (("attn", attn_part), ("append", append_part), ("extend", extend_part), ("generate", generate_part)):
        if args.part in (name, "all"):
            fn(args, out)
    text = "\n".join(out) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
