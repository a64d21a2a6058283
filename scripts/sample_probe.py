"""Time ``models.generate`` with sampling and stop tokens on one MI355X.

    python scripts/sample_probe.py [--quick] [--out sample_probe.md]

dim 640, 4 layers, 8/2 heads, vocab 32768, batch 8, 128 prompt + 128 new tokens, captured (the shape of
``scripts/decode_probe.py --part generate``, which times the default call the same way): the default call
(``key=None``, no eos: the argmax path as before), a key alone, a key with top_k and top_p, and stop tokens alone.
The sampling step is ``ops.kernels.sample_reference``'s torch launches inside the captured step; the difference to
the default call is what they cost per token.  Wall time of the whole call around a device sync, median
(min..max) of three after a warm-up.  Fails without a GPU.
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

ROUNDS = 3
T, TOP_K, TOP_P = 0.8, 50, 0.9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sample_probe needs a GPU")
    os.environ.setdefault("LJS_PLATFORM", "gpu")
    os.environ.setdefault("LJS_NUM_DEVICES", "1")
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd.models import TransformerLM, generate
    B, P, N = 8, 128, 32 if args.quick else 128
    model = TransformerLM(vocab_size=32768, dim=640, layers=4, heads=8, kv_heads=2, dim_head=64, norm="rms",
                          ff="swiglu", rope_theta=10000.0, causal=True)
    tok = torch.randint(0, 32768, (B, P), generator=torch.Generator().manual_seed(0))
    ids = ljs.device_put(tok.numpy())
    params = model.init(ljs.random.PRNGKey(1), ids)["params"]
    key = ljs.random.PRNGKey(2)

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(ROUNDS):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts), min(ts), max(ts)

    runs = {"default (key=None, no eos)": {},
            "key alone": dict(key=key, temperature=T),
            f"key, top_k={TOP_K}, top_p={TOP_P}": dict(key=key, temperature=T, top_k=TOP_K, top_p=TOP_P),
            "stop tokens alone, stop_poll=0": dict(eos_id=0, pad_id=0, stop_poll=0)}
    out = [f"generate, captured: dim 640, 4 layers, 8/2 heads, vocab 32768, B = {B}, {P} prompt + {N} new tokens; ms for "
           f"the whole call, median (min..max) of {ROUNDS}",
           "| call | ms | us per token |", "|---|---|---|"]
    for name, kw in runs.items():
        t = timed(lambda kw=kw: generate(model, params, ids, N, capture=True, **kw))
        out.append(f"| {name} | {t[0]:.1f} ({t[1]:.1f}..{t[2]:.1f}) | {t[0] / N * 1e3:.1f} |")
        print(out[-1], flush=True)
    text = "\n".join(out) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
