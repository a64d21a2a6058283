"""What the clipped step adds to the optimizer (modelled on scripts/adam_probe.py): the bench step's
parameter set -- 3 x [640, 512] QKV projections whose gradient is the split-K slabs of one batched
slab GEMM, W_o [512, 640] with its own slabs, 4 biases -- at the slab counts the weight-gradient
pair takes at B = 64 and B = 8 (hip.pick_dw_pair / pick_dw_slabs), timed in isolation:

  * grad_sumsq + step_hyper reading the slabs in place, against the byte floor of the gradient
    sources and against the same quantity composed in torch (slab_reduce of every weight
    gradient, then torch._foreach_norm and the norm of the norms);
  * the dynamic Adam instance (record {grad_scale, lr}) against the static one on the same inputs.

    python scripts/clip_probe.py
    python scripts/clip_probe.py --by-tiles     grad_sumsq alone on graded inputs: what its time follows
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from learning_jax_sharding_amd import optim  # noqa: E402
from learning_jax_sharding_amd.ops import hip, shadow  # noqa: E402

dev = torch.device("cuda")
ROUNDS = int(os.environ.get("ROUNDS", "7"))
SEQ = 256

_GRAPHS = {}


def timeit(fn, iters=20):
    # captured in a HIP graph: the host side (the tensor tables) takes longer than the kernels
    g = _GRAPHS.get(fn)
    if g is None:
        fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(iters):
                fn()
        _GRAPHS[fn] = g
    g.replay()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    g.replay()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3


def slab_counts(B):
    """(S_qkv, S_o) of the step's weight-gradient GEMMs over B x SEQ tokens: W_o's is reached first
    by the backward and held, the fused QKV one pairs with it."""
    T = B * SEQ
    pick = hip.pick_dw_pair(512, 640, 640, 1536, T)
    if pick is not None:
        return pick[2], pick[1]
    return hip.pick_dw_slabs(640, 1536, T)[1], hip.pick_dw_slabs(512, 640, T)[1]


def params():
    ws = [torch.randn(640, 512, device=dev) * 0.02 for _ in range(3)] + [torch.randn(512, 640, device=dev) * 0.02]
    bs = [torch.zeros(512, device=dev) for _ in range(3)] + [torch.zeros(640, device=dev)]
    for w in ws:
        shadow.get(w, "T")
        shadow.get(w, "N")
    st = [(torch.zeros_like(p), torch.zeros_like(p)) for p in ws + bs]
    return ws, bs, st


def entries(ws, bs, st, Sq, So):
    gq = torch.randn(Sq, 3, 640, 512, device=dev) * 1e-3
    go = torch.randn(So, 512, 640, device=dev) * 1e-3
    out = [(ws[i], hip.SlabGrad(gq, Sq, i * 640 * 512, 512, 3 * 640 * 512, (640, 512)), *st[i]) for i in range(3)]
    out.append((ws[3], hip.SlabGrad(go, So, 0, 640, 512 * 640, (512, 640)), *st[3]))
    for i, b in enumerate(bs):
        out.append((b, torch.randn_like(b) * 1e-3, *st[4 + i]))
    return out, gq, go


def main():
    step = torch.ones(1, dtype=torch.int32, device=dev)
    sched = optim.warmup_cosine_decay_schedule(1e-5, 1e-3, 100, 10000)
    P, nb = 3 * 640 * 512 + 512 * 640, 3 * 512 + 640
    variants, nbytes = {}, {}
    for B in (64, 8):
        Sq, So = slab_counts(B)
        ws, bs, st = params()
        e, gq, go = entries(ws, bs, st, Sq, So)
        srcs = [(t[0].shape, t[1]) for t in e]
        src_bytes = 4 * (Sq * 3 * 640 * 512 + So * 512 * 640 + nb)
        tag = f"B={B} slabs {Sq}/{So}"

        def norm_fused(srcs=srcs):
            return hip.step_hyper(step, 0, schedule=sched, max_norm=1.0, slots=hip.grad_sumsq(srcs, dev))

        goc = torch.empty(512, 640, device=dev)
        plain = [t[1] for t in e[4:]]

        gqc = torch.empty(3 * 640, 512, device=dev)

        def norm_torch_joint(gq=gq, go=go, goc=goc, gqc=gqc, plain=plain, Sq=Sq):
            # the three QKV gradients combined by ONE slab_reduce, as the step's combine does
            hip.slab_reduce(gq.view(Sq, 3 * 640, 512), gqc, 512, 3 * 640 * 512)
            hip.slab_reduce(go, goc, 640, 512 * 640)
            return torch.linalg.vector_norm(torch.stack(torch._foreach_norm([gqc, goc] + plain)))

        rec = torch.tensor([1.0, 1e-4, 0.0, 0.0], device=dev)
        e2, _, _ = entries(*params(), Sq, So)
        variants[f"{tag}: grad_sumsq + step_hyper"] = norm_fused
        variants[f"{tag}: grad_sumsq alone"] = (lambda srcs=srcs: hip.grad_sumsq(srcs, dev))
        variants[f"{tag}: slab_reduce + foreach_norm"] = norm_torch_joint
        variants[f"{tag}: adam static"] = (lambda e=e: hip.adam_multi(e, step, 1e-4, 0.9, 0.999, 1e-8, 0.0))
        variants[f"{tag}: adam dynamic"] = (lambda e2=e2, rec=rec: hip.adam_multi(e2, step, 0.0, 0.9, 0.999, 1e-8, 0.0,
                                                                                    hyper=rec))
        for k in ("grad_sumsq + step_hyper", "grad_sumsq alone"):
            nbytes[f"{tag}: {k}"] = src_bytes
        nbytes[f"{tag}: slab_reduce + foreach_norm"] = src_bytes + 8 * P     # + the combined gradient written, re-read
        for k in ("adam static", "adam dynamic"):
            nbytes[f"{tag}: {k}"] = src_bytes + 28 * P + 24 * nb     # p, m, v in and out, two bf16 shadows
    res = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for k, f in variants.items():
            res[k].append(timeit(f))
    for k, v in res.items():
        v = sorted(v)
        med = v[len(v) // 2]
        print(f"{k:46s} {med:7.2f} us  {nbytes[k] / 1e6:6.1f} MB  {nbytes[k] / med / 1e6:5.2f} TB/s "
              f"(min {v[0]:.2f}, max {v[-1]:.2f})", flush=True)


def by_tiles():
    """grad_sumsq on 1 .. 1024 tiles of plain f32, the four weights plain and as 1 / 2 / 3 / 6 slabs, and
    the four biases: the block count against the byte count."""
    v = {}
    one = [((32, 64), torch.randn(32, 64, device=dev))]
    v["1 tile"] = lambda: hip.grad_sumsq(one, dev)
    for n in (64, 256, 660, 1024):
        s = [((n * 32, 64), torch.randn(n * 32, 64, device=dev))]
        v[f"{n} tiles plain f32 [R][64]"] = (lambda s=s: hip.grad_sumsq(s, dev))
    ws = [torch.randn(640, 512, device=dev) for _ in range(3)] + [torch.randn(512, 640, device=dev)]
    s4 = [(tuple(w.shape), w) for w in ws]
    v["4 plain weights (640 tiles)"] = lambda: hip.grad_sumsq(s4, dev)
    for S in (1, 2, 3, 6):
        gq, go = torch.randn(S, 3, 640, 512, device=dev), torch.randn(S, 512, 640, device=dev)
        ss = [((640, 512), hip.SlabGrad(gq, S, i * 640 * 512, 512, 3 * 640 * 512, (640, 512))) for i in range(3)]
        ss.append(((512, 640), hip.SlabGrad(go, S, 0, 640, 512 * 640, (512, 640))))
        v[f"4 weights as {S} slabs"] = (lambda ss=ss: hip.grad_sumsq(ss, dev))
    bs = [((512,), torch.randn(512, device=dev)) for _ in range(4)]
    v["4 biases (32 tiles)"] = lambda: hip.grad_sumsq(bs, dev)
    res = {k: [] for k in v}
    for _ in range(ROUNDS):
        for k, f in v.items():
            res[k].append(timeit(f))
    for k, r in res.items():
        r = sorted(r)
        print(f"{k:34s} {r[len(r) // 2]:7.2f} us (min {r[0]:.2f})", flush=True)


if __name__ == "__main__":
    by_tiles() if "--by-tiles" in sys.argv else main()
