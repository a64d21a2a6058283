"""SHA-256 of what the streaming kernels (norm, xent, loss, elementwise), the bf16 GEMMs and the MX-fp8
GEMMs compute on a fixed list of small seeded cases, one ``case-name sha256`` line per output tensor:
two builds of the library compute the same bits exactly when their lines are equal.  The ``gemm``
group also prints each case's launch record, so equal lines mean the same kernels on the same grids
too; the ``mx`` group prints hashes only, so it also runs on a library that records no fp8 launch.

    python scripts/kernel_digest.py [--json out.json] [--grep norm]
    LJS_KERNELS_LIB=path/to/libljs_kernels.so python scripts/kernel_digest.py    # another build

(Another build has to export every function ops/hip.py binds; to compare with a commit whose library
does not, copy this script into a checkout of that commit and run it there.)

Every kernel here fixes the order of its sums by the shape alone, so a run is comparable with any
other run by digest; one process per library.  Inputs are made on the CPU from a generator seeded
by the case name and copied to the device.  The shapes are the smallest that reach each code path
of the kernels (named next to each list).  Fails without a GPU.
"""
import argparse
import hashlib
import json
import os
import sys
import zlib

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from learning_jax_sharding_amd.ops import hip  # noqa: E402

F32, BF16 = torch.float32, torch.bfloat16
_N = {F32: "f32", BF16: "bf16", torch.int32: "i32", torch.int64: "i64"}
DEV = torch.device("cuda", 0)

# norm.hip: two rows per wave with an odd tail; a partial second chunk; the wave / block pair
# around kWaveMaxD = 1024; 35 backward blocks = two ticket groups (wave mapping, 16 rows a block);
# two groups in the block mapping; past the 512-block backward cap; the widest row
NORM_SHAPES = [(1, 8), (7, 512), (5, 520), (3, 1024), (3, 1032), (545, 512), (33, 1032), (513, 1032), (2, 8192)]
# xent.hip: tail only; the pair around kWaveMaxV = 2048 (f32: a one-element tail); kU chunks with a
# short last batch; past the 2048-block cap of the block mapping
XENT_SHAPES = [(1, 1), (5, 7), (5, 2048), (5, 2049), (3, 4100), (2049, 2049)]
XENT_STRIDED = (6, 1000, 1024)  # rows of 1000 in a [6][1024] buffer, from column 1
# sum_all: tail only; one block; the test suite's odd size; 33 blocks (32 blocks of 256 threads x
# 16 chunks of 16 bytes, plus one element) = two ticket levels
SUM_N = {F32: [5, 4096, 3 * 2 ** 20 + 8, 32 * 256 * 16 * 4 + 1],
         BF16: [5, 4096, 3 * 2 ** 20 + 8, 32 * 256 * 16 * 8 + 1]}
COLSUM_SHAPES = [(77, 8), (1000, 64), (16384, 640)]
RELU_SHAPES = [(300, 72, 72), (256, 64, 192)]  # (R, C, row stride of y)
# mse: tail only; 33 blocks (256 threads x 4 chunks of 8) = two ticket levels, and a 3-element tail
MSE_N = [11, 262155]
# mse + column sums: one block; 18 row blocks x 2 column blocks = the per-column ticket and both
# levels of the loss ticket
MSE_COLSUM_SHAPES = [(200, 64), (1637, 128)]


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _randn(g, shape, dtype, mul=1.0, add=0.0):
    return (torch.randn(shape, generator=g) * mul + add).to(dtype).to(DEV)


class Out:
    def __init__(self):
        self.lines = []

    def add(self, name, t):
        t = t.detach().contiguous().cpu()
        h = hashlib.sha256(t.reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()
        self.lines.append((f"{name}[{_N.get(t.dtype, t.dtype)}{list(t.shape)}]", h))
        print(*self.lines[-1], flush=True)

    def record(self, name):
        """The last launch's record (ops/hip.py last_launch) as a line of its own."""
        rec = hip.last_launch()
        self.lines.append((name + "/record", ",".join(f"{k}={rec[k]}" for k in sorted(rec)).replace(" ", "")))
        print(*self.lines[-1], flush=True)


def norm_cases(out):
    for kind in ("layer", "rms"):
        for xdt, ydt in ((F32, BF16), (BF16, BF16)):
            for R, D in NORM_SHAPES:
                name = f"norm/{kind}/{_N[xdt]}-{_N[ydt]}/{R}x{D}"
                g = _gen(name)
                x = _randn(g, (R, D), xdt, 1.5, 0.5).requires_grad_(True)
                scale = _randn(g, (D,), F32, 0.1, 1.0).requires_grad_(True)
                bias = _randn(g, (D,), F32, 0.1).requires_grad_(True) if kind == "layer" else None
                cot = _randn(g, (R, D), ydt)
                y = hip.norm(x, scale, bias, 1e-5, kind, ydt)
                y.backward(cot)
                out.add(name + "/y", y)
                out.add(name + "/dx", x.grad)
                out.add(name + "/dscale", scale.grad)
                if bias is not None:
                    out.add(name + "/dbias", bias.grad)


def _xent_one(out, name, x, R, V, ldt):
    g = _gen(name)
    for off in (0, 3):
        lab = torch.randint(off, off + V, (R,), generator=g)
        if off:
            lab[::3] += V  # labels of the shard above, and one of the shard below
            if R > 2:
                lab[1] = 0
        if R > 1:
            lab[R // 2] = -1
        lab = lab.to(ldt).to(DEV)
        x.grad = None
        if off == 0:
            loss = hip.xent(x, lab)
            loss.backward(_randn(g, (R,), F32))
            out.add(f"{name}/loss", loss)
        else:
            m, ls, t = hip.xent_stats(x, lab, off)
            torch.autograd.backward([ls, t], [_randn(g, (R,), F32), _randn(g, (R,), F32)])
            for k, v in (("m", m), ("logs", ls), ("t", t)):
                out.add(f"{name}/off{off}/{k}", v)
        out.add(f"{name}/off{off}/dx", x.grad)


def xent_cases(out):
    for dt in (F32, BF16):
        for ldt in (torch.int32, torch.int64):
            for R, V in XENT_SHAPES:
                name = f"xent/{_N[dt]}/{_N[ldt]}/{R}x{V}"
                x = _randn(_gen(name + "/x"), (R, V), dt, 2.0).requires_grad_(True)
                _xent_one(out, name, x, R, V, ldt)
            R, V, ld = XENT_STRIDED
            name = f"xent/{_N[dt]}/{_N[ldt]}/{R}x{V}-ld{ld}"
            buf = _randn(_gen(name + "/x"), (R, ld), dt, 2.0)
            x = buf[:, 1:1 + V].detach().requires_grad_(True)
            assert x.stride(0) == ld
            _xent_one(out, name, x, R, V, ldt)


def sum_cases(out):
    for dt in (F32, BF16):
        for n in SUM_N[dt]:
            x = _randn(_gen(f"sum/{_N[dt]}/{n}"), (n,), dt)
            for odt in (F32, BF16):
                out.add(f"sum_all/{_N[dt]}-{_N[odt]}/{n}", hip._sum_all_raw(x, odt))


def colsum_cases(out):
    for R, C in COLSUM_SHAPES:
        x = _randn(_gen(f"colsum/{R}x{C}"), (R, C), BF16)
        o = hip.colsum(x)
        out.add(f"colsum/{R}x{C}", o)
        if (R, C) == COLSUM_SHAPES[1]:
            out.add(f"colsum/{R}x{C}/accumulate", hip.colsum(x, o.clone(), accumulate=True))
    for R, C, yld in RELU_SHAPES:
        g = _gen(f"relu/{R}x{C}x{yld}")
        dy, ybuf = _randn(g, (R, C), BF16), _randn(g, (R, yld), BF16)
        ybuf[0, :4] = torch.tensor([0.0, -0.0, 1e-30, -1e-30], dtype=BF16)
        masked, db = hip.relu_bwd_colsum(dy, ybuf[:, :C], R, C)
        out.add(f"relu_bwd_colsum/{R}x{C}x{yld}/masked", masked)
        out.add(f"relu_bwd_colsum/{R}x{C}x{yld}/db", db)
        out.add(f"relu_bwd/{R}x{C}x{yld}", hip.relu_bwd(dy, ybuf[:, :C], R, C))


def mse_cases(out):
    L, p, st = hip.lib(), hip._p, hip._stream
    for tdt in (F32, BF16):
        # ops.hip.mse_loss takes last dims that are a multiple of 8 only; the flat kernel takes any
        # n, so the tail cases go to the library with ops.hip's workspace
        for n in MSE_N:
            name = f"mse/{_N[tdt]}/{n}"
            g = _gen(name)
            y, t = _randn(g, (n,), BF16), _randn(g, (n,), tdt)
            for want_dy in (False, True):
                o = torch.empty((), dtype=F32, device=DEV)
                dy = torch.empty_like(y) if want_dy else None
                ws = hip._workspace(DEV, "mse", (1024 + 33) * 4)
                hip._ck(L.ljs_mse_loss(p(y), p(t), int(tdt == BF16), n, 0.25, p(dy), p(o), p(ws), st(y)), "mse_loss")
                out.add(f"{name}/{'grad' if want_dy else 'nograd'}/loss", o)
                if want_dy:
                    out.add(f"{name}/grad/dy", dy)
        for R, C in MSE_COLSUM_SHAPES:
            name = f"mse_colsum/{_N[tdt]}/{R}x{C}"
            g = _gen(name)
            y, t = _randn(g, (R, C), BF16), _randn(g, (R, C), tdt)
            o = torch.empty((), dtype=F32, device=DEV)
            dy, sums = torch.empty_like(y), torch.empty((C,), dtype=F32, device=DEV)
            ws = hip._workspace(DEV, f"mse_colsum/{R}x{C}", L.ljs_mse_colsum_ws_bytes(R, C))
            hip._ck(L.ljs_mse_colsum(p(y), p(t), int(tdt == BF16), R, C, 0.25, p(dy), p(sums), p(o), p(ws), st(y)),
                    "mse_colsum")
            for k, v in (("loss", o), ("dy", dy), ("colsum", sums)):
                out.add(f"{name}/{k}", v)


def misc_cases(out):
    g = _gen("misc")
    x = _randn(g, (37, 1000), F32)
    out.add("cast/f32-bf16", hip.cast(x, BF16))
    out.add("cast/bf16-f32", hip.cast(x.to(BF16), F32))
    out.add("softmax_rows_f32", hip.softmax_lastdim(_randn(g, (9, 333), F32, 3.0)))
    p, gr = _randn(g, (1003,), F32), _randn(g, (1003,), F32)
    m, v = _randn(g, (1003,), F32, 0.1), _randn(g, (1003,), F32, 0.1).abs()
    step = torch.full((), 3, dtype=torch.int32, device=DEV)
    for k, t in zip("pmv", hip.adam(p, gr, m, v, step, 1e-3, 0.9, 0.999, 1e-8, 0.01, False)):
        out.add(f"adam_f32/{k}", t)


def _gemm(out, name, tile, a_kc, b_kc, out_f32, M, N, K, hashed=True, **kw):
    """One bf16 GEMM from seeded operands in the asked layouts: C, the fused output sums where the
    kernel wrote any, and the launch record (which kernel instance, grid, tile, split, variant)."""
    g = _gen(name)
    A, B = _randn(g, (M, K), BF16), _randn(g, (K, N), BF16)
    As, lda = (A, K) if a_kc else (A.t().contiguous(), M)
    Bs, ldb = (B.t().contiguous(), K) if b_kc else (B, N)
    C = torch.full((M, N), float("nan"), dtype=F32 if out_f32 else BF16, device=DEV)
    if kw.pop("bias", False):
        kw["bias"] = _randn(g, (N,), F32)
    if "res" in kw:
        kw.update(res=_randn(g, (M, N), kw["res"]), res_ld=N)
    psum = torch.zeros(hip.psum_slots(M, N), dtype=F32, device=DEV) if kw.pop("psum", False) else None
    cnt = hip.gemm(As, Bs, C, M, N, K, lda, ldb, N, bool(a_kc), bool(b_kc), tile=tile, psum=psum, **kw)
    out.record(name)
    if hashed:
        out.add(name + "/C", C)
        if cnt:
            out.add(name + "/psum", psum[:cnt])


def gemm_cases(out):
    """gemm.hip's bf16 launcher: every tile and kernel family at one ragged block (the instance
    lists of tests/test_kernel_variants_gpu.py), the epilogue instances, slabs alone and as a
    grouped pair, the folded batch, a persistent grid.  Atomics split-K has no fixed sum order: its
    record is printed, its output is not hashed."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_kernel_variants_gpu as tv
    kk = tv._LEAN + tv._DMA_KK
    for tile, M, N, K, _ in kk:
        _gemm(out, f"gemm/kk/{tile}/{M}x{N}x{K}", tile, 1, 1, 0, M, N, K)
    for tile, M, N, K in ((643, 72, 40, 128), (1284, 136, 72, 128)):          # test_gemm_dma_layout_instances
        for a_kc, b_kc, of in ((a, b, o) for a in (1, 0) for b in (1, 0) for o in (0, 1)):
            forced = 200000 if (tile == 1284 and a_kc and b_kc and not of) else 0
            _gemm(out, f"gemm/layout/{tile}/{a_kc}{b_kc}{of}/{M}x{N}x{K}", tile + forced, a_kc, b_kc, of, M, N, K)
    for tile in (64, 128, 644, 1282):                 # register-staged, asked for and by demotion (K % 64)
        for a_kc, b_kc, of in ((1, 1, 0), (0, 0, 1), (1, 0, 0), (0, 1, 1)):
            _gemm(out, f"gemm/reg/{tile}/{a_kc}{b_kc}{of}/136x72x40", tile, a_kc, b_kc, of, 136, 72, 40)
    epilogues = {"plain": {}, "bias-psum": dict(bias=True, psum=True), "res-bf16": dict(res=BF16),
                 "res-f32": dict(res=F32), "mask": dict(res=BF16, res_mode="mask"),
                 "relu-alpha": dict(bias=True, relu=True, alpha=0.5)}
    for tile, (ename, kw) in ((t, e) for t in sorted({c[0] for c in kk}) for e in epilogues.items()):
        _gemm(out, f"gemm/epilogue/{tile}/{ename}/136x72x128", tile, 1, 1, 0, 136, 72, 128, **kw)
    T, K, N, S = 448, 136, 72, 3                      # test_gemm_slab_instance: 7 K-tiles as 3 + 3 + 1

    def slab_gemm(name, tile, K, N, S):
        g = _gen(name)
        x, dy = _randn(g, (T, K), BF16), _randn(g, (T, N), BF16)
        slabs = torch.full((S, K, N), float("nan"), dtype=F32, device=DEV)
        hip.gemm(x, dy, slabs, K, N, T, K, N, N, False, False, sC=K * N, splitk=S, tile=tile, slabs=True)
        return slabs
    for tile in (1282, 12883, 12884):
        name = f"gemm/slab/{tile}/{K}x{N}x{T}s{S}"
        slabs = slab_gemm(name, tile, K, N, S)
        out.record(name)
        out.add(name + "/slabs", slabs)
    hip.gemm_group_begin()                            # test_gemm_grouped_pair_instance
    pair = [slab_gemm(f"gemm/group/{i}", 1282, k, n, s) for i, (k, n, s) in enumerate(((136, 72, 3), (72, 200, 2)))]
    hip.gemm_group_end(pair[0])
    out.record("gemm/group")
    for i, slabs in enumerate(pair):
        out.add(f"gemm/group/{i}/slabs", slabs)
    # the fused projection's weight-major 3-batch, folded into one 256x192 GEMM
    name, (M, N, K) = "gemm/fold/2562/1000x512x640b3", (1000, 512, 640)
    g = _gen(name)
    x, wt = _randn(g, (M, K), BF16), _randn(g, (3, N, K), BF16, 0.05)
    C = torch.full((M, 3 * N), float("nan"), dtype=BF16, device=DEV)
    psum = torch.zeros(hip.psum_slots(M, N, 3), dtype=F32, device=DEV)
    cnt = hip.gemm(x, wt, C, M, N, K, K, K, 3 * N, True, True, batch=3, sA=0, sB=N * K, sC=N, tile=2562, psum=psum)
    out.record(name)
    out.add(name + "/C", C)
    out.add(name + "/psum", psum[:cnt])
    # whole rounds of 2 blocks per CU on 256 CUs: the persistent grid
    _gemm(out, "gemm/persistent/1282/4096x4096x64", 1282, 1, 1, 0, 4096, 4096, 64)
    _gemm(out, "gemm/atomics/1282/320x128x2048s4", 1282, 0, 0, 1, 320, 128, 2048, hashed=False, splitk=4, zero_c=True)


def mx_cases(out):
    """fp8.hip's MX GEMM launcher on the cases of tests/test_fp8_gemm_oracle_gpu.py (constructed
    operands of tests/gemm_oracle.py mx_case): every tile code x {f32, bf16 + bias + ReLU}, the split,
    the broadcast operands, residual and masks, the MX copies, the fused column sums and the two
    copies-only calls of the FF block (FIX 1 / 2)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import gemm_oracle as O
    import test_fp8_picks as P
    from learning_jax_sharding_amd.ops import fp8

    def run(name, c, M, N, K, odt, tile, nsplit=1, copies=False, colsum_rows=0, **kw):
        ops = [c[n].to(DEV) for n in ("qa", "sa", "qb", "sb")]
        bias = None if c["bias"] is None else c["bias"].to(DEV)
        res = None if c["res"] is None else c["res"].to(DEV)
        C = None if odt is None else torch.full((nsplit, M, N), float("nan"), dtype=odt, device=DEV)
        if copies:
            q = [torch.full(s, 0xAB, dtype=torch.uint8, device=DEV) for s in ((M, N), (M, N // 32), (N, M), (N, M // 32))]
            kw.update(qout=(q[0], q[1]), qtout=(q[2], q[3]))
        if colsum_rows:
            kw["colsum"] = torch.full((colsum_rows, N), float("nan"), device=DEV)
        fp8.gemm_mx(*ops, M, N, K, None if C is None else (C if nsplit > 1 else C[0]), bias=bias, res=res,
                    res_mode=c["res_mode"], tile=tile, nsplit=nsplit, **kw)
        if C is not None:
            out.add(name + "/C", C)
        for k, t in zip(("QC", "SC", "QT", "ST"), q if copies else ()):
            out.add(f"{name}/{k}", t)
        if colsum_rows:
            out.add(name + "/colsum", kw["colsum"])

    for tile, (_, bm, bn, _, _) in P.MX_TILES.items():
        M, N = bm + 8, bn + 8
        for K in (128, 384):
            run(f"mx/tile/{tile}/f32/{M}x{N}x{K}", O.mx_case(M, N, K, seed=tile % 977 + K), M, N, K, F32, tile)
            c = O.mx_case(M, N, K, bias=True, relu=True, out=BF16, seed=tile % 977 + K)
            run(f"mx/tile/{tile}/bf16-bias-relu/{M}x{N}x{K}", c, M, N, K, BF16, tile, relu=True)
    for tile in (1282, 256160):
        bm, bn = P.MX_TILES[tile][1:3]
        M, N = bm + 8, bn + 8
        run(f"mx/split/{tile}", O.mx_case(M, N, 384, nsplit=2, seed=tile % 977), M, N, 384, F32, tile, nsplit=2)
        for which in ("a_bcast", "b_bcast"):
            c = O.mx_case(M, N, 384, seed=tile % 977 + 1, **{which: True})
            run(f"mx/{which}/{tile}", c, M, N, 384, F32, tile, **{which: True})
        for mode, kind in (("add", "bf16"), ("mask", "bf16"), ("mask", "e4m3")):
            c = O.mx_case(M, N, 128, bias=True, out=BF16, res=(mode, kind), seed=tile % 977 + 2)
            run(f"mx/res/{tile}/{mode}-{kind}", c, M, N, 128, BF16, tile)
        M, N = bm + 32, bn + 32
        c = O.mx_case(M, N, 128, bias=True, relu=True, out=BF16, seed=tile % 977 + 3)
        run(f"mx/copies/{tile}", c, M, N, 128, BF16, tile, relu=True, copies=True)
    M, N = 256 + 8, 160 + 8
    run("mx/colsum/256160", O.mx_case(M, N, 128, lo=-2, hi=2, out=BF16, seed=7), M, N, 128, BF16, 256160, colsum_rows=2)
    for fix, K in ((1, 128), (1, 384), (2, 128), (2, 384)):
        c = O.mx_case(160, 160, K, relu=fix == 1, out=BF16, res=("mask", "e4m3") if fix == 2 else None, seed=fix + K)
        run(f"mx/fix{fix}/160x160x{K}", c, 160, 160, K, None, 1282, relu=fix == 1, copies=True)


GROUPS = {"gemm": gemm_cases, "mx": mx_cases, "norm": norm_cases, "xent": xent_cases, "sum": sum_cases, "colsum": colsum_cases, "mse": mse_cases,
          "misc": misc_cases}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default="", help="also write {case: sha256} here")
    ap.add_argument("--grep", default="", help="only the groups whose name contains this")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kernel_digest: no GPU")
    out = Out()
    for name, fn in GROUPS.items():
        if a.grep in name:
            fn(out)
    torch.cuda.synchronize()
    print(f"# {len(out.lines)} outputs, library {hip._LIBPATH}", file=sys.stderr)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(out.lines), f, indent=1)


if __name__ == "__main__":
    main()
