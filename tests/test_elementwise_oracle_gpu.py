"""The elementwise, reduction and MSE HIP kernels (csrc/kernels/elementwise.hip, loss.hip) against the exact oracle
of tests/elementwise_oracle.py, instance by instance (run on a real MI355X: -m gpu).

Exact inputs are held to ``exact_budget`` and compared bit for bit; data movement and the f32 -> bf16 rounding are
compared as integers over the sweep of bit patterns; each test asserts the recorded instance and grid (the cast,
cast_transpose and swap01 launchers record into a ring of their own, ``last_launch(copies=True)``: a torch
fall-back or another ``vin`` / ``vout`` instance than the one a test names would fail it).  Inputs and outputs are views inside buffers filled with a NaN pattern: a read past an input's
end turns a sum into NaN, and every byte around an output must still hold the pattern afterwards.

What exact inputs cannot show - that rounding inside long f32 sums and in the softmax stays at the level of any
valid order - is checked on random inputs with the rule of tests/test_norm_gpu.py: ``E_ref`` is the max-abs error
of torch's f32 evaluation of the same function on the GPU against the float64 oracle; an f32 output may differ from
the oracle by ``4 E_ref + 2^-23 max|oracle|``, a bf16 output by one bf16 ulp of the rounded oracle on top."""
import ctypes

import numpy as np
import pytest
import torch

import elementwise_oracle as O

pytestmark = pytest.mark.gpu

dev = torch.device("cuda", 0)
F32, BF16 = torch.float32, torch.bfloat16
UNIT, SCALE = O.UNIT, O.MSE_SCALE
_INT = {2: (torch.int16, np.uint16, 0x7FC1), 4: (torch.int32, np.uint32, 0x7FC00001), 8: (torch.int64, np.uint64, 0x7FF8000000000001)}
_ES = {F32: 4, BF16: 2, torch.int16: 2, torch.int32: 4, torch.int64: 8}


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from learning_jax_sharding_amd.ops import hip as H
    H.lib()
    return H


# ---------------------------------------------------------------- guarded buffers
class Buf:
    """A (possibly strided) view of ``dtype`` inside a buffer whose every other element holds a NaN pattern.  ``shift``
    moves the view off the 16-byte grid by that many elements."""
    PAD = 64

    def __init__(self, shape, dtype, strides=None, shift=0, bits=None):
        shape = tuple(shape)
        if strides is None:
            strides = tuple(int(np.prod(shape[i + 1:])) for i in range(len(shape)))
        self.idt, self.udt, self.poison = _INT[_ES[dtype]]
        span = 1 + sum((s - 1) * st for s, st in zip(shape, strides)) if all(shape) else 0
        self.geom = (shape, tuple(strides), self.PAD + shift)
        self.raw = torch.full((2 * self.PAD + shift + span,), self.poison, dtype=self.idt, device=dev)
        self.ints = self.raw.as_strided(*self.geom)
        self.t = self.ints.view(dtype) if dtype != self.idt else self.ints
        if bits is not None:
            self.put(bits)

    def put(self, bits):
        a = np.ascontiguousarray(np.asarray(bits).astype(self.udt)).view(self.udt(0).dtype.str.replace("u", "i"))
        self.ints.copy_(torch.from_numpy(a.reshape(self.geom[0])))
        return self

    def bits(self):
        return self.ints.cpu().numpy().view(self.udt)

    def guards_ok(self):
        s = self.raw.clone()
        s.as_strided(*self.geom).fill_(self.poison)
        return bool((s == self.poison).all())


def _vals(k, dtype, **kw):
    """A guarded buffer holding the exact values k * UNIT."""
    x = np.asarray(k) * UNIT
    return Buf(np.shape(k), dtype, bits=O.bf16_bits_exact(x) if dtype == BF16 else O.f32_bits(x), **kw)


def _f32(v):
    return O.f32_bits(np.asarray(v, dtype=np.float64))


def _out_bits(v, dtype):
    """Bits of exact f64 values stored in ``dtype`` (bf16: rounded to nearest even)."""
    return O.rne_bf16_bits(_f32(v)) if dtype == BF16 else _f32(v)


def _rec(hip, name, grid):
    r = hip.last_launch()
    grid = tuple(grid) + (1,) * (3 - len(tuple(grid)))
    assert r["name"] == name and r["grid"] == grid and r["block"] == 256, (r, name, grid)


def _copy_launch(hip, fn, name, grid):
    """Run ``fn``: it makes exactly one launch of the casts' and layout copies' ring, of this instance and grid."""
    with hip.launch_log(copies=True) as log:
        out = fn()
    grid = tuple(grid) + (1,) * (3 - len(tuple(grid)))
    assert log.total == 1 and log[0]["name"] == name and log[0]["grid"] == grid and log[0]["block"] == 256, (list(log), name, grid)
    assert hip.last_launch(copies=True) == log[0]
    return out


def hip_stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _same(got, want, what):
    got, want = np.asarray(got).ravel(), np.asarray(want).ravel()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, bad.size, [(int(i), hex(int(want[i])), hex(int(got[i]))) for i in bad[:4]])


def _dt(is_bf16):
    return BF16 if is_bf16 else F32


_TAG = {F32: "f32", BF16: "bf16", torch.float64: "f32-sum"}


# ================================================================ sum_all, sum_partials
def _sum_all(hip, x, n, is_bf16, out_dtype, aligned=True):
    out = Buf((1,), out_dtype)
    ws = hip._workspace(dev, "sum_all", 1089 * 4)
    rc = hip.lib().ljs_sum_all(_p(x), int(is_bf16), n, _p(out.t), int(out_dtype == BF16), _p(ws), hip_stream(x))
    assert rc == 0
    kind, g = O.sum_all_grid(n, is_bf16, aligned)
    _rec(hip, f"sum_all<{_TAG[_dt(is_bf16)]},{kind}>", (g,))
    assert out.guards_ok()
    return out.bits()[0]


@pytest.mark.parametrize("out_dtype", [F32, BF16], ids=["out_f32", "out_bf16"])
@pytest.mark.parametrize("is_bf16", [True, False], ids=["bf16", "f32"])
def test_sum_all_exact(hip, is_bf16, out_dtype):
    V = O.sum_all_v(is_bf16)
    for n in O.sum_all_dense_ns(is_bf16):
        k = O.planted(1, n, V)[0]
        O.exact_budget(k * UNIT, UNIT)
        x = _vals(k, _dt(is_bf16))
        got = _sum_all(hip, x.t, n, is_bf16, out_dtype)
        assert got == _out_bits(int(k.sum()) * UNIT, out_dtype), (n, hex(int(got)), int(k.sum()))


@pytest.mark.parametrize("is_bf16", [True, False], ids=["bf16", "f32"])
def test_sum_all_sparse_1024_blocks_and_two_unrolled_rounds(hip, is_bf16):
    V = O.sum_all_v(is_bf16)
    for n in O.sum_all_sparse_ns(is_bf16):
        idx, k = O.sparse(n, 64, V)
        O.exact_budget(k * UNIT, UNIT)
        x = Buf((n,), _dt(is_bf16))
        x.t.zero_()
        x.t[torch.from_numpy(idx).to(dev)] = torch.from_numpy(k * UNIT).to(dev, _dt(is_bf16))
        assert O.sum_all_grid(n, is_bf16)[1] == 1024
        for out_dtype in (F32, BF16):
            got = _sum_all(hip, x.t, n, is_bf16, out_dtype)
            assert got == _out_bits(int(k.sum()) * UNIT, out_dtype), (n, hex(int(got)), int(k.sum()))
        del x


@pytest.mark.parametrize("is_bf16", [True, False], ids=["bf16", "f32"])
def test_sum_all_unaligned_base_takes_the_atomic_kernel(hip, is_bf16):
    V = O.sum_all_v(is_bf16)
    for shift, n in O.SUM_ALL_UNALIGNED:
        k = O.planted(1, n, V)[0]
        O.exact_budget(k * UNIT, UNIT)
        x = _vals(k, _dt(is_bf16), shift=shift)
        assert x.t.data_ptr() % 16 != 0
        got = _sum_all(hip, x.t, n, is_bf16, F32, aligned=False)
        assert got == _f32(int(k.sum()) * UNIT), (n, hex(int(got)))
        out = torch.empty((), dtype=BF16, device=dev)       # a bf16 result needs the ticket kernel: refused, not faked
        rc = hip.lib().ljs_sum_all(_p(x.t), int(is_bf16), n, _p(out), 1, _p(hip._workspace(dev, "sum_all", 1089 * 4)),
                                   hip_stream(out))
        assert rc != 0


def test_sum_all_rearms_its_workspace_across_grid_sizes(hip):
    tg = O.ticket_group()
    xs = {}
    for n in O.sum_all_rearm_ns():
        idx, k = O.sparse(n, 16)
        O.exact_budget(k * UNIT, UNIT)
        x = Buf((n,), BF16)
        x.t.zero_()
        x.t[torch.from_numpy(idx).to(dev)] = torch.from_numpy(k * UNIT).to(dev, BF16)
        xs[O.sum_all_grid(n, True)[1]] = (x, n, _f32(int(k.sum()) * UNIT))
    assert list(xs) == [tg + 1, 1, 2, tg, 3 * tg + 5]
    for rnd in range(3):
        for g, (x, n, want) in xs.items():
            assert _sum_all(hip, x.t, n, True, F32) == want, (rnd, g)
    ws = hip._workspace(dev, "sum_all", 1089 * 4)
    assert not ws.view(torch.int32)[1024 + tg:1089].any()       # every ticket word is zero at rest


@pytest.mark.parametrize("out_dtype", [F32, BF16], ids=["out_f32", "out_bf16"])
def test_sum_partials_exact(hip, out_dtype):
    for n in O.SUM_PARTIALS_N:
        k = O.planted(1, n, 4)[0]
        O.exact_budget(k * UNIT, UNIT)
        p, out = _vals(k, F32), Buf((1,), out_dtype)
        assert hip.lib().ljs_sum_partials(_p(p.t), n, _p(out.t), int(out_dtype == BF16), hip_stream(p.t)) == 0
        _rec(hip, "sum_partials", (1,))
        assert out.bits()[0] == _out_bits(int(k.sum()) * UNIT, out_dtype), n
        assert out.guards_ok()


# ================================================================ column sums
def _colsum_case(hip, dtype, R, C, ld, accumulate, col0=0):
    k = O.planted(R, C)
    O.exact_budget(k * UNIT, UNIT)
    x = _vals(k, dtype, strides=(ld, 1), shift=col0)
    base = np.arange(C, dtype=np.int64) % 7 - 3
    out = Buf((C,), F32, bits=_f32(base * UNIT))
    hip.colsum(x.t, out=out.t, accumulate=accumulate)
    name, grid = O.colsum_plan(dtype == BF16, R, C, ld, aligned=x.t.data_ptr() % 16 == 0)
    _rec(hip, name, grid)
    _same(out.bits(), _f32((k.sum(0) + (base if accumulate else 0)) * UNIT), (name, R, C, ld, accumulate))
    assert out.guards_ok()
    return name


@pytest.mark.parametrize("R,C", O.COLSUM_TICKET, ids=[f"{R}x{C}" for R, C in O.COLSUM_TICKET])
def test_colsum_ticket_exact(hip, R, C):
    assert _colsum_case(hip, BF16, R, C, C, False) == "colsum<ticket>"
    assert _colsum_case(hip, BF16, R, C, C + 24, True, col0=8) == "colsum<ticket>"      # a column slice, ld > C


def _deep(R, C):
    """The sparse exact input of a deep ticket shape: (row, column, k) of its non-zero entries."""
    idx, k = O.sparse(R * C, O.COLSUM_DEEP_EVERY)
    O.exact_budget(k * UNIT, UNIT)
    return idx // C, idx % C, k


def _put_sparse(buf, r, c, k):
    buf.t.zero_()
    buf.t[torch.from_numpy(r).to(dev), torch.from_numpy(c).to(dev)] = torch.from_numpy(k * UNIT).to(dev, BF16)


@pytest.mark.parametrize("R,C", O.COLSUM_TICKET_DEEP, ids=[f"{R}x{C}" for R, C in O.COLSUM_TICKET_DEEP])
def test_colsum_ticket_rows_in_flight_loop_exact(hip, R, C):
    """More than 96 rows per block: the 4-rows-in-flight loop runs (tests/test_elementwise_oracle.py states how often)."""
    r, c, k = _deep(R, C)
    x = Buf((R, C), BF16, strides=(C + 8, 1))
    _put_sparse(x, r, c, k)
    want = np.zeros(C, dtype=np.int64)
    np.add.at(want, c, k)
    for acc in (False, True):
        base = np.arange(C, dtype=np.int64) % 7 - 3
        out = Buf((C,), F32, bits=_f32(base * UNIT))
        hip.colsum(x.t, out=out.t, accumulate=acc)
        _rec(hip, *O.colsum_plan(True, R, C, C + 8))
        assert hip.last_launch()["name"] == "colsum<ticket>"
        _same(out.bits(), _f32((want + (base if acc else 0)) * UNIT), (R, C, acc))
        assert out.guards_ok()


@pytest.mark.parametrize("tag,R,C,ld", O.COLSUM_GENERIC, ids=[f"{t}-{R}x{C}-ld{ld}" for t, R, C, ld in O.COLSUM_GENERIC])
def test_colsum_generic_exact(hip, tag, R, C, ld):
    for acc in (False, True):
        assert _colsum_case(hip, BF16 if tag == "bf16" else F32, R, C, ld, acc) == f"colsum<{tag}>"


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_colsum_bcast_exact(hip, dtype):
    for R, C in O.COLSUM_BCAST:
        k = O.planted(1, C)[0]
        O.exact_budget(k * R * UNIT, UNIT)
        row = _vals(k, dtype)
        base = np.arange(C, dtype=np.int64) % 5
        out = Buf((C,), F32, bits=_f32(base * UNIT))
        hip.colsum_ld(row.t, R, C, 0, out=out.t)                 # out given: accumulates
        _rec(hip, "colsum<bcast>", O.colsum_plan(dtype == BF16, R, C, 0)[1])
        _same(out.bits(), _f32((k * R + base) * UNIT), (R, C))
        assert out.guards_ok()
        ws = hip._workspace(dev, "colsum", 4 << 20)
        rc = hip.lib().ljs_colsum(_p(row.t), int(dtype == BF16), R, C, 0, _p(out.t), 0, _p(ws), hip_stream(out.t))
        assert rc == 0
        _same(out.bits(), _f32(k * R * UNIT), (R, C, "overwrite"))
        assert out.guards_ok()


def test_colsum_vec_without_a_workspace_exact(hip):
    R, C, ld = O.COLSUM_VEC
    k = O.planted(R, C)
    O.exact_budget(k * UNIT, UNIT)
    x, out = _vals(k, BF16, strides=(ld, 1)), Buf((C,), F32)
    for acc, base in ((0, 0), (1, k.sum(0))):
        rc = hip.lib().ljs_colsum(_p(x.t), 1, R, C, ld, _p(out.t), acc, None, hip_stream(out.t))
        assert rc == 0
        _rec(hip, *O.colsum_plan(True, R, C, ld, ws=False))
        assert hip.last_launch()["name"] == "colsum<vec>"
        _same(out.bits(), _f32((k.sum(0) + base) * UNIT), acc)
        assert out.guards_ok()


def test_rows_sum_exact(hip):
    for R in O.ROWS_SUM_R:
        for C in O.ROWS_SUM_C:
            k = O.planted(R, C)
            O.exact_budget(k * UNIT, UNIT)
            x, out = _vals(k, F32, strides=(C + 3, 1)), Buf((C,), F32)
            hip.rows_sum(x.t, out=out.t)
            _rec(hip, "rows_sum_f32", ((C + 63) // 64,))
            _same(out.bits(), _f32(k.sum(0) * UNIT), (R, C))
            assert out.guards_ok()


# ================================================================ sum_n, slab_reduce
@pytest.mark.parametrize("is_bf16", [True, False], ids=["bf16", "f32"])
def test_sum_n_exact(hip, is_bf16):
    V, dtype = O.sum_all_v(is_bf16), _dt(is_bf16)
    for n in O.SUM_N_N:
        for count in O.sum_n_counts(is_bf16):
            k = O.planted(n, count, V)
            O.exact_budget(k * UNIT, UNIT)
            pitch = (count + V - 1) // V * V + V             # every row 16-byte aligned, a chunk of poison between rows
            x, out = _vals(k, dtype, strides=(pitch, 1)), Buf((count,), dtype)
            hip.sum_n([x.t[i] for i in range(n)], out=out.t)
            _rec(hip, f"sum_n<{_TAG[dtype]}>", (min(2048, (count // V + 1 + 255) // 256),))
            _same(out.bits(), _out_bits(k.sum(0) * UNIT, dtype), (n, count))
            assert out.guards_ok()


@pytest.mark.parametrize("slab_bf16", [False, True], ids=["f32", "bf16"])
def test_slab_reduce_exact(hip, slab_bf16):
    R, C, cb = 3, 8, 4
    out_bs = R * cb + 8
    for S in O.SLAB_S:
        for acc, tail_n in ((False, 0), (True, 1), (False, 300)):
            k = O.planted(S * R, C, 4).reshape(S, R, C)
            O.exact_budget(k * UNIT, UNIT)
            slabs = _vals(k, _dt(slab_bf16))
            base = (np.arange(2 * R * cb, dtype=np.int64) % 9 - 4).reshape(2, R, cb)
            out = Buf((2, R, cb), F32, strides=(out_bs, cb, 1), bits=_f32(base * UNIT))
            twin = Buf((2, R, cb), BF16, strides=(out_bs, cb, 1))
            tail, tail16 = Buf((tail_n,), F32), Buf((tail_n,), BF16)
            hip.slab_reduce(slabs.t, out.t, cb, out_bs, accumulate=acc, out_bf16=twin.t,
                            tail=tail.t if tail_n else None, tail_bf16=tail16.t if tail_n else None, tail_val=3.14159)
            _rec(hip, f"slab_reduce<{_TAG[_dt(slab_bf16)]}>", (O.slab_reduce_grid(R, C),))
            want = k.sum(0).reshape(R, 2, cb).transpose(1, 0, 2) + (base if acc else 0)
            _same(out.bits(), _f32(want * UNIT), (S, acc))
            _same(twin.bits(), O.rne_bf16_bits(_f32(want * UNIT)), (S, acc, "bf16 twin"))
            _same(tail.bits(), np.full(tail_n, _f32(np.float32(3.14159))), "tail")
            _same(tail16.bits(), np.full(tail_n, O.rne_bf16_bits(_f32(np.float32(3.14159)))), "tail bf16")
            assert out.guards_ok() and twin.guards_ok() and tail.guards_ok() and tail16.guards_ok()


def test_slab_reduce_above_the_grid_cap(hip):
    R, C = O.SLAB_BIG
    idx, k = O.sparse(2 * R * C, 64, 4)
    O.exact_budget(k * UNIT, UNIT)
    slabs = Buf((2, R, C), F32)
    slabs.t.zero_()
    slabs.t.view(-1)[torch.from_numpy(idx).to(dev)] = torch.from_numpy(k * UNIT).to(dev, F32)
    out = Buf((R, C), F32)
    hip.slab_reduce(slabs.t, out.t, C, R * C)
    _rec(hip, "slab_reduce<f32>", (2048,))
    want = np.zeros(2 * R * C, dtype=np.int64)
    want[idx] = k
    _same(out.bits(), _f32(want.reshape(2, -1).sum(0) * UNIT), "big")
    assert out.guards_ok()


# ================================================================ ReLU backward
_MASKS = np.array([0x0000, 0x8000, 0x3F80, 0xBF80, 0x0001, 0x8001, 0x7F80, 0xFF80, 0x0080, 0x7F7F, 0x3C00], dtype=np.uint16)


@pytest.mark.parametrize("R,C", O.COLSUM_TICKET, ids=[f"{R}x{C}" for R, C in O.COLSUM_TICKET])
def test_relu_bwd_exact(hip, R, C):
    k = O.planted(R, C)
    O.exact_budget(k * UNIT, UNIT)
    r, c = np.arange(R)[:, None], np.arange(C)[None, :]
    mbits = _MASKS[(r * 3 + c * 5 + c // 8) % _MASKS.size]
    keep = O.relu_keep(mbits)
    dy, mask = _vals(k, BF16, strides=(C + 8, 1)), Buf((R, C), BF16, strides=(C + 16, 1), bits=mbits)
    want = np.where(keep, O.bf16_bits_exact(k * UNIT), 0)
    masked, db = Buf((R, C), BF16), Buf((C,), F32)
    ws = hip._workspace(dev, "colsum", 4 << 20)
    L = hip.lib()
    assert L.ljs_relu_bwd_colsum(_p(dy.t), _p(mask.t), R, C, C + 8, C + 16, _p(masked.t), _p(db.t), _p(ws), hip_stream(db.t)) == 0
    _rec(hip, "relu_bwd_colsum", O.relu_bwd_colsum_grid(R, C))
    _same(masked.bits(), want, "masked")
    _same(db.bits(), _f32((k * keep).sum(0) * UNIT), "db")
    assert masked.guards_ok() and db.guards_ok()
    masked2 = Buf((R, C), BF16)
    assert L.ljs_relu_bwd(_p(dy.t), _p(mask.t), R, C, C + 8, C + 16, _p(masked2.t), hip_stream(db.t)) == 0
    _rec(hip, "relu_bwd", (O.relu_bwd_grid(R, C),))
    _same(masked2.bits(), want, "relu_bwd")
    assert masked2.guards_ok()


@pytest.mark.parametrize("R,C", O.COLSUM_TICKET_DEEP, ids=[f"{R}x{C}" for R, C in O.COLSUM_TICKET_DEEP])
def test_relu_bwd_rows_in_flight_loop_exact(hip, R, C):
    """The masked 4-rows-in-flight loop (it also stores masked_out), with mld != ld."""
    r, c, k = _deep(R, C)
    dy = Buf((R, C), BF16, strides=(C + 8, 1))
    _put_sparse(dy, r, c, k)
    rr, cc = np.arange(R)[:, None], np.arange(C)[None, :]
    mbits = _MASKS[(rr * 3 + cc * 5 + cc // 8) % _MASKS.size]
    mask = Buf((R, C), BF16, strides=(C + 16, 1), bits=mbits)
    keep = O.relu_keep(mbits[r, c])
    want = np.zeros((R, C), dtype=np.uint16)
    want[r, c] = np.where(keep, O.bf16_bits_exact(k * UNIT), 0)
    wdb = np.zeros(C, dtype=np.int64)
    np.add.at(wdb, c[keep], k[keep])
    assert keep.any() and not keep.all()
    masked, db = Buf((R, C), BF16), Buf((C,), F32)
    ws = hip._workspace(dev, "colsum", 4 << 20)
    L = hip.lib()
    assert L.ljs_relu_bwd_colsum(_p(dy.t), _p(mask.t), R, C, C + 8, C + 16, _p(masked.t), _p(db.t), _p(ws), hip_stream(db.t)) == 0
    _rec(hip, "relu_bwd_colsum", O.relu_bwd_colsum_grid(R, C))
    _same(masked.bits(), want, "masked")
    _same(db.bits(), _f32(wdb * UNIT), "db")
    assert masked.guards_ok() and db.guards_ok()


def test_relu_mask_rule_on_every_bf16_pattern(hip):
    """All 65 536 mask patterns: kept iff the sign bit is clear and the magnitude bits are not zero, positive-sign NaNs
    included (a float comparison would drop those 127)."""
    R, C = 1024, 64
    mbits = np.arange(1 << 16, dtype=np.uint16).reshape(R, C)
    dyb = np.array([0x3F80, 0xBF80, 0x7FC1, 0x0001, 0xFFFF, 0x8000, 0x7F80], dtype=np.uint16)[(np.arange(R * C) * 3 // 2) % 7].reshape(R, C)
    want = np.where(O.relu_keep(mbits), dyb, 0)
    assert (want.ravel()[0x7F81:0x8000] == dyb.ravel()[0x7F81:0x8000]).all()
    dy, mask = Buf((R, C), BF16, bits=dyb), Buf((R, C), BF16, bits=mbits)
    masked, masked2, db = Buf((R, C), BF16), Buf((R, C), BF16), Buf((C,), F32)
    ws = hip._workspace(dev, "colsum", 4 << 20)
    L = hip.lib()
    assert L.ljs_relu_bwd_colsum(_p(dy.t), _p(mask.t), R, C, C, C, _p(masked.t), _p(db.t), _p(ws), hip_stream(db.t)) == 0
    _rec(hip, "relu_bwd_colsum", O.relu_bwd_colsum_grid(R, C))
    assert L.ljs_relu_bwd(_p(dy.t), _p(mask.t), R, C, C, C, _p(masked2.t), hip_stream(db.t)) == 0
    _rec(hip, "relu_bwd", (O.relu_bwd_grid(R, C),))
    _same(masked.bits(), want, "relu_bwd_colsum")
    _same(masked2.bits(), want, "relu_bwd")
    assert masked.guards_ok() and masked2.guards_ok() and db.guards_ok()


# ================================================================ MSE
def _mse_want(ky, kt):
    d = (ky - kt).astype(np.int64)
    O.exact_budget(d * d * UNIT * UNIT, UNIT * UNIT)
    O.exact_budget(2 * SCALE * d * UNIT, 2 * SCALE * UNIT)
    loss = _f32(SCALE * int((d * d).sum()) * UNIT * UNIT)
    return d, loss, O.bf16_bits_exact(2 * SCALE * d * UNIT)


def _mse_raw(hip, y, t, n, tgt_bf16, want_dy):
    dy, out = Buf((n,), BF16), Buf((1,), F32)
    ws = hip._workspace(dev, "mse", (1024 + 33) * 4)
    rc = hip.lib().ljs_mse_loss(_p(y), _p(t), int(tgt_bf16), n, SCALE, _p(dy.t) if want_dy else None, _p(out.t), _p(ws),
                                hip_stream(y))
    assert rc == 0
    _rec(hip, "mse<" + ("tbf16" if tgt_bf16 else "tf32") + (",dy>" if want_dy else ">"), (O.mse_grid(n),))
    assert out.guards_ok() and dy.guards_ok()
    return out.bits()[0], dy.bits()


@pytest.mark.parametrize("want_dy", [True, False], ids=["dy", "nody"])
@pytest.mark.parametrize("tgt_bf16", [True, False], ids=["tbf16", "tf32"])
def test_mse_exact_with_tails(hip, tgt_bf16, want_dy):
    for n in O.MSE_DENSE_N:
        ky, kt = O.mse_inputs(1, n)
        d, loss, dyb = _mse_want(ky[0], kt[0])
        y, t = _vals(ky[0], BF16), _vals(kt[0], _dt(tgt_bf16))
        got_loss, got_dy = _mse_raw(hip, y.t, t.t, n, tgt_bf16, want_dy)
        assert got_loss == loss, (n, hex(int(got_loss)), hex(int(loss)))
        _same(got_dy, dyb if want_dy else np.full(n, 0x7FC1), (n, "dy"))


@pytest.mark.parametrize("tgt_bf16", [True, False], ids=["tbf16", "tf32"])
def test_mse_sparse_1024_blocks_and_beyond(hip, tgt_bf16):
    for n in O.MSE_SPARSE_N:
        idx, k = O.sparse(n, 64)
        kd = k % 8
        O.exact_budget(kd * kd * UNIT * UNIT, UNIT * UNIT)
        y, t = Buf((n,), BF16), Buf((n,), _dt(tgt_bf16))
        y.t.zero_()
        t.t.zero_()
        t.t[torch.from_numpy(idx).to(dev)] = torch.from_numpy(-kd * UNIT).to(dev, _dt(tgt_bf16))
        got_loss, got_dy = _mse_raw(hip, y.t, t.t, n, tgt_bf16, True)
        assert got_loss == _f32(SCALE * int((kd * kd).sum()) * UNIT * UNIT), n
        want = np.zeros(n, dtype=np.uint16)
        want[idx] = O.bf16_bits_exact(2 * SCALE * kd * UNIT)
        _same(got_dy, want, (n, "dy"))
        del y, t


def _mse_colsum(hip, R, C, tgt_bf16, kmax=7):
    ky, kt = O.mse_inputs(R, C, kmax)
    d, loss, dyb = _mse_want(ky, kt)
    y, t = _vals(ky, BF16), _vals(kt, _dt(tgt_bf16))
    dy, sums, out = Buf((R, C), BF16), Buf((C,), F32), Buf((1,), F32)
    L = hip.lib()
    plan = O.mse_colsum_plan(R, C)
    assert L.ljs_mse_colsum_ws_bytes(R, C) == 4 * plan["words"]
    ws = hip._workspace(dev, f"mse_colsum/{R}x{C}", 4 * plan["words"])
    rc = L.ljs_mse_colsum(_p(y.t), _p(t.t), int(tgt_bf16), R, C, SCALE, _p(dy.t), _p(sums.t), _p(out.t), _p(ws),
                          hip_stream(y.t))
    assert rc == 0
    _rec(hip, "mse_colsum<" + ("tbf16>" if tgt_bf16 else "tf32>"), (plan["cb"], plan["gy"]))
    assert out.bits()[0] == loss, (R, C, hex(int(out.bits()[0])), hex(int(loss)))
    _same(dy.bits(), dyb, (R, C, "dy"))
    _same(sums.bits(), _f32(2 * SCALE * d.sum(0) * UNIT), (R, C, "colsum"))
    assert dy.guards_ok() and sums.guards_ok() and out.guards_ok()
    nt = plan["cb"] + 1 + (plan["cb"] * plan["gy"] + 31) // 32
    assert not ws.view(torch.int32)[:nt].any()                    # tickets re-armed


@pytest.mark.parametrize("tgt_bf16", [True, False], ids=["tbf16", "tf32"])
@pytest.mark.parametrize("C", O.MSE_COLSUM_C)
def test_mse_colsum_exact(hip, C, tgt_bf16):
    for R in O.MSE_COLSUM_R:
        _mse_colsum(hip, R, C, tgt_bf16)


def test_mse_colsum_above_512_blocks_and_alternating_geometries(hip):
    _mse_colsum(hip, *O.MSE_COLSUM_BIG, tgt_bf16=False, kmax=1)
    for _ in range(3):
        _mse_colsum(hip, 97, 64, True)
        _mse_colsum(hip, 193, 128, False)


def test_mse_loss_wrapper_on_a_seq_major_prediction(hip):
    B, S, C = 3, 33, 64
    ky, kt = O.mse_inputs(B * S, C)
    d, loss, dyb = _mse_want(ky, kt)
    # y is [B][S][C] stored seq-major; the oracle's rows are the storage rows (s, b)
    ysb = torch.from_numpy((ky * UNIT).astype(np.float32)).to(dev, BF16).reshape(S, B, C)
    tsb = torch.from_numpy((kt * UNIT).astype(np.float32)).to(dev).reshape(S, B, C)
    y = ysb.transpose(0, 1).requires_grad_(True)
    t = tsb.transpose(0, 1).contiguous()
    with hip.launch_log() as log:
        out = hip.mse_loss(y, t, SCALE)
        (gy,) = torch.autograd.grad(out, y, torch.tensor(1.0, device=dev))
    p = O.mse_colsum_plan(B * S, C)
    recs = [r for r in log if r["name"].startswith("mse")]
    assert [(r["name"], r["grid"]) for r in recs] == [("mse_colsum<tf32>", (p["cb"], p["gy"], 1))], list(log)
    assert out.view(torch.int32).item() == int(loss.view(np.int32))
    got = gy.transpose(0, 1).contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    _same(got, dyb, "gy")


# ================================================================ data movement: bit patterns, NaN payloads included
def _patterns(shape, seed):
    return np.random.default_rng(seed).integers(0, 1 << 16, size=shape, dtype=np.uint16)


def test_transpose_bf16_moves_every_bit(hip):
    for R in (1, 63, 64, 65, 200):
        for C in (1, 63, 64, 65, 200):
            for pad in (8, 3):            # 8: the 16-byte path where R, C are multiples of 8; 3: the scalar path
                src = _patterns((R, C), R * 1000 + C)
                x, out = Buf((R, C), BF16, strides=(C + pad, 1), bits=src), Buf((C, R), BF16, strides=(R + pad, 1))
                hip.transpose_bf16(x.t, out=out.t)
                _rec(hip, "transpose_bf16", ((C + 63) // 64, (R + 63) // 64))
                _same(out.bits(), src.T, (R, C, pad))
                assert out.guards_ok()


def test_swap01_bf16_moves_every_bit(hip):
    # B and S through 1, 63, 64, 65 and 200; (65, 2, 2048): more chunks per output row than the 64-block grid covers at once
    for B, S, K in ((1, 1, 8), (63, 64, 8), (64, 63, 72), (65, 200, 8), (200, 65, 64), (1, 200, 72), (200, 1, 8), (65, 2, 2048)):
        src = _patterns((B, S, K), B + S + K)
        x, out = Buf((B, S, K), BF16, bits=src), Buf((S, B, K), BF16)
        grid = (min(64, (B * K // 8 + 255) // 256), S)
        rc = _copy_launch(hip, lambda: hip.lib().ljs_swap01_bf16(_p(x.t), 1, _p(out.t), B, S, K, hip_stream(x.t)), "swap01<bf16>", grid)
        assert rc == 0
        _same(out.bits(), src.transpose(1, 0, 2), (B, S, K))
        assert out.guards_ok()


def _pad_box(hip, dtype, full, lo, size, sstrides=None):
    es = _ES[dtype]
    udt = _INT[es][1]
    rng = np.random.default_rng(sum(full) + es)
    src_bits = rng.integers(1, 1 << 15, size=size).astype(udt) * udt(0x0101 if es > 2 else 1)
    src = Buf(size, dtype, strides=sstrides, bits=src_bits)
    out = Buf(full, dtype)
    nd = len(full)
    arr = lambda v: (ctypes.c_long * nd)(*[int(x) for x in v])  # noqa: E731
    rc = hip.lib().ljs_pad_box(_p(src.t), _p(out.t), nd, arr(full), arr(lo), arr(size), arr(src.geom[1]), es, hip_stream(out.t))
    assert rc == 0
    total = int(np.prod(full))
    _rec(hip, f"pad_box<{es}>", (min(4096, (total + 255) // 256),))
    want = np.zeros(full, dtype=udt)
    want[tuple(slice(a, a + s) for a, s in zip(lo, size))] = src_bits
    _same(out.bits(), want, (full, lo, size))
    assert out.guards_ok()


@pytest.mark.parametrize("dtype", [torch.int16, torch.int32, torch.int64], ids=["2", "4", "8"])
def test_pad_box_exact(hip, dtype):
    _pad_box(hip, dtype, (1000,), (37,), (300,), sstrides=(3,))                       # a vector from a strided source
    _pad_box(hip, dtype, (1000,), (0,), (1000,))                                        # the full box
    _pad_box(hip, dtype, (1000,), (500,), (0,))                                         # an empty box
    for lo in ((0, 0, 0), (2, 3, 4)):                                                   # touching each low / high face
        _pad_box(hip, dtype, (5, 7, 9), lo, (3, 4, 5), sstrides=(40, 6, 1))
    _pad_box(hip, dtype, (5, 7, 9), (0, 0, 0), (5, 7, 9))
    _pad_box(hip, dtype, (2, 3, 2, 3, 4, 5), (1, 0, 0, 1, 2, 0), (1, 3, 1, 2, 2, 5))
    _pad_box(hip, dtype, (2, 3, 2, 3, 4, 5), (0, 1, 1, 0, 0, 3), (2, 2, 1, 3, 3, 2))


# ================================================================ the rounding sweep through every rounding kernel
@pytest.fixture(scope="module")
def sweep():
    bits = O.sweep_bits()
    return bits, O.rne_bf16_bits(bits)


def test_cast_f32_bf16_rounds_the_sweep(hip, sweep):
    bits, want = sweep
    x, out = Buf(bits.shape, F32, bits=bits), Buf(bits.shape, BF16)
    _copy_launch(hip, lambda: hip._cast_raw(x.t, BF16, out=out.t), "cast<f32,bf16>", (min(2048, (bits.size + 2047) // 2048),))
    O.assert_bf16_bits(out.bits(), want, "cast sweep")
    assert out.guards_ok()
    f32max = np.flatnonzero(bits == O.F32_MAX)[0]
    assert out.bits()[f32max] == O.BF16_INF
    ties = np.flatnonzero((bits >> 16) == 0x3F80)[0]             # 1.0 and its lower halves: tie to even, both neighbours
    for n in list(range(1, 10)) + [15, 16, 17, 23]:              # n % 8 tails on short slices
        xs, o = Buf((n,), F32, bits=bits[ties:ties + n]), Buf((n,), BF16)
        _copy_launch(hip, lambda: hip._cast_raw(xs.t, BF16, out=o.t), "cast<f32,bf16>", (1,))
        O.assert_bf16_bits(o.bits(), want[ties:ties + n], n)
        assert o.guards_ok()


def test_cast_bf16_f32_is_exact_on_every_pattern(hip):
    src = np.arange(1 << 16, dtype=np.uint16)
    for n in (1 << 16, 13):
        x, out = Buf((n,), BF16, bits=src[-n:]), Buf((n,), F32)
        _copy_launch(hip, lambda: hip._cast_raw(x.t, F32, out=out.t), "cast<bf16,f32>", (min(2048, (n + 2047) // 2048),))
        _same(out.bits(), src[-n:].astype(np.uint32) << 16, n)
        assert out.guards_ok()


@pytest.mark.parametrize("vin,vout", [(1, 1), (1, 0), (0, 1), (0, 0)])
def test_cast_transpose_rounds_the_sweep(hip, sweep, vin, vout):
    bits, want = sweep
    R, C = 771, 511                                              # ragged against the 32 x 32 tile and the 4-wide accesses
    src, exp = np.resize(bits, R * C).reshape(R, C), np.resize(want, R * C).reshape(R, C)
    x = Buf((R, C), F32, strides=(512 if vin else 513, 1), bits=src)
    out = Buf((C, R), BF16, strides=(772 if vout else 773, 1))
    grid = ((C + 31) // 32, (R + 31) // 32)
    _copy_launch(hip, lambda: hip.cast_transpose_bf16(x.t, out=out.t), f"cast_transpose<{vin},{vout}>", grid)
    O.assert_bf16_bits(out.bits(), exp.T, (vin, vout))
    assert out.guards_ok()
    if vin:                                                      # the same strides on a base off the 16-byte grid
        x2 = Buf((R, C), F32, strides=(512, 1), shift=1, bits=src)
        _copy_launch(hip, lambda: hip.cast_transpose_bf16(x2.t, out=out.t), f"cast_transpose<0,{vout}>", grid)
        O.assert_bf16_bits(out.bits(), exp.T, (vin, vout, "unaligned"))
        assert out.guards_ok()


def test_swap01_f32_rounds_the_sweep(hip, sweep):
    bits, want = sweep
    B, S, K = 6, 64, 1024
    x, out = Buf((B, S, K), F32, bits=bits.reshape(B, S, K)), Buf((S, B, K), BF16)
    assert _copy_launch(hip, lambda: hip.lib().ljs_swap01_bf16(_p(x.t), 0, _p(out.t), B, S, K, hip_stream(x.t)), "swap01<f32>", (3, S)) == 0
    O.assert_bf16_bits(out.bits(), want.reshape(B, S, K).transpose(1, 0, 2), "swap01")
    assert out.guards_ok()


def test_bcast_scalar_and_fill_row_round_and_fill_every_element(hip, sweep):
    bits, want = sweep
    special = [np.flatnonzero(bits == b)[0] for b in (O.F32_MAX, 0x3F808000, 0x3F818000, 0x3F808001, 0x00008001, 0x7F800000,
                                                      0xFF800000, 0x7FC00000, 0x80000000, 0x4049FFFF)]
    pick = np.unique(np.concatenate([np.array(special), np.arange(0, bits.size, 4099)]))
    g32 = Buf((pick.size,), F32, bits=bits[pick])
    g16 = Buf((pick.size,), BF16, bits=want[pick])
    L, Rf = hip.lib(), 12.0
    for C in (1, 255, 256, 257):
        N = pick.size
        row, db, db16, fill = Buf((2 * N, C), BF16), Buf((2 * N, C), F32), Buf((2 * N, C), BF16), Buf((2 * N, C), BF16)
        for i in range(N):
            for j, (g, gb) in enumerate(((g32.t, 0), (g16.t, 1))):
                o = 2 * i + j
                assert L.ljs_bcast_scalar(_p(g[i:]), gb, C, Rf, _p(row.t[o]), _p(db.t[o]), _p(db16.t[o]), hip_stream(row.t)) == 0
                assert L.ljs_fill_row_bf16(_p(g[i:]), gb, _p(fill.t[o]), C, hip_stream(row.t)) == 0
        _rec(hip, "fill_row", (max(1, (C + 255) // 256),))
        assert L.ljs_bcast_scalar(_p(g32.t), 0, C, Rf, _p(row.t[0]), None, None, hip_stream(row.t)) == 0       # no db
        _rec(hip, "bcast_scalar", ((C + 255) // 256,))
        w = np.repeat(want[pick], 2)
        O.assert_bf16_bits(row.bits(), np.repeat(w[:, None], C, 1), ("row", C))
        O.assert_bf16_bits(fill.bits(), np.repeat(w[:, None], C, 1), ("fill", C))
        prod = ((w.astype(np.uint32) << 16).view(np.float32).astype(np.float64) * Rf)
        with np.errstate(over="ignore", invalid="ignore"):
            p32 = prod.astype(np.float32)                        # R * bf16(g): exact in f64, rounded once to f32
        nan = np.isnan(p32)
        got = db.bits()
        assert np.isnan(got.view(np.float32)[nan]).all()
        _same(got[~nan], np.repeat(p32.view(np.uint32)[:, None], C, 1)[~nan], ("db", C))
        O.assert_bf16_bits(db16.bits(), np.repeat(O.rne_bf16_bits(p32.view(np.uint32))[:, None], C, 1), ("db bf16", C))
        assert row.guards_ok() and db.guards_ok() and db16.guards_ok() and fill.guards_ok()


# ================================================================ random inputs, float64 oracle
WORST = {}


def _check(kernel, name, got, want64, ref32):
    """The rule of the module docstring; prints the figures first."""
    want64, ref32 = want64.double().cpu(), ref32.double().cpu()
    e_ref = (ref32 - want64).abs().max().item()
    slack = 4.0 * e_ref + 2.0 ** -23 * want64.abs().max().item()
    if got.dtype == BF16:
        want = want64.to(BF16).double()
        allowed = 2.0 ** -7 * want.abs() + slack
    else:
        want = want64
        allowed = torch.full_like(want, slack)
    err = (got.double().cpu().reshape(want.shape) - want).abs()
    frac = (err / allowed).max().item()
    WORST[kernel] = max(WORST.get(kernel, 0.0), frac)
    print(f"ew-figures {kernel} {name} dtype={_TAG[got.dtype]} max_err={err.max().item():.3e} E_ref={e_ref:.3e} "
          f"worst_fraction_of_bound={frac:.3f} (worst so far for {kernel}: {WORST[kernel]:.3f})")
    assert torch.isfinite(got).all(), name
    assert frac <= 1.0, (kernel, name, err.max().item(), e_ref, frac)


def _randn(shape, offset, seed, std=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return offset + std * torch.randn(*shape, generator=g)


@pytest.mark.parametrize("offset", [0.0, 100.0], ids=["centred", "offset100"])
def test_random_sums_against_float64(hip, offset):
    n = 300007
    for dtype in (F32, BF16):
        x = _randn((n,), offset, 1).to(dtype)
        xd = x.to(dev)
        for out_dtype in (F32, BF16):
            got = hip._sum_all_raw(xd, out_dtype)
            _check(f"sum_all<{_TAG[dtype]}>", f"n={n} offset={offset:g} out={_TAG[out_dtype]}", got, x.double().sum(), xd.float().sum())
    R, C = 3001, 192
    xb = _randn((R, C), offset, 2).to(BF16)
    _check("colsum<ticket>", f"{R}x{C} offset={offset:g}", hip.colsum(xb.to(dev)), xb.double().sum(0), xb.to(dev).float().sum(0))
    assert hip.last_launch()["name"] == "colsum<ticket>"
    xf = _randn((R, C), offset, 3)
    _check("colsum<f32>", f"{R}x{C} offset={offset:g}", hip.colsum(xf.to(dev)), xf.double().sum(0), xf.to(dev).sum(0))
    assert hip.last_launch()["name"] == "colsum<f32>"
    xr = _randn((61, 640), offset, 4)
    _check("rows_sum_f32", f"61x640 offset={offset:g}", hip.rows_sum(xr.to(dev)), xr.double().sum(0), xr.to(dev).sum(0))
    S, Rr, Cc = 9, 64, 640
    sl = _randn((S, Rr, Cc), offset, 5)
    out = torch.empty((Rr, Cc), device=dev)
    twin = torch.empty((Rr, Cc), dtype=BF16, device=dev)
    hip.slab_reduce(sl.to(dev), out, Cc, Rr * Cc, out_bf16=twin)
    _check("slab_reduce<f32>", f"S={S} offset={offset:g}", out, sl.double().sum(0), sl.to(dev).sum(0))
    _check("slab_reduce<f32>", f"S={S} offset={offset:g} twin", twin, sl.double().sum(0), sl.to(dev).sum(0))


@pytest.mark.parametrize("offset", [0.0, 100.0], ids=["centred", "offset100"])
def test_random_mse_against_float64(hip, offset):
    R, C = 1000, 640
    y, t = _randn((R, C), offset, 6).to(BF16), _randn((R, C), offset, 7)
    scale = 1.0 / (R * C)

    def formula(yy, tt):
        d = yy - tt
        return (d * d).sum() * scale, 2 * scale * d

    want = formula(y.double(), t.double())
    ref = formula(y.to(dev).float(), t.to(dev))
    yd, td = y.to(dev), t.to(dev)
    L = hip.lib()
    dy, out = torch.empty_like(yd), torch.empty((), device=dev)
    ws = hip._workspace(dev, "mse", (1024 + 33) * 4)
    assert L.ljs_mse_loss(_p(yd), _p(td), 0, R * C, scale, _p(dy), _p(out), _p(ws), hip_stream(yd)) == 0
    assert hip.last_launch()["name"] == "mse<tf32,dy>"
    _check("mse", f"{R}x{C} offset={offset:g} loss", out, want[0], ref[0])
    _check("mse", f"{R}x{C} offset={offset:g} dy", dy, want[1], ref[1])
    sums = torch.empty((C,), device=dev)
    ws2 = hip._workspace(dev, f"mse_colsum/{R}x{C}", L.ljs_mse_colsum_ws_bytes(R, C))
    assert L.ljs_mse_colsum(_p(yd), _p(td), 0, R, C, scale, _p(dy), _p(sums), _p(out), _p(ws2), hip_stream(yd)) == 0
    assert hip.last_launch()["name"] == "mse_colsum<tf32>"
    _check("mse_colsum", f"{R}x{C} offset={offset:g} loss", out, want[0], ref[0])
    _check("mse_colsum", f"{R}x{C} offset={offset:g} dy", dy, want[1], ref[1])
    stored = dy.double().cpu()                                   # the bias gradient sums the bf16 values that were stored
    _check("mse_colsum", f"{R}x{C} offset={offset:g} colsum", sums, stored.sum(0), dy.float().sum(0))


def _softmax(hip, x):
    rows, L = x.shape
    xin, out = Buf((rows, L), F32), Buf((rows, L), F32)
    xin.t.copy_(x)
    assert hip.lib().ljs_softmax_rows_f32(_p(xin.t), _p(out.t), rows, L, hip_stream(out.t)) == 0
    _rec(hip, "softmax_rows_f32", ((rows + 3) // 4,))
    assert out.guards_ok()
    return out.t.clone()


@pytest.mark.parametrize("dist", [(1.5, 0.0), (1.5, 100.0), (8.0, 0.0)], ids=["std1.5", "offset100", "std8"])
@pytest.mark.parametrize("L", [1, 63, 64, 65, 300, 4097])
def test_softmax_rows_against_float64(hip, L, dist):
    std, offset = dist
    for rows in (1, 4, 5):
        x = _randn((rows, L), offset, 10 * L + rows, std)
        if L > 2:
            x[rows - 1, 1::3] = float("-inf")                    # a row holding -inf entries
        if rows > 1:
            x[0, :] = offset + 0.5                               # a row of equal values
        got = _softmax(hip, x.to(dev))
        want, ref = torch.softmax(x.double(), -1), torch.softmax(x.to(dev), -1)
        tag = f"L={L} rows={rows} std={std:g} offset={offset:g}"
        _check("softmax_rows_f32", tag, got, want, ref)
        _check("softmax_rows_f32", tag + " rowsum", got.double().sum(-1), want.sum(-1), ref.double().sum(-1))
        if rows > 1:
            assert (got[0] == got[0, 0]).all()
        if L > 2:
            assert (got[rows - 1, 1::3] == 0).all()
