"""Exact oracles for the elementwise, reduction and MSE kernels (csrc/kernels/elementwise.hip, loss.hip): plain
numpy on int64 and on bit patterns, nothing of the package.

Exact inputs.  Every value is ``k * unit`` with a small integer ``k`` and ``unit`` a power of two, so it is
bf16-representable (``|k| < 256``) and sums of such values are integers times ``unit``.  ``exact_budget(x, unit)``
asserts, in int64, that ``sum(|x_i|) / unit < 2^24``.  Under that condition every partial sum of every subset, in
every order and grouping, is an integer multiple of ``unit`` below ``2^24 * unit`` and therefore exact in f32: a
kernel's result must equal the integer sum bit for bit, whatever its reduction tree, ticket order or atomics do.
It is a condition on the input, not a measurement of a kernel; every exact test calls it on its own input.

Planted values.  ``planted(R, C)`` gives ``k >= 0`` everywhere: an even background (0, 2, 4) and distinct odd
values (``odd(j)``, 64 of them, neighbours always different) at every chunk start (column ``c % 8 == 0``, which
includes every row start) and at every tail position (the columns past the last whole 8-element chunk of a row).
Since every value is non-negative and every chunk, row and block holds at least one odd (hence positive) value,
dropping any one 8-element chunk, row or block partial lowers the sum and counting one twice raises it; a chunk or
row that lands in the wrong place changes the positional outputs (column sums, transposes, gradients) because
neighbouring chunks and rows carry different odd values.  ``sparse(n, every)`` is the same idea for arrays too
long for the budget: zeros, with ``odd`` values at every ``every``-th chunk start and at each tail position.

MSE.  ``mse_inputs`` gives ``y`` and ``t`` as small integers times ``unit`` with ``d = y - t`` signed, odd at the
chunk starts and tail positions.  ``d``, ``d * d`` (an integer times ``unit^2``) and ``sum(d * d)`` are held to the
same budget, so the kernels' ``fmaf`` accumulation is exact; with ``scale`` a power of two ``loss = scale * sum`` and
``dy = bf16(2 * scale * d)`` are exact too.

Rounding sweep.  ``sweep_bits()`` is every 16-bit upper half of an f32 combined with the lower halves 0x0000,
0x0001, 0x7fff, 0x8000, 0x8001 and 0xffff (393 216 patterns: ties, both neighbours of a tie, NaNs, infinities,
denormals and the f32 maximum are there by construction); ``rne_bf16_bits`` is round-to-nearest-even on the bit
pattern, in integers.

ReLU mask rule.  ``relu_keep(mask_bits)``: sign bit clear and magnitude bits non-zero.  It agrees with
``float(mask) > 0`` on every non-NaN bf16 pattern (-0.0 and denormals included) and differs on the 127 positive-sign
NaN patterns 0x7f81 .. 0x7fff, which the kernels keep and a float comparison drops.

Launch geometry.  ``colsum_plan``, ``relu_bwd_colsum_grid``, ``mse_colsum_plan``, ``sum_all_grid`` and ``mse_grid``
re-state the launchers' arithmetic; they choose shapes and predict the recorded grid, and the GPU tests assert them
against the launch record, so a drift is caught.
"""
import os
import re

import numpy as np

_KERNELS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "learning_jax_sharding_amd", "csrc",
                        "kernels")


def ticket_group() -> int:
    """``kTicketGroup`` as csrc/kernels/rowwise.h states it."""
    with open(os.path.join(_KERNELS, "rowwise.h")) as f:
        return int(re.search(r"constexpr unsigned kTicketGroup = (\d+);", f.read()).group(1))


# ============================================================================ exact inputs
LIMIT = 1 << 24


def exact_budget(x, unit: float) -> int:
    """Assert ``sum(|x_i|) / unit < 2^24`` in int64 (every x_i an integer multiple of ``unit``); returns the sum."""
    q = np.asarray(x, dtype=np.float64).ravel() / unit
    k = np.rint(q).astype(np.int64)
    assert np.array_equal(k.astype(np.float64), q), "values are not integer multiples of the unit"
    total = int(np.abs(k).sum(dtype=np.int64))
    assert total < LIMIT, (total, LIMIT)
    return total


def odd(j):
    """64 distinct odd values 1 .. 127; odd(j) != odd(j + 1)."""
    return 2 * ((np.asarray(j, dtype=np.int64) * 29 + 7) % 64) + 1


def planted(R: int, C: int, chunk: int = 8) -> np.ndarray:
    """int64 k[R][C] >= 0 (see the module docstring)."""
    r = np.arange(R, dtype=np.int64)[:, None]
    c = np.arange(C, dtype=np.int64)[None, :]
    nch = (C + chunk - 1) // chunk
    k = 2 * ((r * 5 + c * 3 + (c >> 3)) % 3)
    k = np.where(c % chunk == 0, odd(r * nch + c // chunk), k)
    k = np.where(c >= C - C % chunk, odd(r * 31 + c + 11), k)
    return np.ascontiguousarray(np.broadcast_to(k, (R, C)))


def sparse(n: int, every: int, chunk: int = 8):
    """(indices, k) of the non-zero entries of a length-n array: ``odd`` values at every ``every``-th chunk start and at
    each tail position."""
    idx = np.arange(0, n - n % chunk, chunk * every, dtype=np.int64)
    tail = np.arange(n - n % chunk, n, dtype=np.int64)
    idx = np.concatenate([idx, tail])
    return idx, odd(idx // chunk + idx % chunk)


def mse_inputs(R: int, C: int, kmax: int = 7):
    """(ky, kt) int64 [R][C]: d = ky - kt is odd with |d| <= kmax (kmax + 1 a power of two) at chunk starts and tail
    positions, alternating in sign from chunk to chunk, and |d| <= 2 elsewhere."""
    assert kmax & (kmax + 1) == 0
    r = np.arange(R, dtype=np.int64)[:, None]
    c = np.arange(C, dtype=np.int64)[None, :]
    nch = (C + 7) // 8
    mark = (c % 8 == 0) | (c >= C - C % 8)
    mag = odd(r * nch + c // 8 + c % 8) % (kmax + 1)
    kd = np.where(mark, np.where((r + c // 8 + c % 8) % 2 == 0, mag, -mag), (r * 7 + c * 5) % 5 - 2)
    ky = np.broadcast_to((r + c) % 4, (R, C))
    return np.ascontiguousarray(ky), np.ascontiguousarray(ky - kd)


def f32_bits(x) -> np.ndarray:
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def bf16_bits_exact(x) -> np.ndarray:
    """uint16 bf16 patterns of values that are bf16-representable (asserted)."""
    b = f32_bits(x)
    assert not (b & 0xFFFF).any(), "value is not bf16-representable"
    return (b >> 16).astype(np.uint16)


# ============================================================================ rounding
SWEEP_LOW = (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF)
F32_MAX, BF16_INF = 0x7F7FFFFF, 0x7F80


def sweep_bits() -> np.ndarray:
    hi = np.arange(1 << 16, dtype=np.uint32) << 16
    return (hi[:, None] | np.array(SWEEP_LOW, dtype=np.uint32)[None, :]).ravel()


def is_nan_f32(bits) -> np.ndarray:
    return (np.asarray(bits, dtype=np.uint32) & 0x7FFFFFFF) > 0x7F800000


def is_nan_bf16(bits) -> np.ndarray:
    return (np.asarray(bits).astype(np.uint32) & 0x7FFF) > 0x7F80


def rne_bf16_bits(bits) -> np.ndarray:
    """uint16 bf16 pattern of each f32 pattern, round to nearest, ties to even, on integers.  A NaN gives a NaN
    (0x7fc0 with the sign kept: only NaN-ness is part of the contract)."""
    b = np.asarray(bits, dtype=np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF
    nan = ((b >> 16) & 0x8000) | 0x7FC0
    return np.where(is_nan_f32(bits), nan, r).astype(np.uint16)


def round_bf16(x) -> np.ndarray:
    """f32 values rounded to bf16 and widened back to f32."""
    return (rne_bf16_bits(f32_bits(x)).astype(np.uint32) << 16).view(np.float32)


def assert_bf16_bits(got, want, what=""):
    """Equal bit for bit where ``want`` is not a NaN, NaN where it is."""
    got, want = np.asarray(got).astype(np.uint16).ravel(), np.asarray(want).astype(np.uint16).ravel()
    nan = is_nan_bf16(want)
    bad = np.flatnonzero(np.where(nan, ~is_nan_bf16(got), got != want))
    assert bad.size == 0, (what, bad.size, [(int(i), hex(int(want[i])), hex(int(got[i]))) for i in bad[:4]])


# ============================================================================ ReLU mask
def relu_keep(mask_bits) -> np.ndarray:
    m = np.asarray(mask_bits).astype(np.uint32)
    return ((m & 0x8000) == 0) & ((m & 0x7FFF) != 0)


RELU_NAN_DIFFERENCES = 127   # 0x7f81 .. 0x7fff


# ============================================================================ launch geometry
MAX_GRID = 2048
SUM_MAX_BLOCKS = 1024
MSE_MAX_BLOCKS = 1024
COLSUM_WS_FLOATS = 1 << 20


def _grid_for(n, per):
    return int(min(MAX_GRID, max(1, -(-n // per))))


def sum_all_v(is_bf16):
    return 8 if is_bf16 else 4


def sum_all_per(is_bf16):
    """Elements one block of the ticket kernel covers in one batch of 16 loads per thread."""
    return 256 * sum_all_v(is_bf16) * 16


def sum_all_grid(n, is_bf16, aligned=True):
    """(instance suffix, blocks) of ljs_sum_all."""
    if aligned:
        return "ticket", min(SUM_MAX_BLOCKS, _grid_for(n, sum_all_per(is_bf16)))
    return "atomic", _grid_for(n, 256 * 16)


def _ticket_rows(R, C):
    cb = (C + 63) // 64
    gy = max(1, 512 // cb)
    rpb = max(32, -(-R // gy))
    return cb, -(-R // rpb), rpb


def colsum_plan(is_bf16, R, C, ld, aligned=True, ws=True):
    """(recorded name, grid (x, y)) of ljs_colsum."""
    if ld == 0:
        return "colsum<bcast>", ((C + 255) // 256, 1)
    if is_bf16 and C % 8 == 0 and ld % 8 == 0 and aligned:
        cb, gy, _ = _ticket_rows(R, C)
        ok = ws and cb <= 4096 and gy * C + 4096 <= COLSUM_WS_FLOATS
        return ("colsum<ticket>" if ok else "colsum<vec>"), (cb, gy)
    return ("colsum<bf16>" if is_bf16 else "colsum<f32>"), ((C + 255) // 256, min(64, max(1, R // 256)))


def ticket_unrolled_rounds(rpb, rl):
    """Iterations of colsum_ticket_kernel's 4-rows-in-flight loop (``r + 96 < r1``, ``r += 128``) for row lane
    ``rl`` of a full block of ``rpb`` rows."""
    return len(range(rl, max(rl, rpb - 96), 128))


def relu_bwd_colsum_grid(R, C):
    cb, gy, _ = _ticket_rows(R, C)
    return cb, gy


def relu_bwd_grid(R, C):
    return int(min(8192, max(1, -(-(R * (C // 8)) // 256))))


def mse_grid(n):
    return int(min(MSE_MAX_BLOCKS, max(1, -(-(n // 8) // 1024))))


def mse_colsum_plan(R, C):
    """cb, gy, rpb and the workspace offsets (4-byte words) of ljs_mse_colsum."""
    cb = C // 64
    want = max(1, 1024 // max(1, cb))
    rpb = max(96, -(-(-(-R // want)) // 96) * 96)
    gy = -(-R // rpb)
    nblk = cb * gy
    col_part = cb + 1 + (nblk + 31) // 32 + 64
    loss_part = col_part + gy * C
    return dict(cb=cb, gy=gy, rpb=rpb, col_part=col_part, loss_part=loss_part, words=loss_part + nblk + 64)


def slab_reduce_grid(R, C):
    return int(min(2048, max(1, -(-(R * C // 4) // 256))))


# ============================================================================ the shapes the GPU tests run
# (tests/test_elementwise_oracle_gpu.py takes them from here; tests/test_elementwise_oracle.py holds every exact
# input built from them to exact_budget on the CPU)
UNIT = 2.0 ** -3
MSE_SCALE = 2.0 ** -4


def sum_all_dense_ns(is_bf16):
    """Lengths of the dense sum_all inputs: every n % V tail at one block, one chunk short of / over one full batch
    of 16 loads per thread, and the first n of 2, kTicketGroup and kTicketGroup + 1 blocks."""
    V, per, tg = sum_all_v(is_bf16), sum_all_per(is_bf16), ticket_group()
    ns = [40 * V + t for t in range(V)] + [4095 * V, 4097 * V]
    return ns + [(g - 1) * per + 1 for g in (2, tg, tg + 1)]


def sum_all_sparse_ns(is_bf16):
    """1024 blocks, and 32 grid strides of chunks and a bit: the unrolled loop runs twice for every thread."""
    V, per = sum_all_v(is_bf16), sum_all_per(is_bf16)
    return [(SUM_MAX_BLOCKS - 1) * per + V + 1, 2 * SUM_MAX_BLOCKS * per + 3 * V + 3]


def sum_all_rearm_ns():
    """bf16 lengths of the re-arm sequence: kTicketGroup + 1, 1, 2, kTicketGroup and 3 kTicketGroup + 5 blocks."""
    tg, per = ticket_group(), sum_all_per(True)
    return [(g - 1) * per + 9 for g in (tg + 1, 1, 2, tg, 3 * tg + 5)]


SUM_ALL_UNALIGNED = ((1, 5000), (3, 70001))              # (elements the base is off the 16-byte grid, n)
SUM_PARTIALS_N = (1, 63, 64, 255, 256, 257, 1000)
COLSUM_TICKET = [(R, 64) for R in (1, 33, 129, 1024, 1056, 2100)] + [(129, 72), (2100, 8)]
# rows per block above 96: the 4-rows-in-flight loops run (one round for lane 0 only, one round for every lane, two
# rounds for lane 0); sparse inputs, an ``odd`` value at every COLSUM_DEEP_EVERY-th chunk
COLSUM_TICKET_DEEP = [(4900, 640), (6500, 640), (11500, 640)]
COLSUM_DEEP_EVERY = 7
COLSUM_BCAST = ((37, 1), (37, 255), (1000, 257))
COLSUM_VEC = (129, 72, 80)                               # R, C, ld
COLSUM_GENERIC = [("f32", R, 5, 5) for R in (1, 255, 256, 300, 16385)] + [("f32", 300, 300, 304), ("bf16", 300, 13, 13),
                                                                            ("bf16", 16385, 16, 17)]
ROWS_SUM_R, ROWS_SUM_C = (1, 4, 5, 28, 29, 32, 33, 61), (1, 63, 64, 65)
SUM_N_N = (1, 2, 3, 128)
SLAB_S = (1, 2, 4, 5, 8, 9)
SLAB_BIG = (1032, 2048)                                  # R x C with R * C / 4 above 2048 blocks of 256
MSE_SPARSE_N = (8 * ((MSE_MAX_BLOCKS - 1) * 1024 + 1), MSE_MAX_BLOCKS * 256 * 4 * 8 + 8 * 2048 + 3)
MSE_DENSE_N = (320, 321, 327, 8 * 1025 + 1, 8 * (32 * 1024 + 1) + 7)      # 1, 1, 1, 2 and 33 blocks
MSE_COLSUM_R, MSE_COLSUM_C = (1, 31, 95, 96, 97, 160, 161, 193, 900), (64, 128, 640)
MSE_COLSUM_BIG = (5000, 640)                             # 10 x 53 = 530 blocks


def sum_n_counts(is_bf16):
    V = sum_all_v(is_bf16)
    return (1, V - 1, V, V + 1, 256 * V + 3)


def budget_cases():
    """(label, values, unit) of every exact input of the GPU tests."""
    for bf in (True, False):
        V, tag = sum_all_v(bf), "bf16" if bf else "f32"
        for n in sum_all_dense_ns(bf) + [n for _, n in SUM_ALL_UNALIGNED]:
            yield f"sum_all {tag} n={n}", planted(1, n, V) * UNIT, UNIT
        for n in sum_all_sparse_ns(bf):
            yield f"sum_all {tag} sparse n={n}", sparse(n, 64, V)[1] * UNIT, UNIT
        for n in SUM_N_N:
            for count in sum_n_counts(bf):
                yield f"sum_n {tag} {n}x{count}", planted(n, count, V) * UNIT, UNIT
        for S in SLAB_S:
            yield f"slab_reduce {tag} S={S}", planted(S * 3, 8, 4) * UNIT, UNIT
        yield f"slab_reduce {tag} big", sparse(2 * SLAB_BIG[0] * SLAB_BIG[1], 64, 4)[1] * UNIT, UNIT
    for n in SUM_PARTIALS_N:
        yield f"sum_partials n={n}", planted(1, n, 4) * UNIT, UNIT
    for R, C in COLSUM_TICKET:                           # (relu_bwd_colsum and relu_bwd take the same inputs)
        yield f"colsum ticket {R}x{C}", planted(R, C) * UNIT, UNIT
    for R, C in COLSUM_TICKET_DEEP:
        yield f"colsum ticket deep {R}x{C}", sparse(R * C, COLSUM_DEEP_EVERY)[1] * UNIT, UNIT
    for R, C in COLSUM_BCAST:
        yield f"colsum bcast {R}x{C}", planted(1, C) * R * UNIT, UNIT
    yield "colsum vec", 2 * planted(*COLSUM_VEC[:2]) * UNIT, UNIT        # (summed twice: the accumulate pass)
    for n in sum_all_rearm_ns():
        yield f"sum_all rearm n={n}", sparse(n, 16)[1] * UNIT, UNIT
    for tag, R, C, _ in COLSUM_GENERIC:
        yield f"colsum {tag} {R}x{C}", planted(R, C) * UNIT, UNIT
    for R in ROWS_SUM_R:
        for C in ROWS_SUM_C:
            yield f"rows_sum {R}x{C}", planted(R, C) * UNIT, UNIT
    shapes = [(1, n, 7) for n in MSE_DENSE_N] + [(R, C, 7) for C in MSE_COLSUM_C for R in MSE_COLSUM_R]
    for R, C, kmax in shapes + [MSE_COLSUM_BIG + (1,)]:
        ky, kt = mse_inputs(R, C, kmax)
        d = (ky - kt) * UNIT
        yield f"mse {R}x{C} d*d", d * d, UNIT * UNIT
        yield f"mse {R}x{C} dy", 2 * MSE_SCALE * d, 2 * MSE_SCALE * UNIT
    for n in MSE_SPARSE_N:
        d = sparse(n, 64)[1] % 8 * UNIT
        yield f"mse sparse n={n}", d * d, UNIT * UNIT
