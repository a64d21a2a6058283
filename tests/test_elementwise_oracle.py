"""The oracle of tests/elementwise_oracle.py held to independent statements of the same rules, on the CPU: the
integer rounding against torch's own f32 -> bf16 conversion, the ReLU mask rule against a float comparison, the
exact-input generators against the budget at every shape the GPU tests use, and the launch-geometry re-statements
against the loop edges the GPU shapes were chosen for."""
import numpy as np
import pytest
import torch

import elementwise_oracle as O


# ---------------------------------------------------------------- rounding
@pytest.fixture(scope="module")
def sweep():
    bits = O.sweep_bits()
    return bits, O.rne_bf16_bits(bits)


def _torch_bf16_bits(bits):
    t = torch.from_numpy(bits.view(np.int32).copy()).view(torch.float32)
    return t.bfloat16().view(torch.int16).numpy().view(np.uint16)


def test_sweep_holds_every_upper_half_with_six_lower_halves(sweep):
    bits, _ = sweep
    assert bits.size == 393216 == np.unique(bits).size
    assert set((bits & 0xFFFF).tolist()) == set(O.SWEEP_LOW) and np.unique(bits >> 16).size == 65536


def test_integer_rounding_equals_torch_on_every_non_nan_pattern(sweep):
    bits, want = sweep
    got, nan = _torch_bf16_bits(bits), O.is_nan_f32(bits)
    assert nan.sum() == 2 * (127 * 6 + 5)           # exponent 0xff, mantissa != 0, both signs
    assert np.array_equal(got[~nan], want[~nan])
    assert O.is_nan_bf16(got[nan]).all() and O.is_nan_bf16(want[nan]).all()


def test_f32_max_rounds_to_infinity(sweep):
    bits, want = sweep
    for sign in (0, 0x80000000):
        (i,) = np.flatnonzero(bits == (O.F32_MAX | sign))
        assert want[i] == (O.BF16_INF | (sign >> 16))
        assert want[np.flatnonzero(bits == (0x7F7F7FFF | sign))[0]] == (0x7F7F | (sign >> 16))   # below the tie: finite


def test_ties_round_to_even(sweep):
    bits, want = sweep
    tie = (bits & 0xFFFF) == 0x8000
    fin = tie & ~O.is_nan_f32(bits) & ((bits & 0x7F800000) != 0x7F800000)
    up = bits[fin] >> 16
    assert np.array_equal(want[fin], (up + (up & 1)).astype(np.uint16))
    below, above = (bits & 0xFFFF) == 0x7FFF, (bits & 0xFFFF) == 0x8001
    ok = ~O.is_nan_f32(bits) & ((bits & 0x7F800000) != 0x7F800000)
    assert np.array_equal(want[below & ok], (bits[below & ok] >> 16).astype(np.uint16))
    assert np.array_equal(want[above & ok], ((bits[above & ok] >> 16) + 1).astype(np.uint16))


def test_denormal_inputs_round_like_any_other(sweep):
    bits, want = sweep
    den = ((bits & 0x7F800000) == 0) & ((bits & 0x7FFFFF) != 0)
    assert den.sum() == 2 * (127 * 6 + 5)
    assert np.array_equal(want[den], _torch_bf16_bits(bits[den]))
    assert want[np.flatnonzero(bits == 0x00008000)[0]] == 0 and want[np.flatnonzero(bits == 0x00008001)[0]] == 1
    assert want[np.flatnonzero(bits == 0x007FFFFF)[0]] == 0x0080        # the largest denormal rounds to the least normal


def test_round_bf16_and_exact_bits():
    x = np.array([1.0, 1.00390625, 1.01171875, -3.0e38, 255.0, 257.0], dtype=np.float32)
    want = torch.from_numpy(x).bfloat16().float().numpy()
    assert np.array_equal(O.round_bf16(x), want)
    assert O.bf16_bits_exact(np.array([255.0 * O.UNIT]))[0] == _torch_bf16_bits(O.f32_bits([255.0 * O.UNIT]))[0]
    with pytest.raises(AssertionError):
        O.bf16_bits_exact(np.array([257.0]))


# ---------------------------------------------------------------- ReLU mask
def test_relu_mask_rule_against_float_comparison():
    m = np.arange(1 << 16, dtype=np.uint32)
    keep = O.relu_keep(m)
    f = (m << 16).view(np.float32)
    with np.errstate(invalid="ignore"):
        cmp = f > 0
    nan = O.is_nan_bf16(m)
    assert np.array_equal(keep[~nan], cmp[~nan])
    assert not keep[0x8000] and not keep[0x0000] and keep[0x0001] and not keep[0x8001] and keep[0x7F80] and not keep[0xFF80]
    differ = np.flatnonzero(keep != cmp)
    assert differ.size == O.RELU_NAN_DIFFERENCES == 127
    assert differ[0] == 0x7F81 and differ[-1] == 0x7FFF and keep[differ].all()      # positive-sign NaNs are kept


# ---------------------------------------------------------------- exact inputs
def test_every_gpu_input_satisfies_the_budget():
    n = 0
    for label, values, unit in O.budget_cases():
        try:
            O.exact_budget(values, unit)
        except AssertionError as e:
            raise AssertionError(label) from e
        n += 1
    assert n > 150


def test_exact_budget_refuses():
    with pytest.raises(AssertionError):
        O.exact_budget(np.full(1 << 17, 128 * O.UNIT), O.UNIT)          # 2^24 exactly
    O.exact_budget(np.full((1 << 17) - 1, 128 * O.UNIT), O.UNIT)
    with pytest.raises(AssertionError):
        O.exact_budget(np.array([1.5 * O.UNIT]), O.UNIT)                # not a multiple of the unit


def test_budget_makes_every_order_exact():
    """What the condition is for: f32 sums of a budgeted input in several orders and groupings equal the integer sum."""
    k = O.planted(33, 72)
    x = (k * O.UNIT).astype(np.float32)
    O.exact_budget(x, O.UNIT)
    want = np.float32(int(k.sum()) * O.UNIT)
    rng = np.random.default_rng(0)
    for _ in range(4):
        p = rng.permutation(x.ravel())
        seq = np.float32(0)
        for v in p[:500]:
            seq = np.float32(seq + v)
        rest = np.add.reduce(p[500:].reshape(-1, 4).astype(np.float32), axis=1, dtype=np.float32)
        assert np.float32(seq + np.add.reduce(rest, dtype=np.float32)) == want


@pytest.mark.parametrize("R,C,chunk", [(1, 327, 8), (5, 72, 8), (33, 13, 8), (1, 4099, 4), (3, 64, 8)])
def test_planted_values(R, C, chunk):
    k = O.planted(R, C, chunk)
    assert k.shape == (R, C) and k.min() >= 0 and k.max() <= 127
    c = np.arange(C)
    marks = (c % chunk == 0) | (c >= C - C % chunk)
    assert (k[:, marks] % 2 == 1).all() and (k[:, ~marks] % 2 == 0).all()
    starts = k[:, (c % chunk == 0) & (c < C - C % chunk)].ravel()
    assert (starts[1:] != starts[:-1]).all()                 # neighbouring chunks (and rows) differ
    tail = k[:, C - C % chunk:]
    assert tail.shape[1] < 2 or (tail[:, 1:] != tail[:, :-1]).all()
    # one chunk, one row or any run of chunks dropped or counted twice changes the sum: all of them are positive
    assert (k.reshape(-1)[: (R * C) // chunk * chunk].reshape(-1, chunk).sum(1) > 0).all() and (k.sum(1) > 0).all()


def test_sparse_and_mse_inputs():
    idx, k = O.sparse(8 * 64 * 5 + 3, 64)
    assert idx.tolist() == [0, 512, 1024, 1536, 2048, 2560, 2561, 2562] and (k % 2 == 1).all()
    ky, kt = O.mse_inputs(97, 72)
    d = ky - kt
    c = np.arange(72)
    assert (d[:, c % 8 == 0] % 2 != 0).all() and np.abs(d).max() == 7 and (d > 0).any() and (d < 0).any()
    assert np.abs(ky).max() < 256 and np.abs(kt).max() < 256
    assert np.abs(O.mse_inputs(5, 64, 1)[0] - O.mse_inputs(5, 64, 1)[1]).max() <= 2


# ---------------------------------------------------------------- launch geometry
def test_sum_all_grids_reach_the_ticket_edges():
    tg = O.ticket_group()
    assert tg == 32
    for bf in (True, False):
        grids = [O.sum_all_grid(n, bf)[1] for n in O.sum_all_dense_ns(bf)]
        assert grids == [1] * O.sum_all_v(bf) + [1, 2, 2, tg, tg + 1], grids
        V, (n1, n2) = O.sum_all_v(bf), O.sum_all_sparse_ns(bf)
        assert O.sum_all_grid(n1, bf) == ("ticket", 1024) == O.sum_all_grid(n2, bf)
        assert O.sum_all_grid(n1 - V - 1, bf)[1] == 1023
        assert n2 // V >= 32 * 1024 * 256                      # every thread's unrolled loop runs twice
    assert [O.sum_all_grid(n, True, aligned=False) for _, n in O.SUM_ALL_UNALIGNED] == [("atomic", 2), ("atomic", 18)]


def test_colsum_plans_reach_the_loop_edges():
    ticket = [O.colsum_plan(True, R, C, C) for R, C in O.COLSUM_TICKET]
    assert [g for _, g in ticket] == [(1, 1), (1, 2), (1, 5), (1, 32), (1, 33), (1, 66), (2, 5), (1, 66)]
    assert all(n == "colsum<ticket>" for n, _ in ticket)
    # every shape above has 32 rows per block: the 4-rows-in-flight loops (r + 96 < r1) never run there ..
    assert all(O._ticket_rows(R, C)[2] == 32 for R, C in O.COLSUM_TICKET)
    assert all(O.ticket_unrolled_rounds(32, rl) == 0 for rl in range(32))
    # .. the deep shapes reach them: one round for row lane 0 alone, one for every lane, two for lane 0
    deep = [O._ticket_rows(R, C) for R, C in O.COLSUM_TICKET_DEEP]
    assert deep == [(10, 51, 97), (10, 51, 128), (10, 51, 226)], deep
    rounds = [[O.ticket_unrolled_rounds(rpb, rl) for rl in (0, 1, 31)] for _, _, rpb in deep]
    assert rounds == [[1, 0, 0], [1, 1, 1], [2, 2, 1]], rounds
    assert all(O.colsum_plan(True, R, C, C + 8) == ("colsum<ticket>", (10, 51)) for R, C in O.COLSUM_TICKET_DEEP)
    generic = [O.colsum_plan(t == "bf16", R, C, ld) for t, R, C, ld in O.COLSUM_GENERIC]
    assert [g[1] for _, g in generic] == [1, 1, 1, 1, 64, 1, 1, 64]
    assert [n for n, _ in generic] == ["colsum<f32>"] * 6 + ["colsum<bf16>"] * 2
    assert O.colsum_plan(True, 129, 64, 64, ws=False) == ("colsum<vec>", (1, 5))
    assert O.colsum_plan(True, 129, 64, 64, aligned=False)[0] == "colsum<bf16>"
    assert O.colsum_plan(False, 37, 257, 0) == ("colsum<bcast>", (2, 1))
    assert O.relu_bwd_colsum_grid(2100, 64) == (1, 66) and O.relu_bwd_grid(2100, 64) == 66


def test_mse_plans_reach_the_loop_edges():
    assert [O.mse_grid(n) for n in O.MSE_DENSE_N] == [1, 1, 1, 2, 33]
    assert [O.mse_grid(n) for n in O.MSE_SPARSE_N] == [1024, 1024]
    assert O.MSE_SPARSE_N[1] > 1024 * 256 * 4 * 8
    gys = [O.mse_colsum_plan(R, 64)["gy"] for R in O.MSE_COLSUM_R]
    assert gys == [1, 1, 1, 1, 2, 2, 2, 3, 10], gys
    p = O.mse_colsum_plan(*O.MSE_COLSUM_BIG)
    assert p["cb"] * p["gy"] == 530 > 512 and p["rpb"] == 96
    p = O.mse_colsum_plan(1024, 640)
    assert (p["cb"], p["gy"], p["rpb"]) == (10, 11, 96)
    assert p["col_part"] == 10 + 1 + 4 + 64 and p["loss_part"] == p["col_part"] + 11 * 640 and p["words"] == p["loss_part"] + 110 + 64
    assert O.slab_reduce_grid(*O.SLAB_BIG) == 2048 and O.SLAB_BIG[0] * O.SLAB_BIG[1] // 4 > 2048 * 256
