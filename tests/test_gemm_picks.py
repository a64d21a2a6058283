"""Host-side GEMM dispatch decisions (ops/hip.py cost models), pinned on the CPU."""
import pytest

from learning_jax_sharding_amd.ops import hip


@pytest.fixture
def chip(monkeypatch):
    monkeypatch.setattr(hip, "_cus", lambda: 256)
    monkeypatch.setattr(hip, "_PAIR_PICKS", {})
    monkeypatch.setattr(hip, "_DW_PAIR", "")


def test_dw_pair_one_round_equal_splits(chip):
    # the step's dW_o (20 tiles of [512 x 640]) and dW_qkv (60 tiles of [640 x 1536])
    for T, want_tile, slots in ((2048, 12884, 256), (16384, 1282, 512)):
        tile, s0, s1 = hip.pick_dw_pair(512, 640, 640, 1536, T)
        assert tile == want_tile
        assert 20 * s0 + 60 * s1 <= slots           # one round of resident blocks
        assert hip.slab_count(T // 64, s0) == s0 and hip.slab_count(T // 64, s1) == s1
    assert hip.pick_dw_pair(512, 640, 640, 1536, 16384)[1:] == (6, 6)
    assert hip.pick_dw_pair(512, 640, 640, 1536, 2048)[1:] == (3, 3)


def test_dw_pair_none_when_no_round_fits(chip):
    assert hip.pick_dw_pair(2560, 2560, 2560, 1280, 16384) is None


def test_dw_pair_forced(chip, monkeypatch):
    monkeypatch.setattr(hip, "_DW_PAIR", "11,4")
    assert hip.pick_dw_pair(512, 640, 640, 1536, 2048) == (12884, 11, 4)
    monkeypatch.setattr(hip, "_DW_PAIR", "6,6,1282")
    monkeypatch.setattr(hip, "_PAIR_PICKS", {})
    assert hip.pick_dw_pair(512, 640, 640, 1536, 2048) == (1282, 6, 6)


def test_dw_pair_ff_block_stays_separate(chip):
    # two 100-tile GEMMs (the FF block's [2560 x 640] / [640 x 2560]) would need 2-3 splits for one
    # round: the separate launches' estimate is lower
    assert hip.pick_dw_pair(2560, 640, 640, 2560, 16384) is None


def test_dw_single_picks_unchanged(chip):
    # the separate launches (a lone held GEMM, or grouping off)
    assert hip.pick_dw_slabs(640, 1536, 16384) == (1282, 8, True)
    assert hip.pick_dw_slabs(512, 640, 16384) == (1282, 16, True)   # (single-launch slab weight)
    assert hip.pick_dw_slabs(640, 1536, 2048) == (12884, 4, True)


class _FakeHip:
    """Records the grouped-launch calls of ops/linear._hold_dw (no kernels)."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        return getattr(self.real, name)

    def gemm_group_begin(self):
        self.calls.append("begin")

    def gemm_group_end(self, ref):
        self.calls.append("end")


def test_held_weight_gradient_jobs_pair_and_flush(chip, monkeypatch):
    """ops/linear._hold_dw: the first slab GEMM is held, the next one launches both as a pair with
    the jointly picked split counts (inside one group), a lone held job launches alone at flush."""
    import torch
    from learning_jax_sharding_amd.ops import linear
    fake = _FakeHip(hip)
    monkeypatch.setattr(linear, "hip", fake)
    monkeypatch.setattr(linear, "_HELD", {})
    ran = []

    def job(name, K, N, T=16384):
        return linear._DwJob(K, N, T, -(-K // 128) * -(-N // 128),
                             lambda tile, S, n=name: ran.append((n, tile, S)))
    ref = torch.empty(1)
    linear._hold_dw(job("o", 512, 640), ref)
    assert ran == [] and fake.calls == []
    linear._hold_dw(job("qkv", 640, 1536), ref)
    assert fake.calls == ["begin", "end"]
    assert ran == [("o", 1282, 6), ("qkv", 1282, 6)]
    # a pair the pick declines (the FF block's): both alone with their single picks
    ran.clear()
    linear._hold_dw(job("ff_out", 2560, 640), ref)
    linear._hold_dw(job("ff_in", 640, 2560), ref)
    assert [r[0] for r in ran] == ["ff_out", "ff_in"] and fake.calls == ["begin", "end"]
    # a lone held job: launched alone when flushed
    ran.clear()
    linear._hold_dw(job("o2", 512, 640), ref)
    assert ran == []
    linear.flush_held_dw()
    assert ran == [("o2",) + tuple(hip.pick_dw_slabs(512, 640, 16384)[:2])]
    assert linear._HELD == {}


# ============================================================================ the launcher's plan step
# ljs_gemm_plan (hip.gemm_plan) is the launcher's own resolution of a call -- tile, kernel instance,
# grid, split, psum count -- as a pure function: the built library answers it without a GPU.
@pytest.fixture(scope="module")
def planned():
    import os
    if not os.path.exists(hip._LIBPATH):
        from learning_jax_sharding_amd.csrc import build
        build.build_all()
    hip.lib()


def _layouts_matrix():
    """test_gemm_layouts' parametrize marks: (tiles, layouts, outputs, shapes)."""
    import test_kernels_gpu as tk
    params = {m.args[0]: m.args[1] for m in tk.test_gemm_layouts.pytestmark if m.name == "parametrize"}
    return params["tile"], params["a_kc,b_kc"], params["out_f32"], params["M,N,K"]


def _marks(fn):
    return {m.args[0]: m.args[1] for m in fn.pytestmark if m.name == "parametrize"}


def _plan(tile, a_kc, b_kc, out_f32, M, N, K, **kw):
    """The plan of a test_gemm_layouts-style call (dense operands unless ``kw`` says otherwise)."""
    lda, ldb, ldc = kw.pop("lda", K if a_kc else M), kw.pop("ldb", K if b_kc else N), kw.pop("ldc", N)
    return hip.gemm_plan(M, N, K, lda, ldb, ldc, bool(a_kc), bool(b_kc), bool(out_f32), tile=tile, **kw)


def _agrees(tile, a_kc, b_kc, out_f32, M, N, K, plan_kw=None, mirror_kw=None):
    """The plan's resolved tile against the Python statement of the rules; returns the plan."""
    from test_kernel_variants_gpu import resolved_tile
    plan = _plan(tile, a_kc, b_kc, out_f32, M, N, K, **(plan_kw or {}))
    want = resolved_tile(tile, a_kc, b_kc, out_f32, M, N, K, **(mirror_kw or {}))
    assert plan["err"] == 0 and plan["resolved_tile"] == want, (tile, a_kc, b_kc, out_f32, M, N, K, plan_kw, plan, want)
    return plan


_FORCED = (0, 100000, 200000)


def test_plan_resolves_the_layouts_matrix_as_the_mirror(planned):
    import itertools
    tiles, layouts, outs, shapes = _layouts_matrix()
    assert (len(tiles), len(layouts), len(outs), len(shapes)) == (13, 4, 2, 5)
    for t, f, (a_kc, b_kc), of, (M, N, K) in itertools.product(tiles, _FORCED, layouts, outs, shapes):
        plan = _agrees(t + f, a_kc, b_kc, of, M, N, K)
        # forcing picks between a tile's two kernels, never the tile; the general one when asked for
        assert plan["resolved_tile"] == _plan(t, a_kc, b_kc, of, M, N, K)["resolved_tile"]
        assert f != 200000 or plan["family"] != "lean"
        assert plan["family"] != "lean" or (a_kc and b_kc and not of)


def test_plan_resolves_further_calls_as_the_mirror(planned):
    import itertools
    import torch
    tiles, layouts, _, shapes = _layouts_matrix()
    for t, f, (a_kc, b_kc) in itertools.product(tiles, _FORCED, layouts):
        t += f
        for M, N, K in shapes:
            for rd in (torch.bfloat16, torch.float32):     # an epilogue operand (bf16 outputs only)
                plan = _agrees(t, a_kc, b_kc, 0, M, N, K, dict(res_dtype=rd, res_ld=N), dict(res=True))
                assert plan["variant"] in (None, 2 if rd == torch.float32 else 1), plan
            for bd, of in itertools.product((torch.bfloat16, torch.float32), (0, 1)):     # a bias
                _agrees(t, a_kc, b_kc, of, M, N, K, dict(bias_dtype=bd), dict(bias=True))
            _agrees(t, a_kc, b_kc, 1, M, N, K, dict(splitk=4), dict(splitk=4))     # split-K (f32 outputs only)
            _agrees(t, a_kc, b_kc, 0, M, N, K, dict(c_addr=4096 + 8), dict(c_aligned=False))     # a misaligned C
        # an operand extent past 2^30 elements (A when k-contiguous: M x lda, else K x lda; B likewise)
        for of in (0, 1):
            _agrees(t, a_kc, b_kc, of, 1 << 20, 128, 1024)
            _agrees(t, a_kc, b_kc, of, 128, 1 << 20, 1024)
            _agrees(t, a_kc, b_kc, of, 128, 128, 1024, dict(lda=1 << 21), dict(lda=1 << 21))
        # the fused projection's weight-major 3-batch: folded into one GEMM by 2562, else a real batch
        M, N, K = 1000, 512, 640
        fold = dict(batch=3, sA=0, sB=N * K, sC=N, ldc=3 * N)
        if a_kc and b_kc:
            plan = _agrees(t, 1, 1, 0, M, N, K, fold, fold)
            folded = plan["resolved_tile"] == 2562
            assert (plan["N"], plan["batch"]) == ((3 * N, 1) if folded else (N, 3)) and folded == (t % 100000 == 2562)
            for unfoldable, mk in ((dict(fold, bias_dtype=torch.float32), dict(fold, bias=True)),
                                   (dict(fold, sB=N * K + 8),) * 2, (dict(fold, sA=8),) * 2):
                plan = _agrees(t, 1, 1, 0, M, N, K, unfoldable, mk)
                assert (plan["N"], plan["batch"]) == (N, 3) and plan["resolved_tile"] != 2562
        # slab mode (weight gradients: m/n-contiguous operands, f32 slabs): an LDS-DMA tile or an error
        T, K2, N2, S = 448, 136, 72, 3
        slab = dict(sC=K2 * N2, splitk=S, slabs=True)
        if not a_kc and not b_kc and t % 100000 not in (64, 128):
            plan = _agrees(t, 0, 0, 1, K2, N2, T, slab, dict(sC=K2 * N2, splitk=S, slabs=True))
            assert plan["splitk"] == S and plan["kt_per_split"] == 3          # 7 K-tiles: 3 + 3 + 1
            assert plan["blocks"] == -(-K2 // plan["BM"]) * -(-N2 // plan["BN"]) * S
        else:
            assert _plan(t, a_kc, b_kc, 1, K2, N2, T, **slab)["err"] != 0
        assert _plan(t, a_kc, b_kc, 1, K2, N2, T, zero_c=True, **slab)["err"] != 0      # (slabs are not zeroed)
        assert _plan(t, a_kc, b_kc, 0, K2, N2, T, **slab)["err"] != 0                   # (... and are f32)


def test_plan_names_the_instances_the_gpu_tests_pin(planned):
    """The instance lists of tests/test_kernel_variants_gpu.py (imported, not copied), asked of the
    plan: name, block, block count, epilogue variant, split count."""
    import test_kernel_variants_gpu as tv
    for (tile, M, N, K, name), fam in [(c, "lean") for c in tv._LEAN] + [(c, "lds-dma") for c in tv._DMA_KK]:
        plan = _plan(tile, 1, 1, 0, M, N, K)
        bm, bn, wm, wn = tv._tile_of(name)
        assert plan["err"] == 0 and plan["name"] == name and plan["family"] == fam, plan
        assert plan["block"] == 64 * wm * wn and plan["blocks"] == -(-M // bm) * -(-N // bn)
        assert plan["resolved_tile"] == tile % 100000 and plan["splitk"] == 1 and plan["variant"] == 3
        assert (plan["BM"], plan["BN"], plan["WM"], plan["WN"]) == (bm, bn, wm, wn)
    import itertools
    m = _marks(tv.test_gemm_dma_layout_instances)
    for (a_kc, b_kc), of, (tile, M, N, K) in itertools.product(m["a_kc,b_kc"], m["out_f32"], m["tile,M,N,K"]):
        forced = 200000 if (tile == 1284 and a_kc and b_kc and not of) else 0
        plan = _plan(tile + forced, a_kc, b_kc, of, M, N, K)
        shape, bm = ("64,64,2,2,3", 64) if tile == 643 else ("128,128,2,2,4", 128)
        assert plan["name"] == f"gemm_dma<{shape},{tv._kc(a_kc)},{tv._kc(b_kc)},{'f32' if of else 'bf16'}>", plan
        assert plan["resolved_tile"] == tile and plan["grid"] == (-(-M // bm) * -(-N // bm), 1, 1)
        assert plan["block"] == 256 and plan["splitk"] == 1 and plan["family"] == "lds-dma"
    T, K, N, S = 448, 136, 72, 3                      # test_gemm_slab_instance's shape
    for tile, shape in _marks(tv.test_gemm_slab_instance)["tile,shape"]:
        plan = _plan(tile, 0, 0, 1, K, N, T, sC=K * N, splitk=S, slabs=True)
        assert plan["name"] == f"gemm_dma<{shape},mn,mn,f32>" and plan["variant"] == 3 and plan["family"] == "slab"
        assert plan["resolved_tile"] == tile and plan["splitk"] == S and plan["blocks"] == 2 * 1 * S
        assert plan["block"] == 64 * plan["WM"] * plan["WN"] == 64 * int(shape.split(",")[2]) * int(shape.split(",")[3])
    m = _marks(tv.test_gemm_register_staged_instances)
    M, N, K = 136, 72, 40
    for tile, (a_kc, b_kc, of) in itertools.product(m["tile"], m["a_kc,b_kc,out_f32"]):
        name = f"gemm_bf16<{tile},{tile},{tv._kc(a_kc)},{tv._kc(b_kc)},{'f32' if of else 'bf16'}>"
        for req in (tile, 644 if tile == 64 else 1282):
            plan = _plan(req, a_kc, b_kc, of, M, N, K)
            assert plan["name"] == name and plan["resolved_tile"] == tile and plan["family"] == "register-staged"
            assert plan["grid"] == (-(-M // tile) * -(-N // tile), 1, 1) and plan["block"] == 256
            assert plan["variant"] is None and plan["splitk"] == 1


def test_plan_epilogue_variants_and_grid(planned):
    """The compile-time epilogue instances of the k-contiguous bf16 kernels, general and lean alike,
    and the persistent grid: whole rounds of the resident slots, else one block per item."""
    import torch
    for tile in (1282, 201282, 2561, 202562, 644, 1602, 101602):
        kw = dict(tile=tile, a_kc=True, b_kc=True, out_f32=False)
        def variant(**more):
            return hip.gemm_plan(136, 72, 128, 128, 128, 72, **kw, **more)["variant"]
        assert variant() == 3                                              # plain
        assert variant(bias_dtype=torch.float32) == 4 == variant(bias_dtype=torch.float32, psum=True)
        assert variant(bias_dtype=torch.bfloat16) == 0 == variant(bias_dtype=torch.float32, relu=True)
        assert variant(alpha=0.5) == 0 == variant(bias_dtype=torch.float32, alpha=0.5)
        assert variant(psum=True) == (3 if tile % 100000 == 644 else 0)   # (no fused sums at 64x64)
    # 4096 x 4096 at 128x128, 2 blocks / CU: 1024 items are two whole rounds of 512 slots on 256 CUs
    plan = _plan(1282, 1, 1, 0, 4096, 4096, 64)
    assert plan["name"] == "gemm_lean<128,128,2,2,2>" and plan["grid"] == (512, 1, 1) and plan["mfast"] == 0
    assert _plan(1282, 1, 1, 0, 4096, 4096, 64, cus=304)["grid"] == (1024, 1, 1)      # 608 slots: no whole rounds
    assert _plan(1282, 1, 1, 0, 4096, 2048, 64)["grid"] == (512, 1, 1)                # one round: a block per item
    assert _plan(12884, 1, 1, 0, 4096, 4096, 64)["grid"] == (256, 1, 1)               # 8 waves: 1 block / CU
    assert _plan(1282, 1, 1, 0, 128, 4096, 64)["mfast"] == 1                          # fewer tile rows than columns


def test_plan_rejects_bias_and_relu_on_split_or_slab_calls(planned):
    """A split's partial is no output: the kernels add a bias only when splitk == 1 and would apply
    a ReLU to each partial, so the plan refuses both (after clamping the split count)."""
    import torch
    kw = dict(M=136, N=72, K=256, lda=136, ldb=72, ldc=72, a_kc=False, b_kc=False, out_f32=True, tile=1282)
    assert hip.gemm_plan(**kw, splitk=2)["err"] == 0
    for bad in (dict(relu=True), dict(bias_dtype=torch.float32), dict(bias_dtype=torch.bfloat16, relu=True)):
        assert hip.gemm_plan(**kw, splitk=2, **bad)["err"] != 0
        assert hip.gemm_plan(**kw, splitk=1, **bad)["err"] == 0
        assert hip.gemm_plan(**kw, splitk=9, **bad)["err"] != 0          # clamped to 4 splits: still split
        assert hip.gemm_plan(**kw, sC=136 * 72, splitk=2, slabs=True, **bad)["err"] != 0
        assert hip.gemm_plan(**kw, sC=136 * 72, splitk=1, slabs=True, **bad)["err"] != 0      # one slab is a slab
    assert hip.gemm_plan(**dict(kw, K=64), splitk=4, relu=True)["err"] == 0     # one K-tile: clamped to no split


def test_psum_slots_bounds_the_plans_partials(planned):
    """hip.psum_slots sizes the caller's buffer; the kernel writes the plan's psum count."""
    import itertools
    tiles, layouts, _, shapes = _layouts_matrix()
    shapes = list(shapes) + [(4096, 4096, 64), (1000, 512, 640)]
    counted = 0
    for t, f, (a_kc, b_kc), (M, N, K) in itertools.product(tiles, _FORCED, layouts, shapes):
        plan = _plan(t + f, a_kc, b_kc, 0, M, N, K, psum=True)
        assert plan["err"] == 0 and 0 <= plan["psum_count"] <= hip.psum_slots(M, N, 1), (t + f, M, N, K, plan)
        assert (plan["psum_count"] > 0) == (plan["family"] in ("lds-dma", "lean") and plan["BM"] >= 128), plan
        if plan["psum_count"]:
            items = -(-M // plan["BM"]) * -(-N // plan["BN"])       # one float per (item, wave)
            assert plan["psum_count"] == items * plan["WM"] * plan["WN"], plan
            counted += 1
    M, N, K = 1000, 512, 640
    plan = _plan(2562, 1, 1, 0, M, N, K, psum=True, batch=3, sA=0, sB=N * K, sC=N, ldc=3 * N)
    assert 0 < plan["psum_count"] == 4 * 8 * 8 <= hip.psum_slots(M, N, 3)      # folded: 4 x 8 tiles of 8 waves
    assert counted >= 54


def test_gemm_layouts_matrix_runs_every_tile_code_as_itself():
    """test_gemm_layouts (tests/test_kernels_gpu.py) names 13 tile codes; the launcher demotes a
    code its layout / output type / shape does not allow.  By the launcher's rules (resolved_tile,
    tests/test_kernel_variants_gpu.py) every code must stay itself for at least one case of that
    matrix, or the matrix never runs that kernel."""
    import itertools
    import test_kernels_gpu as tk
    from test_kernel_variants_gpu import resolved_tile
    params = {m.args[0]: m.args[1] for m in tk.test_gemm_layouts.pytestmark if m.name == "parametrize"}
    tiles, layouts, outs, shapes = params["tile"], params["a_kc,b_kc"], params["out_f32"], params["M,N,K"]
    assert len(tiles) == 13 and len(set(tiles)) == 13
    as_itself = {t: [] for t in tiles}
    for t, (a_kc, b_kc), of, (M, N, K) in itertools.product(tiles, layouts, outs, shapes):
        if resolved_tile(t, a_kc, b_kc, of, M, N, K) == t:
            as_itself[t].append((a_kc, b_kc, of, M, N, K))
    assert all(as_itself.values()), [t for t, v in as_itself.items() if not v]
    # and the forcing codes resolve to the plain one
    assert resolved_tile(101602, 1, 1, 0, 128, 160, 64) == 1602 == resolved_tile(201602, 1, 1, 0, 128, 160, 64)
    # spot checks of single rules: K no multiple of 64, a layout a tile does not have, f32 output
    assert resolved_tile(1282, 1, 1, 0, 136, 72, 40) == 128 and resolved_tile(644, 1, 1, 0, 136, 72, 40) == 64
    assert resolved_tile(2561, 1, 0, 0, 256, 192, 320) == 1284 and resolved_tile(2562, 1, 1, 1, 256, 192, 320) == 1282
    assert resolved_tile(2563, 1, 1, 1, 256, 192, 320) == 1282 and resolved_tile(12884, 1, 0, 0, 256, 192, 320) == 1282
