"""The attention launchers' instance choice, pinned on the CPU: ljs_attn_plan (hip.attn_plan) is the
plan step the entry points of csrc/kernels/attention.hip themselves run -- instance, grid, block,
vst, flags32 -- as a pure function, so the built library answers it without a GPU.  The Python
statements of the rules it is held to (_fwd_instances, _bwd_names, _BWD_SWITCHES) are the ones the
GPU oracle tests use, imported and not copied."""
import contextlib
import itertools
import os

import pytest

import attn_oracle as AO
from learning_jax_sharding_amd.ops import hip

# the table defaults of LJS_ATTN_SWITCHES, by hip._ATTN_SWITCHES name
_DEFAULTS = {"bwd_pair": 1, "dkv32": 1, "dq32": 1, "vst": 1, "cus": 0, "fwd_res": 8, "bwd_kv_dma": 2, "bwd_fused": 2,
             "bwd_proj": 2}
_SETTERS = {"bwd_pair": "set_attention_bwd_pair", "dkv32": "set_attention_dkv32", "dq32": "set_attention_dq32",
            "vst": "set_attention_vst", "cus": "set_attention_cus", "fwd_res": "set_attention_fwd_resident",
            "bwd_kv_dma": "set_attention_bwd_kv_dma", "bwd_fused": "set_attention_bwd_fused",
            "bwd_proj": "set_attention_bwd_proj"}


@pytest.fixture(scope="module")
def planned():
    if not os.path.exists(hip._LIBPATH):
        from learning_jax_sharding_amd.csrc import build
        build.build_all()
    hip.lib()


@contextlib.contextmanager
def _sw(**values):
    """Switches set through the public setters, all nine back at their defaults on the way out."""
    try:
        for name, v in values.items():
            getattr(hip, _SETTERS[name])(v)
        yield
    finally:
        for i in range(len(hip._ATTN_SWITCHES)):
            hip.lib().ljs_attn_set(i, -1)


def _plan(kind, shape, **kw):
    B, H, Sq, Sk, causal, q_off = shape
    return hip.attn_plan(kind, B, Sq, Sk, H, causal=causal, q_offset=q_off, **kw)


def _cdiv(a, b):
    return -(-a // b)


def _one(plan, name, grid, block, acc_mode=None):
    assert plan["err"] == 0 and plan["launches"] == [
        {"name": name, "grid": grid, "blocks": grid[0] * grid[1], "block": block, "acc_mode": acc_mode}], plan


# ============================================================================ switches
def test_switch_table_defaults_and_the_one_rule(planned):
    L = hip.lib()
    assert tuple(_DEFAULTS) == hip._ATTN_SWITCHES and set(_SETTERS) == set(_DEFAULTS)
    try:
        for i, name in enumerate(hip._ATTN_SWITCHES):
            assert L.ljs_attn_get(i) == _DEFAULTS[name], name
            assert L.ljs_attn_set(i, 5) == 0 and L.ljs_attn_get(i) == 5
            assert L.ljs_attn_set(i, -1) == 0 and L.ljs_attn_get(i) == _DEFAULTS[name], name
            assert L.ljs_attn_set(i, 0) == 0 and L.ljs_attn_get(i) == 0
            assert L.ljs_attn_set(i, -7) == 0 and L.ljs_attn_get(i) == _DEFAULTS[name], name
        assert L.ljs_attn_set(9, 1) != 0 and L.ljs_attn_set(-1, 1) != 0 and L.ljs_attn_get(9) == -1
        # the public setters' None / True / False / int meanings
        for name in hip._ATTN_SWITCHES:
            i, setter = hip._ATTN_SWITCHES.index(name), getattr(hip, _SETTERS[name])
            for v, want in ((True, 1), (False, 0), (None, _DEFAULTS[name])) if name not in ("cus", "fwd_res") else \
                    ((4, 4), (0, 0), (-1, _DEFAULTS[name])):
                setter(v)
                assert L.ljs_attn_get(i) == want, (name, v)
        hip.set_attention_cus(None)
        assert L.ljs_attn_get(hip._ATTN_SWITCHES.index("cus")) == 0
    finally:
        for i in range(9):
            L.ljs_attn_set(i, -1)


# ============================================================================ forward
def test_forward_plan_is_the_instance_the_oracle_tests_allow(planned):
    from test_attention_oracle_gpu import _fwd_instances
    shapes = sorted(set(AO.FWD_SHAPES + AO.FWD_KIND_SHAPES + AO.FWD_TILED_ONLY))
    assert len(shapes) == 11
    for shape, res in itertools.product(shapes, (-1, 8, 4, 0)):
        B, H, Sq, Sk, _, _ = shape
        allowed = _fwd_instances(shape)
        want = {-1: allowed[-1], 8: allowed[-1], 4: allowed[min(1, len(allowed) - 1)], 0: allowed[0]}[res]
        with _sw(fwd_res=res):
            plan = _plan("fwd", shape)
        nw = {"attn_fwd_res<8>": 8, "attn_fwd_res<4>": 4, "attn_fwd_tiled<1>": 0}[want]
        nqb = _cdiv(Sq, 16 * nw) if nw else _cdiv(Sq, 64)
        _one(plan, want, (nqb * H * B, 1, 1), 64 * nw if nw else 256, acc_mode=0)
        assert (plan["nw"], plan["nqb"], plan["vst"][0]) == (nw, nqb, 1), (shape, res, plan)
    assert all(_plan("fwd", s)["launches"][0]["name"] == "attn_fwd_tiled<1>" for s in AO.FWD_TILED_ONLY)


def test_forward_resident_limit_and_vst(planned):
    """The resident kernel addresses K / V with 32-bit byte offsets: a row stride for which
    (Sk - 1) stride 2 + 128 reaches 2^31 plans the tiled kernel; the larger of the K and V strides
    decides."""
    shape = (2, 3, 256, 256, False, 0)
    fits, over = 4210744, 4210760
    assert 255 * fits * 2 + 128 < 2 ** 31 <= 255 * over * 2 + 128
    for op in ("k", "v"):
        assert _plan("fwd", shape, strides={op: (256 * fits, fits, 64)})["launches"][0]["name"] == "attn_fwd_res<4>"
        assert _plan("fwd", shape, strides={op: (256 * over, over, 64)})["launches"][0]["name"] == "attn_fwd_tiled<1>"
    # vst: the output 16-byte aligned with strides % 8 == 0, and the switch
    assert _plan("fwd", shape, addrs={"o": 4096 + 8})["vst"][0] == 0
    assert _plan("fwd", shape, strides={"o": (256 * 196, 196, 64)})["vst"][0] == 0
    with _sw(vst=False):
        assert _plan("fwd", shape)["vst"][0] == 0


def test_forward_acc_check(planned):
    shape = (2, 4, 128, 128, True, 0)
    for mode in (1, 2, 3):
        _one(_plan("fwd_acc", shape, acc_mode=mode), "attn_fwd_res<4>", (2 * 4 * 2, 1, 1), 256, acc_mode=mode)
    _one(_plan("fwd_acc", (2, 4, 128, 300, True, 0), acc_mode=2), "attn_fwd_tiled<1>", (2 * 4 * 2, 1, 1), 256, 2)
    for kw in (dict(acc_mode=0), dict(acc_mode=4), dict(acc_mode=2, addrs={"oacc": 4096 + 8}),
               dict(acc_mode=2, addrs={"oacc": 0}), dict(acc_mode=2, addrs={"lse": 0}),
               dict(acc_mode=2, strides={"oacc": (128 * 258, 258, 64)}),
               dict(acc_mode=2, strides={"oacc": (128 * 256, 256, 66)}),
               dict(acc_mode=2, strides={"oacc": (128 * 256 + 2, 256, 64)})):
        plan = _plan("fwd_acc", shape, **kw)
        assert plan["err"] != 0 and plan["launches"] == [], (kw, plan)
    # o is written by the last hop only
    assert _plan("fwd_acc", shape, acc_mode=1, addrs={"o": 0})["err"] == 0
    assert _plan("fwd_acc", shape, acc_mode=3, addrs={"o": 0})["err"] != 0


# ============================================================================ backward
def _bwd_shapes():
    return sorted(set(AO.BWD_SHAPES + [AO.BWD_KIND_SHAPE, AO.BWD_NEG_OFFSET, (2, 3, 128, 128, True, 128)]))


def _bwd_grids(names, shape):
    """The launcher's grid formulas, by launch name."""
    B, H, Sq, Sk, _, _ = shape
    nq, nk, nq128, nk128 = _cdiv(Sq, 64), _cdiv(Sk, 64), _cdiv(Sq, 128), _cdiv(Sk, 128)
    per_head = {"attn_bwd_pair32<dq32=1>": nq128 + nk128, "attn_bwd_pair32<dq32=0>": nq + nk128,
                "attn_bwd_pair": nq + nk, "attn_bwd_dq": nq, "attn_bwd_dkv": nk}
    return [((H, B, 1), 512) if n.startswith("attn_bwd_fused") else ((per_head[n] * H * B, 1, 1), 256) for n in names]


def _check_bwd(plan, names, shape):
    assert plan["err"] == 0 and [r["name"] for r in plan["launches"]] == names, (shape, names, plan)
    for rec, (grid, block) in zip(plan["launches"], _bwd_grids(names, shape)):
        assert (rec["grid"], rec["blocks"], rec["block"], rec["acc_mode"]) == (grid, grid[0] * grid[1], block, None), \
            (shape, rec)


def test_backward_plan_names_every_instance_as_the_oracle_tests_do(planned):
    from test_attention_oracle_gpu import _BWD_SWITCHES, _bwd_names, _switches
    seen = set()
    for shape, inst in itertools.product(_bwd_shapes(), _BWD_SWITCHES):
        # the fused kernel holds at most 256 keys: above, its switch rows run the default split kernel
        names = (_bwd_names(inst, shape) if shape[3] <= 256 or not inst.startswith("attn_bwd_fused")
                 else ["attn_bwd_pair32<dq32=1>"])
        with _sw(), _switches(hip, inst):
            plan = _plan("bwd", shape)
        _check_bwd(plan, names, shape)
        assert plan["flags32"] == int(names == ["attn_bwd_pair32<dq32=1>"])
        assert plan["vst"] == ((1, 0) if names[0].startswith("attn_bwd_fused") else (1, 1))
        seen.update(names)
    assert len(seen) == 9, seen


def test_backward_plan_defaults(planned):
    """Under the defaults: fused iff Sk <= 256 and B H >= 128, LDS-DMA staging iff Sq <= 128, the
    sw = 1 sweep as _bwd_names states it, else the 128-key pair kernel."""
    from test_attention_oracle_gpu import _bwd_names
    for shape in _bwd_shapes():                                     # (all below 128 (batch, head) pairs)
        _check_bwd(_plan("bwd", shape), ["attn_bwd_pair32<dq32=1>"], shape)
    for (B, H), Sk, Sq, causal in itertools.product(((15, 8), (16, 8), (127, 1), (128, 1), (64, 8)),
                                                    (128, 256, 257, 320), (64, 128, 129, 192, 256), (False, True)):
        shape = (B, H, Sq, Sk, causal, 0)
        if Sk <= 256 and B * H >= 128:
            names = _bwd_names(f"attn_bwd_fused<dma={int(Sq <= 128)}>", shape)
        else:
            names = ["attn_bwd_pair32<dq32=1>"]
        _check_bwd(_plan("bwd", shape), names, shape)


def test_backward_sweep_needs_row_stores(planned):
    """sw = 1 only with vst = 1: an output address or stride that breaks the 16-byte row stores, or
    the switch, plans sw = 0 and hands the kernel vst = 0."""
    shape = (64, 8, 256, 256, False, 0)
    B, H, S = 64, 8, 256
    _check_bwd(_plan("bwd", shape), ["attn_bwd_fused<dma=0,sw=1>"], shape)
    broken = [dict(addrs={n: 4096 + 8}) for n in ("dq", "dk", "dv")]
    broken += [dict(strides={n: st}) for n in ("dq", "dk", "dv")
               for st in ((S * H * 64 + 4, H * 64, 64), (S * (H * 64 + 4), H * 64 + 4, 64), (S * H * 68, H * 68, 68))]
    for kw in broken:
        plan = _plan("bwd", shape, **kw)
        _check_bwd(plan, ["attn_bwd_fused<dma=0,sw=0>"], shape)
        assert plan["vst"][0] == 0, (kw, plan)
    with _sw(vst=False):
        plan = _plan("bwd", shape)
    _check_bwd(plan, ["attn_bwd_fused<dma=0,sw=0>"], shape)
    # the split kernels: dQ's vst and dK / dV's apart
    split = (2, 3, 320, 320, True, 0)
    assert _plan("bwd", split, addrs={"dq": 4096 + 8})["vst"] == (0, 1)
    assert _plan("bwd", split, addrs={"dv": 4096 + 8})["vst"] == (1, 0)
    # inputs do not enter it
    assert _plan("bwd", shape, addrs={"q": 4096 + 8, "dout": 4096 + 2})["vst"][0] == 1


# ============================================================================ attn_bwd_proj
def _proj(B, Sq, Sk, H, M, dy_ld, causal=False, **kw):
    return hip.attn_plan("bwd_proj", B, Sq, Sk, H, causal=causal, M=M, dy_ld=dy_ld, **kw)


def test_projection_shape_gate(planned):
    """tests/test_attn_bwd_proj_walk.py::test_shape_gate's cases (the head_dim one is Python's), and
    what the entry point's gate adds on addresses and strides."""
    with _sw(bwd_proj=True):
        _one(_proj(64, 256, 256, 8, 640, 0), "attn_bwd_proj", (512, 1, 1), 512)          # dy_ld = 0: one row for all
        _one(_proj(1, 256, 256, 1, 32, 32), "attn_bwd_proj", (1, 1, 1), 512)
        _one(_proj(1, 256, 256, 1, 32, 40), "attn_bwd_proj", (1, 1, 1), 512)
        assert _proj(64, 256, 256, 8, 640, 640)["vst"][0] == 1
        for args in ((64, 256, 256, 8, 40, 40), (64, 128, 256, 8, 640, 640), (64, 256, 128, 8, 640, 640),
                     (64, 256, 256, 8, 640, 636), (64, 256, 256, 8, 640, 644), (0, 256, 256, 8, 640, 640),
                     (64, 256, 256, 0, 640, 640), (64, 256, 256, 8, 0, 0)):
            plan = _proj(*args)
            assert plan["err"] != 0 and plan["launches"] == [], (args, plan)
        assert _proj(64, 256, 256, 8, 640, 640, causal=True)["err"] != 0
        ok = (64, 256, 256, 8, 640, 640)
        for n in ("dy", "w", "q", "k", "v", "o", "dq", "dk", "dv"):                        # 16-byte alignment
            assert _proj(*ok, addrs={n: 4096 + 8})["err"] != 0, n
            assert _proj(*ok, addrs={n: 0})["err"] != 0, n
        assert _proj(*ok, addrs={"lse": 4096 + 2})["err"] != 0 and _proj(*ok, addrs={"lse": 4096 + 4})["err"] == 0
        for n in ("q", "k", "v", "o", "dq", "dk", "dv"):                                   # strides % 8
            assert _proj(*ok, strides={n: (256 * 516, 516, 64)})["err"] != 0, n
            assert _proj(*ok, strides={n: (256 * 3 * 512, 3 * 512, 64)})["err"] == 0, n    # (a fused-QKV slice)
        for n in ("q", "k", "v", "o"):                                                     # 32-bit byte offsets
            fits, over = 4210744, 4210752                                                  # 2 (255 stride + 64) < 0x7ffffff0
            assert _proj(*ok, strides={n: (256 * fits, fits, 64)})["err"] == 0, n
            assert _proj(*ok, strides={n: (256 * over, over, 64)})["err"] != 0, n
            assert _proj(*ok, strides={n: (256 * 512, -512, 64)})["err"] != 0, n
        assert _proj(64, 256, 256, 8, 640, 4210744)["err"] == 0                            # (dy rows likewise)
        assert _proj(64, 256, 256, 8, 640, 4210752)["err"] != 0


def test_projection_automatic_gate(planned):
    """tests/test_attn_bwd_proj_gpu.py::test_automatic_gate's rule over B H = 32 / 128 / 192 / 512 and
    the settings of bwd_proj, bwd_fused and vst, asked of the exported predicate and of the plan."""
    for (B, H), proj, fused, vst in itertools.product(((4, 8), (16, 8), (24, 8), (64, 8)), (None, True, False),
                                                      (None, True, False), (None, False)):
        want = (proj is not False and vst is None
                and (proj is True or (fused is not False and B * H >= 192)))
        with _sw(bwd_proj=proj, bwd_fused=fused, vst=vst):
            assert bool(hip.lib().ljs_attn_bwd_proj_enabled(B, H)) == want, (B, H, proj, fused, vst)
            assert (_proj(B, 256, 256, H, 640, 640)["err"] == 0) == want, (B, H, proj, fused, vst)
    L = hip.lib()
    try:
        L.ljs_attn_set(hip._ATTN_SWITCHES.index("vst"), 2)       # (dK / dV staged, per-lane dQ: not vst = 1)
        hip.set_attention_bwd_proj(True)
        assert not L.ljs_attn_bwd_proj_enabled(64, 8) and _proj(64, 256, 256, 8, 640, 640)["err"] != 0
    finally:
        with _sw():
            pass


def test_projection_ok_asks_the_plan(planned):
    """hip.attn_bwd_proj_ok on CPU tensors (it reads addresses and strides only): the library's gate
    plus what only Python sees."""
    import torch
    B, H, S, M = 1, 2, 256, 64
    bf = torch.bfloat16
    q, k, v, o = (torch.empty(B, S, H, 64, dtype=bf) for _ in range(4))
    dy, w = torch.empty(B * S, M, dtype=bf), torch.empty(H * 64, M, dtype=bf)
    with _sw(bwd_proj=True):
        assert hip.attn_bwd_proj_ok(q, k, v, o, dy, M, w, False)
        assert hip.attn_bwd_proj_ok(q, k, v, o, dy, M, w, False, outs=(q, k, v))
        assert not hip.attn_bwd_proj_ok(q, k, v, o, dy, M, w, True)
        assert not hip.attn_bwd_proj_ok(q.float(), k, v, o, dy, M, w, False)
        assert not hip.attn_bwd_proj_ok(q, k, v, o, dy.float(), M, w, False)
        assert not hip.attn_bwd_proj_ok(q, k, v, o, dy, M, w.t(), False)                    # w not contiguous
        assert not hip.attn_bwd_proj_ok(q, k, v, o, dy, M, w[:64], False)                   # w.shape[0] != H * 64
        q32 = torch.empty(B, S, H, 32, dtype=bf)
        assert not hip.attn_bwd_proj_ok(q32, q32, q32, q32, dy, M, w[:64], False)           # head_dim
        odd = torch.empty(B, S, H, 68, dtype=bf)[..., 2:66]                                 # 4 bytes off, strides % 8 != 0
        assert not hip.attn_bwd_proj_ok(q, k, v, o, dy, M, w, False, outs=(odd, k, v))
        assert not hip.attn_bwd_proj_ok(q[:, :128], k, v, o, dy, M, w, False)               # 128 queries
    assert not hip.attn_bwd_proj_ok(q, k, v, o, dy, M, w, False)                            # automatic: B H < 192


# ============================================================================ qkv_attn_fwd
def _qkv(B, H, K, **kw):
    return hip.attn_plan("qkv_fwd", B, kw.pop("S", 256), 256, H, K=K, **kw)


def test_qkv_forward_grid_and_argument_check(planned):
    _one(_qkv(1, 2, 128), "qkv_attn_fwd", (2, 1, 1), 512)
    _one(_qkv(64, 8, 640), "qkv_attn_fwd", (256, 1, 1), 512)
    _one(_qkv(64, 8, 640, cus=304), "qkv_attn_fwd", (304, 1, 1), 512)
    _one(_qkv(16, 8, 640, cus=304), "qkv_attn_fwd", (128, 1, 1), 512)
    with _sw(cus=3):
        _one(_qkv(64, 8, 640), "qkv_attn_fwd", (3, 1, 1), 512)
        _one(_qkv(1, 2, 128), "qkv_attn_fwd", (2, 1, 1), 512)
    assert _qkv(1, 2, 128, ldx=136)["err"] == 0
    for kw in (dict(S=255), dict(S=0), dict(K=192), dict(K=64), dict(K=0), dict(N=64 * 2 + 64), dict(N=64),
               dict(ldx=132), dict(ldx=120), dict(addrs={"x": 4096 + 8}), dict(addrs={"w": 4096 + 8}),
               dict(addrs={"qkv": 4096 + 8}), dict(addrs={"o": 4096 + 8})):
        plan = _qkv(1, 2, kw.pop("K", 128), **kw)
        assert plan["err"] != 0 and plan["launches"] == [], (kw, plan)
    assert _qkv(1, 0, 128, N=0)["err"] != 0
    assert _qkv(1 << 12, 2, 1024)["err"] != 0                  # x past 2^31 bytes


# ============================================================================ grids that do not fit, null operands
def test_grid_overflow_and_null_operands_are_errors(planned):
    """A grid from 2^30 blocks up (the pair kernels' bound) and a missing operand: hipErrorInvalidValue
    and nothing planned.  No tensor that fits in memory reaches the former."""
    B, H = 1 << 13, 1 << 10
    for kind, kw in (("fwd", {}), ("fwd_acc", dict(acc_mode=2))):
        _one(_plan(kind, (B, H, 64 * 127, 320, False, 0), **kw), "attn_fwd_tiled<1>", (127 << 23, 1, 1), 256,
             kw.get("acc_mode", 0))
        plan = _plan(kind, (B, H, 64 * 128, 320, False, 0), **kw)
        assert plan["err"] != 0 and plan["launches"] == [], plan
        _one(_plan(kind, (B, H, 64 * 127, 256, False, 0), **kw), "attn_fwd_res<8>", (64 << 23, 1, 1), 512,
             kw.get("acc_mode", 0))
        assert _plan(kind, (B, H, 128 * 128, 256, False, 0), **kw)["err"] != 0
    # backward: the pair kernels' own tests fall through to the two launches, which then do not fit either
    _check_bwd(_plan("bwd", (B, H, 64 * 60, 64 * 60, False, 0)), ["attn_bwd_pair32<dq32=1>"],
               (B, H, 64 * 60, 64 * 60, False, 0))
    _check_bwd(_plan("bwd", (B, H, 64 * 90, 64 * 90, False, 0)), ["attn_bwd_dq", "attn_bwd_dkv"],
               (B, H, 64 * 90, 64 * 90, False, 0))
    plan = _plan("bwd", (B, H, 64 * 128, 64 * 128, False, 0))
    assert plan["err"] != 0 and plan["launches"] == [], plan
    with _sw(dkv32=False, bwd_pair=False):                                   # (the second launch alone)
        _check_bwd(_plan("bwd", (B, H, 64, 64 * 127, False, 0)), ["attn_bwd_dq", "attn_bwd_dkv"],
                   (B, H, 64, 64 * 127, False, 0))
        assert _plan("bwd", (B, H, 64, 64 * 128, False, 0))["err"] != 0
    shape = (2, 3, 256, 256, False, 0)
    for n in ("q", "k", "v", "o", "lse"):
        assert _plan("fwd", shape, addrs={n: 0})["err"] != 0, n
    for n in ("q", "k", "v", "o", "lse", "dout", "delta", "dq", "dk", "dv"):
        plan = _plan("bwd", shape, addrs={n: 0})
        assert plan["err"] != 0 and plan["launches"] == [], (n, plan)
