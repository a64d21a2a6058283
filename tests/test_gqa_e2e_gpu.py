"""End-to-end on a real MI355X: one step of the causal RoPE SwiGLU TransformerLM of
tests/test_swiglu_e2e_gpu.py with grouped-query attention (heads=4, kv_heads=2) under
VOCAB_PARALLEL_RULES, on one GPU and on a virtual 2 x 2 mesh, against the same step on host devices."""
import numpy as np
import pytest

from test_embed import lm_step
from test_swiglu_e2e_gpu import BATCH, LM as SWIGLU_LM, SEQ

pytestmark = pytest.mark.gpu

LM = dict(SWIGLU_LM, heads=4, kv_heads=2)

# the library's attention entry points, multi-head and grouped-query, and the fold
_WATCHED = ("ljs_attn_fwd", "ljs_attn_fwd_acc", "ljs_attn_bwd", "ljs_attn_bwd_proj", "ljs_qkv_attn_fwd",
            "ljs_attn_fwd_gqa", "ljs_attn_fwd_acc_gqa", "ljs_attn_bwd_gqa", "ljs_gqa_reduce")
_STEPS = {}


def _gpu_step(mesh_shape, lm, gpu_devices):
    """(lm_step's result, [(entry point, launch names)], torch attention calls) of one step on the GPU."""
    from learning_jax_sharding_amd.ops import kernels as K
    n = int(np.prod(mesh_shape))
    calls, ref = [], K.attention_reference
    K.attention_reference = lambda *a, **k: (calls.append(1), ref(*a, **k))[1]
    launches, saved = [], {}
    gpu_devices(n)
    from learning_jax_sharding_amd.ops import hip
    L = hip.lib()
    try:
        for fn in _WATCHED:
            saved[fn] = getattr(L, fn)

            def watched(*a, _fn=saved[fn], _name=fn):
                with hip.launch_log() as log:
                    rc = _fn(*a)
                launches.append((_name, [r["name"] for r in log]))
                return rc
            setattr(L, fn, watched)
        res = lm_step(mesh_shape, lm, BATCH, SEQ)
    finally:
        K.attention_reference = ref
        for fn, f in saved.items():
            setattr(L, fn, f)
    return res, launches, len(calls)


def _both_steps(mesh_shape, host_devices, gpu_devices):
    if mesh_shape not in _STEPS:
        host_devices(int(np.prod(mesh_shape)))
        host = lm_step(mesh_shape, LM, BATCH, SEQ)
        _STEPS[mesh_shape] = (host,) + _gpu_step(mesh_shape, LM, gpu_devices)
    return _STEPS[mesh_shape]


@pytest.mark.parametrize("mesh_shape", [(1, 1), (2, 2)])
def test_gqa_lm_step_runs_the_gqa_kernels(host_devices, gpu_devices, mesh_shape):
    """Per layer (one), device and backward (one) a ``gqa_reduce`` launch behind the backward kernels of
    ``ljs_attn_bwd_gqa``; three forwards per device (model.init, the logits call, the step) through
    ``ljs_attn_fwd_gqa``; no ``qkv_attn_fwd`` or ``attn_bwd_proj`` launch, no multi-head entry point;
    the torch attention formulation is never called on the GPU; the loss matches the host step within
    3e-2 max(1, |loss|) (tests/test_swiglu_e2e_gpu.py)."""
    n = int(np.prod(mesh_shape))
    host, gpu, launches, torch_calls = _both_steps(mesh_shape, host_devices, gpu_devices)
    assert torch_calls == 0
    by_entry = {}
    for fn, names in launches:
        by_entry.setdefault(fn, []).append(names)
    assert set(by_entry) == {"ljs_attn_fwd_gqa", "ljs_attn_bwd_gqa", "ljs_gqa_reduce"}, sorted(by_entry)
    assert len(by_entry["ljs_attn_fwd_gqa"]) == 3 * n and len(by_entry["ljs_attn_bwd_gqa"]) == n
    assert by_entry["ljs_gqa_reduce"] == [["gqa_reduce"]] * n
    names = [x for _, ns in launches for x in ns]
    assert "qkv_attn_fwd" not in names and "attn_bwd_proj" not in names
    assert all(len(ns) == 1 and ns[0].startswith("attn_fwd") for ns in by_entry["ljs_attn_fwd_gqa"]), by_entry
    assert all(ns and all(x.startswith("attn_bwd") for x in ns) for ns in by_entry["ljs_attn_bwd_gqa"]), by_entry
    assert tuple(gpu[0].shape) == (BATCH, SEQ, LM["vocab_size"])
    vh, vg = host[1], gpu[1]
    print(f"gqa-e2e {mesh_shape} loss host={vh:.6g} gpu={vg:.6g}")
    assert abs(vh - vg) <= 3e-2 * max(1.0, abs(vh)), (vh, vg)


@pytest.mark.parametrize("mesh_shape", [(1, 1), (2, 2)])
def test_gqa_lm_step_gradients_match_host(host_devices, gpu_devices, mesh_shape):
    """Every parameter's gradient is finite; the embedding table's is within rtol 5e-2 and atol 5e-2
    max|host| of the host step's (the criteria of tests/test_swiglu_e2e_gpu.py); the others' figures,
    the narrow K / V kernels' among them, are printed."""
    host, gpu, *_ = _both_steps(mesh_shape, host_devices, gpu_devices)
    gh, gg = host[2], gpu[2]
    assert set(gh) == set(gg) and "embed/embedding" in gg
    assert gg["layer_0/attn/to_k/kernel"].shape == (128, 128) and gg["layer_0/attn/to_v/kernel"].shape == (128, 128)
    assert gg["layer_0/attn/to_q/kernel"].shape == (128, 256)
    failed = []
    for name in sorted(gh):
        a, b = gh[name], gg[name]
        assert np.isfinite(b).all(), name
        bad = np.abs(b - a) > 5e-2 * np.abs(a) + 5e-2 * np.abs(a).max()
        print(f"gqa-e2e {mesh_shape} {name} max|host|={np.abs(a).max():.4g} max|gpu-host|={np.abs(b - a).max():.4g} "
              f"outside={int(bad.sum())}/{bad.size}")
        if bad.any() and name.endswith("embedding"):
            failed.append(name)
    assert not failed, failed


def test_kv_heads_none_leaves_the_multi_head_launches(gpu_devices):
    """The same model with ``kv_heads=None`` and with the field absent: the same attention entry points
    and instance names in the same order, none of them a grouped-query one."""
    lm_none, lm_absent = dict(LM, kv_heads=None), {k: v for k, v in LM.items() if k != "kv_heads"}
    _, with_none, _ = _gpu_step((1, 1), lm_none, gpu_devices)
    _, absent, _ = _gpu_step((1, 1), lm_absent, gpu_devices)
    assert with_none == absent and with_none
    assert not [fn for fn, _ in with_none if fn.endswith("_gqa") or fn == "ljs_gqa_reduce"], with_none
