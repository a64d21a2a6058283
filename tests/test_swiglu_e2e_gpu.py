"""End-to-end on a real MI355X: one step of a causal RoPE TransformerLM with a gated (SwiGLU)
feed-forward (tests/test_embed.py lm_step) under VOCAB_PARALLEL_RULES, on one GPU and on a virtual
2 x 2 mesh, against the same step on host devices."""
import numpy as np
import pytest

from test_embed import lm_step

pytestmark = pytest.mark.gpu

# The layer and token count of tests/test_rope_e2e_gpu.py (16384 tokens through a 128-wide layer: see
# tests/test_xent_e2e_gpu.py SHAPE for why the gradient bound needs that many), with the gated
# feed-forward in place of the ReLU one.
LM = dict(vocab_size=1024, dim=128, layers=1, heads=2, dim_head=64, ff_dim=256, causal=True, rope_theta=10000.0,
          ff="swiglu")
BATCH, SEQ = 32, 512

_STEPS = {}


def _both_steps(mesh_shape, host_devices, gpu_devices):
    """The step on host devices and on the GPU for one mesh: run once, shared by the tests below.
    On the GPU the library's swiglu entry points are watched through the launch log."""
    if mesh_shape not in _STEPS:
        from learning_jax_sharding_amd.ops import kernels as K
        n = int(np.prod(mesh_shape))
        calls, ref = [], K.swiglu_reference
        K.swiglu_reference = lambda *a, **k: (calls.append(1), ref(*a, **k))[1]
        launches, saved = [], {}
        try:
            host_devices(n)
            host = lm_step(mesh_shape, LM, BATCH, SEQ)
            host_calls = len(calls)
            del calls[:]
            gpu_devices(n)
            from learning_jax_sharding_amd.ops import hip
            L = hip.lib()
            for fn in ("ljs_swiglu", "ljs_swiglu_bwd"):
                saved[fn] = getattr(L, fn)

                def watched(*a, _fn=saved[fn]):
                    with hip.launch_log() as log:
                        rc = _fn(*a)
                    launches.extend(r["name"] for r in log)
                    return rc
                setattr(L, fn, watched)
            gpu = lm_step(mesh_shape, LM, BATCH, SEQ)
            gpu_calls = len(calls)
        finally:
            K.swiglu_reference = ref
            for fn, f in saved.items():
                setattr(hip.lib(), fn, f)
        _STEPS[mesh_shape] = (host, gpu, launches, host_calls, gpu_calls)
    return _STEPS[mesh_shape]


@pytest.mark.parametrize("mesh_shape", [(1, 1), (2, 2)])
def test_gated_lm_step_runs_the_swiglu_kernels(host_devices, gpu_devices, mesh_shape):
    """Per layer (one) and device: one forward ``swiglu<bf16,bf16>`` launch for each forward pass of
    lm_step (model.init, the logits call, the step) and one ``swiglu_bwd<bf16,bf16>`` launch in the
    step's backward; the torch formulation is never called on the GPU; the loss matches the host step
    within 3e-2 max(1, |loss|)."""
    n = int(np.prod(mesh_shape))
    host, gpu, launches, host_calls, gpu_calls = _both_steps(mesh_shape, host_devices, gpu_devices)
    assert host_calls and not gpu_calls
    assert launches.count("swiglu<bf16,bf16>") == 3 * n, launches
    assert launches.count("swiglu_bwd<bf16,bf16>") == n, launches
    assert not [name for name in launches if not name.startswith("swiglu")], launches
    assert tuple(gpu[0].shape) == (BATCH, SEQ, LM["vocab_size"])
    vh, vg = host[1], gpu[1]
    print(f"swiglu-e2e {mesh_shape} loss host={vh:.6g} gpu={vg:.6g}")
    assert abs(vh - vg) <= 3e-2 * max(1.0, abs(vh)), (vh, vg)


@pytest.mark.parametrize("mesh_shape", [(1, 1), (2, 2)])
def test_gated_lm_step_gradients_match_host(host_devices, gpu_devices, mesh_shape):
    """Every parameter's gradient is finite; the embedding table's is within rtol 5e-2 and atol 5e-2
    max|host| of the host step's (the tolerances of tests/test_embed_e2e_gpu.py); the others' figures,
    the three feed-forward weights' among them, are printed."""
    host, gpu, *_ = _both_steps(mesh_shape, host_devices, gpu_devices)
    gh, gg = host[2], gpu[2]
    assert set(gh) == set(gg) and "embed/embedding" in gg
    assert {"layer_0/ff/w_gate", "layer_0/ff/w_up", "layer_0/ff/w_out"} <= set(gg) and "layer_0/ff/w_in" not in gg
    failed = []
    for name in sorted(gh):
        a, b = gh[name], gg[name]
        assert np.isfinite(b).all(), name
        bad = np.abs(b - a) > 5e-2 * np.abs(a) + 5e-2 * np.abs(a).max()
        print(f"swiglu-e2e {mesh_shape} {name} max|host|={np.abs(a).max():.4g} max|gpu-host|={np.abs(b - a).max():.4g} "
              f"outside={int(bad.sum())}/{bad.size}")
        if bad.any() and name.endswith("embedding"):
            failed.append(name)
    assert not failed, failed
