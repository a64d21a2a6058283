"""End-to-end on a real MI355X: one TransformerLM step from token ids to the mean cross-entropy loss
(tests/test_embed.py lm_step: token + position Embed -> pre-norm TransformerLayer -> RMSNorm ->
Dense(vocab) -> loss) under VOCAB_PARALLEL_RULES, on one GPU and on a virtual 2 x 2 mesh whose model
axis shards both tables' rows and the head's columns, against the same step on host devices."""
import numpy as np
import pytest
import torch

from test_embed import lm_step

pytestmark = pytest.mark.gpu

# The layer and token count of tests/test_xent_e2e_gpu.py (16384 tokens through a 128-wide layer, see
# its SHAPE for why the gradient bound needs that many), with a 1024-row token table in front.
LM = dict(vocab_size=1024, dim=128, layers=1, heads=2, dim_head=64, ff_dim=256, max_len=512)
BATCH, SEQ = 32, 512
_INDEX_OPS = ("index", "index_select", "embedding", "embedding_dense_backward", "index_add", "index_add_",
              "index_put", "index_put_", "_index_put_impl_", "_unsafe_index")

_STEPS = {}


def _both_steps(mesh_shape, host_devices, gpu_devices, monkeypatch):
    """The step on host devices and on the GPU for one mesh: run once, shared by the tests below.
    The GPU step runs under utils.aten_trace (which torch kernels it reached) with the two embedding
    entry points of the library watched through the launch log."""
    if mesh_shape not in _STEPS:
        from learning_jax_sharding_amd.ops import kernels as K
        from learning_jax_sharding_amd.utils.aten_trace import AtenTrace
        n = int(np.prod(mesh_shape))
        calls, ref = [], K.embed_reference
        K.embed_reference = lambda *a, **k: (calls.append(1), ref(*a, **k))[1]
        launches, saved = [], {}
        try:
            host_devices(n)
            host = lm_step(mesh_shape, LM, BATCH, SEQ)
            host_calls = len(calls)
            del calls[:]
            gpu_devices(n)
            from learning_jax_sharding_amd.ops import hip
            L = hip.lib()
            for fn in ("ljs_embed_fwd", "ljs_embed_bwd"):
                saved[fn] = getattr(L, fn)

                def watched(*a, _fn=saved[fn]):
                    with hip.launch_log() as log:
                        rc = _fn(*a)
                    launches.extend(r["name"] for r in log)
                    return rc
                setattr(L, fn, watched)
            monkeypatch.setenv("LJS_ATEN_TRACE", "1")   # the backward on this thread, where the tracer sees it
            with AtenTrace() as trace:
                gpu = lm_step(mesh_shape, LM, BATCH, SEQ)
            gpu_calls = len(calls)
        finally:
            K.embed_reference = ref
            for fn, f in saved.items():
                setattr(hip.lib(), fn, f)
        index_ops = sorted({op for (op, _, _) in trace.calls if op.split(".")[1] in _INDEX_OPS})
        _STEPS[mesh_shape] = (host, gpu, launches, host_calls, gpu_calls, index_ops)
    return _STEPS[mesh_shape]


@pytest.mark.parametrize("mesh_shape", [(1, 1), (2, 2)])
def test_lm_step_runs_the_embedding_kernels(host_devices, gpu_devices, monkeypatch, mesh_shape):
    """On every device the token and the position lookup take embed_fwd (three times: model.init, the
    logits and the step) and embed_bwd (with its embed_combine: thousands of tokens per device); the torch formulation is never called and no torch index kernel runs; on
    2 x 2 both lookups run over two vocabulary shards; the loss matches the host step."""
    n = int(np.prod(mesh_shape))
    host, gpu, launches, host_calls, gpu_calls, index_ops = _both_steps(mesh_shape, host_devices, gpu_devices,
                                                                        monkeypatch)
    assert host_calls and not gpu_calls
    assert not index_ops, index_ops
    assert launches.count("embed_fwd<f32,bf16>") == 6 * n, launches
    assert launches.count("embed_bwd<bf16>") == 2 * n and launches.count("embed_combine") == 2 * n, launches
    assert host[3] == gpu[3] == [(mesh_shape[1], 1)] * 4
    assert tuple(gpu[0].shape) == (BATCH, SEQ, LM["vocab_size"])
    vh, vg = host[1], gpu[1]
    print(f"embed-e2e {mesh_shape} loss host={vh:.6g} gpu={vg:.6g}")
    assert abs(vh - vg) <= 3e-2 * max(1.0, abs(vh)), (vh, vg)


@pytest.mark.parametrize("mesh_shape", [(1, 1), (2, 2)])
def test_lm_step_table_gradients_match_host(host_devices, gpu_devices, monkeypatch, mesh_shape):
    """The two tables' gradients (and every other parameter's, printed) against the host step: rtol
    5e-2 and atol 5e-2 max|host|, what tests/test_xent_e2e_gpu.py allows for parameters upstream of
    the bf16 layer."""
    host, gpu, *_ = _both_steps(mesh_shape, host_devices, gpu_devices, monkeypatch)
    gh, gg = host[2], gpu[2]
    assert set(gh) == set(gg)
    failed = []
    for name in sorted(gh):
        a, b = gh[name], gg[name]
        assert np.isfinite(b).all(), name
        bad = np.abs(b - a) > 5e-2 * np.abs(a) + 5e-2 * np.abs(a).max()
        print(f"embed-e2e {mesh_shape} {name} max|host|={np.abs(a).max():.4g} max|gpu-host|={np.abs(b - a).max():.4g} "
              f"outside={int(bad.sum())}/{bad.size}")
        if bad.any() and name.endswith("embedding"):
            failed.append(name)
    assert not failed, failed
