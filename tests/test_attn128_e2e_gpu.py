"""End-to-end on a real MI355X with LJS_ATTN_D128=1: one training step of a two-layer causal RoPE /
RMSNorm grouped-query TransformerLM with dim_head 128 against the host run, with no warning, the
attn128 kernels in the launch log, and equal losses from two replays of the captured step.

The feed-forward is the gated one (ff="swiglu", the Llama shape): with the default ReLU one the up-projection's
gradient misses test_gpu_e2e.py's tolerance on the GPU with the switch OFF already (the parent's torch
attention: 354 of 262144 elements of the second layer's, worst 2.5 x the tolerance), because a pre-activation
that rounds to the other side of zero flips its mask -- nothing the attention path decides."""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LM = dict(vocab_size=512, dim=256, layers=2, heads=2, kv_heads=1, dim_head=128, causal=True, rope_theta=10000.0,
          norm="rms", ff="swiglu")
BATCH, SEQ = 2, 96


def _setup():
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd import nn
    from learning_jax_sharding_amd.models import TransformerLM, lm_loss
    model = TransformerLM(**LM)
    gen = torch.Generator().manual_seed(5)
    ids = ljs.device_put(torch.randint(0, LM["vocab_size"], (BATCH, SEQ), generator=gen).numpy())
    labels = ljs.device_put(torch.randint(0, LM["vocab_size"], (BATCH, SEQ), generator=gen).numpy())
    params = model.init(ljs.random.PRNGKey(1), ids)["params"]
    vg = ljs.value_and_grad(lambda p: lm_loss(model, p, ids, labels))
    leaves = lambda g: [np.asarray(a, dtype=np.float32) for a in ljs.tree_util.tree_leaves(nn.unbox(g))]
    return ljs, vg, params, leaves


def test_lm_step_dim_head_128(host_devices, gpu_devices, monkeypatch):
    host_devices(1)
    _, vg, params, leaves = _setup()
    vh, gh = vg(params)
    vh, gh = float(np.asarray(vh)), leaves(gh)

    gpu_devices(1)
    monkeypatch.setenv("LJS_ATTN_D128", "1")
    from learning_jax_sharding_amd.ops import hip, kernels
    monkeypatch.setattr(kernels, "_WARNED_DH", set())
    ljs, vg, params, leaves = _setup()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        v, g = vg(params)
        vgpu, ggpu = float(np.asarray(v)), leaves(g)
    assert not [w for w in rec if issubclass(w.category, UserWarning)], [str(w.message) for w in rec]
    assert abs(vh - vgpu) <= 3e-2 * max(1.0, abs(vh)), (vh, vgpu)
    for i, (a, b) in enumerate(zip(gh, ggpu)):
        np.testing.assert_allclose(b, a, rtol=5e-2, atol=5e-2 * np.abs(a).max(), err_msg=f"leaf {i}")

    # the launch ring keeps 32 records, fewer than a step makes: read the record after each attention call
    seen = []
    fwd, bwd = hip._attn_fwd_call, hip._attn_bwd_call
    monkeypatch.setattr(hip, "_attn_fwd_call", lambda *a: (fwd(*a), seen.append(hip.last_launch()["name"]))[0])
    monkeypatch.setattr(hip, "_attn_bwd_call", lambda *a: (bwd(*a), seen.append(hip.last_launch()["name"]))[0])
    vg(params)
    assert seen == ["attn128_fwd<mask=1>"] * 2 + ["attn128_bwd<mask=1>"] * 2, seen

    graph = ljs.jit(vg, capture=True)
    losses = [float(np.asarray(graph(params)[0])) for _ in range(4)]   # warm-up and capture, then replays
    torch.cuda.synchronize()
    assert losses[-1] == losses[-2] and abs(losses[-1] - vgpu) <= 1e-3 * max(1.0, abs(vgpu)), (losses, vgpu)
