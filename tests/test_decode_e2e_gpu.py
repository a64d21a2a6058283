"""Cached decoding end to end on a real MI355X: tests/test_decode.py's model rule on the GPU

    max|C - R| <= 4 max|A - R| + 2^-23 max|R|

(``R``: the float32 uncached logits, computed on the host; ``A``: the bf16 uncached logits on the GPU;
``C``: the bf16 cached logits on the GPU) at batch 8, at batch 2 (the dense layers' torch fallback) and
with ``LJS_FUSED_DECODE=0``; a captured decode step against the eager one, bit for bit; ``generate``
captured against eager; two virtual devices with the batch sharded against one."""
import numpy as np
import pytest
import torch

from test_decode import (LM, STEPS, lm_params, mesh_setup, rule_check, teacher_forced, tokens, uncached_logits)

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
PLENS8 = [5, 9, 7, 6, 8, 5, 9, 6]


def _host_side(host_devices, lm, tok):
    """The parameters as host tensors by path, and R, from one host device."""
    from learning_jax_sharding_amd import nn
    import learning_jax_sharding_amd as ljs
    host_devices(1)
    params, put = lm_params(lm, tok)
    R = uncached_logits(lm, params, tok, put, F32)
    return ljs.tree_map(lambda a: a.to_torch().numpy(), nn.unbox(params)), R


def _on_gpu(host_params):
    import learning_jax_sharding_amd as ljs
    put = lambda a: ljs.device_put(np.asarray(a))   # noqa: E731
    return ljs.tree_map(put, host_params), put


@pytest.mark.parametrize("B", [8, 2])
def test_cached_decode_rule_on_gpu(host_devices, gpu_devices, monkeypatch, B):
    from learning_jax_sharding_amd.ops import hip
    plens = PLENS8[:B]
    tok = tokens(B=B)
    host_params, R = _host_side(host_devices, LM, tok)
    gpu_devices(1)
    params, put = _on_gpu(host_params)
    A = uncached_logits(LM, params, tok, put, BF16)
    with hip.launch_log() as log:
        rows, cache = teacher_forced(LM, params, tok, plens, STEPS, put, max_len=32)
    names = [r["name"] for r in log]
    assert any(n == "kv_append<rot,q>" for n in names) and any(n.startswith("attn_decode<G2>") for n in names), names
    assert "lens_add" in names, names
    assert cache.k[0].local_tensors()[0].is_cuda
    rule_check(f"gpu B{B}", rows, R, A, plens, STEPS)
    if B == 8:
        monkeypatch.setenv("LJS_FUSED_DECODE", "0")
        with hip.launch_log() as log:
            rows0, _ = teacher_forced(LM, params, tok, plens, STEPS, put, max_len=32)
        assert not [r for r in log if r["name"].startswith(("kv_append", "attn_decode", "lens_add"))], log
        rule_check(f"gpu B{B} LJS_FUSED_DECODE=0", rows0, R, A, plens, STEPS)
        diff = max((a - b).abs().max().item() for a, b in zip(rows, rows0))
        print(f"decode-figures fused vs LJS_FUSED_DECODE=0 max|diff|={diff:.4e}")


def test_captured_step_matches_eager(host_devices, gpu_devices):
    """The decode step under ``jit(capture=True)``: one eager warm-up, the captures, then replays only --
    the eager run's logits and cache bits, and ``lens`` at prompt + 8."""
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd.models import TransformerLM
    from learning_jax_sharding_amd.ops import hip
    tok = tokens(B=8)
    host_params, _ = _host_side(host_devices, LM, tok)
    gpu_devices(1)
    params, put = _on_gpu(host_params)
    eager_rows, eager_cache = teacher_forced(LM, params, tok, PLENS8, STEPS, put, max_len=32)
    model = TransformerLM(**LM)
    step = ljs.jit(lambda p, x, c: model.apply({"params": p}, x, cache=c), donate_argnums=(2,), capture=True)
    launches = []

    def counted(p, x, c):
        n0 = hip.lib().ljs_launch_count()
        out = step(p, x, c)
        launches.append(hip.lib().ljs_launch_count() - n0)
        return out

    rows, cache = teacher_forced(LM, params, tok, PLENS8, STEPS, put, max_len=32, step_fn=counted)
    torch.cuda.synchronize()
    print(f"decode-figures launches recorded per step call: {launches}")
    assert launches[0] > 0 and launches[-5:] == [0] * 5, launches       # replays record nothing
    assert cache.lens.to_torch().tolist() == [n + STEPS for n in PLENS8]
    for b in range(8):
        assert torch.equal(rows[b], eager_rows[b]), b
    for i in range(len(cache)):
        assert torch.equal(cache.k[i].to_torch(), eager_cache.k[i].to_torch()), i
        assert torch.equal(cache.v[i].to_torch(), eager_cache.v[i].to_torch()), i


def test_generate_captured_matches_eager(host_devices, gpu_devices):
    from learning_jax_sharding_amd.models import TransformerLM, generate
    tok = tokens(B=8)
    host_params, _ = _host_side(host_devices, LM, tok)
    gpu_devices(1)
    params, put = _on_gpu(host_params)
    model = TransformerLM(**LM)
    ids = put(tok[:, :9].numpy())
    eager = generate(model, params, ids, 8, prompt_lens=PLENS8, capture=False)
    captured = generate(model, params, ids, 8, prompt_lens=PLENS8, capture=True)
    assert eager.shape == (8, 8) and torch.equal(eager, captured), (eager, captured)
    with pytest.raises(ValueError, match="max_len"):
        generate(model, params, ids, 8, prompt_lens=PLENS8, max_len=16)


def test_two_virtual_devices_batch_sharded(host_devices, gpu_devices):
    lm = dict(LM, vocab_size=256)
    tok = tokens(B=8, vocab=256)
    host_params, R = _host_side(host_devices, lm, tok)
    gpu_devices(1)
    params1, put1 = _on_gpu(host_params)
    A = uncached_logits(lm, params1, tok, put1, BF16)
    gpu_devices(2)
    params, put, cache_sh, Ctx = mesh_setup((2, 1), lm, tok, host_params)
    with Ctx():
        rows, cache = teacher_forced(lm, params, tok, PLENS8, STEPS, put, cache_sharding=cache_sh)
    assert tuple(cache.k[0].tile.tile_shape) == (2, 1, 1, 1) and len(cache.k[0].local) == 2
    rule_check("gpu 2 virtual devices, batch sharded", rows, R, A, PLENS8, STEPS)
