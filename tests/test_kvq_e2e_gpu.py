"""Decoding with the MX-fp8 KV cache end to end on a real MI355X, on the small model of tests/test_decode_e2e_gpu.py.

Teacher-forced logits: ``R`` the float32 uncached logits (host), ``A`` the bf16 uncached logits (GPU), ``C8`` the bf16
model with the fp8 cache on the kernels, ``C8ref`` the same with ``LJS_FUSED_DECODE=0`` (the torch references, on the
same GPU).  The fp8 cache's own error is whatever ``C8ref`` has; the kernels may add to it what the decode tests
already allow a kernel over its torch formulation:

    max|C8 - R| <= max|C8ref - R| + 4 max|A - R| + 2^-23 max|R|

Both sides are printed.  Then ``generate(..., cache_quant="mxfp8")`` captured against eager, the launches of one
decode step (the unquantised step's count, every ``kv_append`` / ``attn_decode`` in its ``mx8`` instance), and the default
``generate``'s launch names against the ones recorded before this cache existed
(tests/golden/kvq_default_generate_launches.json)."""
import json
import os

import numpy as np
import pytest
import torch

from test_decode import LM, STEPS, lm_params, tokens, uncached_logits

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
PLENS8 = [5, 9, 7, 6, 8, 5, 9, 6]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kvq_default_generate_launches.json")


def _host_side(host_devices, lm, tok):
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


def _teacher_forced(lm, params, tok, plens, steps, put, quant, max_len, step_fn=None):
    """test_decode.teacher_forced with a ``quant``: cached logits of the real positions, and the cache."""
    from learning_jax_sharding_amd.models import TransformerLM
    model = TransformerLM(**lm, dtype=BF16)
    B, P = tok.shape[0], max(plens)
    cache = model.init_cache(B, max_len, quant=quant)
    logits, cache = model.apply({"params": params}, put(tok[:, :P].numpy()), cache=cache, prompt_lens=plens)
    lp = logits.to_torch().double()
    rows = [[lp[b, :plens[b]]] for b in range(B)]
    step_fn = step_fn or (lambda p, x, c: model.apply({"params": p}, x, cache=c))
    for s in range(steps):
        t = torch.stack([tok[b, plens[b] + s] for b in range(B)])[:, None]
        lg, cache = step_fn(params, put(t.numpy()), cache)
        lg = lg.to_torch().double()
        for b in range(B):
            rows[b].append(lg[b])
    assert cache.lens.to_torch().tolist() == [n + steps for n in plens]
    return [torch.cat(r) for r in rows], cache


def _err(rows, R, plens, steps):
    return max((rows[b] - R[b, :plens[b] + steps]).abs().max().item() for b in range(len(plens)))


def test_fp8_cache_logits_rule(host_devices, gpu_devices, monkeypatch):
    from learning_jax_sharding_amd.models import TransformerLM
    from learning_jax_sharding_amd.ops import hip
    tok = tokens(B=8)
    host_params, R = _host_side(host_devices, LM, tok)
    gpu_devices(1)
    params, put = _on_gpu(host_params)
    A = uncached_logits(LM, params, tok, put, BF16)
    with hip.launch_log() as log:          # (the log keeps the last 32 launches: the last decode step and more)
        c8, cache = _teacher_forced(LM, params, tok, PLENS8, STEPS, put, "mxfp8", 32)
    names = [r["name"] for r in log]
    assert names.count("kv_append<rot,q,mx8>") >= LM["layers"] and names.count("attn_decode<G2,mx8>") >= LM["layers"], names
    assert "lens_add" in names, names
    assert not [n for n in names if n.startswith(("kv_append", "attn_decode")) and "mx8" not in n], names
    assert cache.k[0].local_tensors()[0].is_cuda and cache.k[0].dtype == torch.uint8
    with hip.launch_log() as log:          # a prefill: one append launch per layer, the copy instance (k is rotated)
        TransformerLM(**LM).apply({"params": params}, put(tok[:, :9].numpy()), cache=cache, prompt_lens=PLENS8)
    pre = [r["name"] for r in log if r["name"].startswith(("kv_append", "attn_decode"))]
    assert pre and set(pre) == {"kv_append<copy,mx8>"}, [r["name"] for r in log]
    monkeypatch.setenv("LJS_FUSED_DECODE", "0")
    with hip.launch_log() as log:
        c8ref, _ = _teacher_forced(LM, params, tok, PLENS8, STEPS, put, "mxfp8", 32)
    assert not [r for r in log if r["name"].startswith(("kv_append", "attn_decode", "lens_add"))], log
    monkeypatch.delenv("LJS_FUSED_DECODE")
    e8, e8ref = _err(c8, R, PLENS8, STEPS), _err(c8ref, R, PLENS8, STEPS)
    ea = max((A[b, :n + STEPS] - R[b, :n + STEPS]).abs().max().item() for b, n in enumerate(PLENS8))
    rmax = max(R[b, :n + STEPS].abs().max().item() for b, n in enumerate(PLENS8))
    allowed = e8ref + 4.0 * ea + 2.0 ** -23 * rmax
    print(f"kvq-figures max|C8-R|={e8:.4e} max|C8ref-R|={e8ref:.4e} max|A-R|={ea:.4e} allowed={allowed:.4e} "
          f"max|R|={rmax:.3f} max|C8ref-R|/max|A-R|={e8ref / ea:.3f}")
    assert all(torch.isfinite(r).all() for r in c8)
    assert e8 <= allowed, (e8, e8ref, ea, allowed)


def test_generate_captured_matches_eager(host_devices, gpu_devices):
    from learning_jax_sharding_amd.models import TransformerLM, generate
    tok = tokens(B=8)
    host_params, _ = _host_side(host_devices, LM, tok)
    gpu_devices(1)
    params, put = _on_gpu(host_params)
    model = TransformerLM(**LM)
    ids = put(tok[:, :9].numpy())
    eager = generate(model, params, ids, 8, prompt_lens=PLENS8, capture=False, cache_quant="mxfp8")
    captured = generate(model, params, ids, 8, prompt_lens=PLENS8, capture=True, cache_quant="mxfp8")
    assert eager.shape == (8, 8) and torch.equal(eager, captured), (eager, captured)
    plain = generate(model, params, ids, 8, prompt_lens=PLENS8, capture=True)
    assert torch.equal(eager[:, 0], plain[:, 0])          # the prefill attends to unquantised keys


def test_captured_step_launches(host_devices, gpu_devices):
    """The launches one decode step records while it is captured: as many with the fp8 cache as without, the
    append and the decode of every layer in their mx8 instances and every other name unchanged."""
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd.models import TransformerLM
    from learning_jax_sharding_amd.ops import hip
    tok = tokens(B=8)
    host_params, _ = _host_side(host_devices, LM, tok)
    gpu_devices(1)
    params, put = _on_gpu(host_params)
    model = TransformerLM(**LM)
    logs = {}
    for quant in (None, "mxfp8"):
        step = ljs.jit(lambda p, x, c: model.apply({"params": p}, x, cache=c), donate_argnums=(2,), capture=True)
        per_call = []

        def logged(p, x, c):
            with hip.launch_log() as log:
                out = step(p, x, c)
            assert log.total == len(log), (log.total, len(log))       # the log held every launch of the call
            per_call.append([r["name"] for r in log])
            return out

        _teacher_forced(LM, params, tok, PLENS8, STEPS, put, quant, 32, step_fn=logged)
        torch.cuda.synchronize()
        recorded = [c for c in per_call if c]
        assert recorded and per_call[-1] == [], per_call              # replays record nothing
        logs[quant] = recorded[-1]                                   # the capture's own launches
    plain, q8 = logs[None], logs["mxfp8"]
    print(f"kvq-figures launches of one captured step: {len(plain)} unquantised, {len(q8)} mxfp8")
    assert len(q8) == len(plain), (plain, q8)
    dec = [n for n in q8 if n.startswith(("kv_append", "attn_decode"))]
    assert len(dec) == 2 * LM["layers"] and all(n.endswith(",mx8>") for n in dec), q8
    assert [n.replace(",mx8>", ">") for n in q8] == plain, (plain, q8)


def test_default_generate_launch_names_unchanged(host_devices, gpu_devices):
    """``generate`` without ``cache_quant`` records the launches it recorded before the fp8 cache existed: their count,
    and the names of the last 32 (what the launch log keeps: the last decode step and the end of the one before)."""
    from learning_jax_sharding_amd.models import TransformerLM, generate
    from learning_jax_sharding_amd.ops import hip
    tok = tokens(B=8)
    host_params, _ = _host_side(host_devices, LM, tok)
    gpu_devices(1)
    params, put = _on_gpu(host_params)
    model = TransformerLM(**LM)
    ids = put(tok[:, :9].numpy())
    with hip.launch_log() as log:
        generate(model, params, ids, 4, prompt_lens=PLENS8, capture=False)
    torch.cuda.synchronize()
    with open(GOLDEN) as f:
        gold = json.load(f)
    want, got = gold["names"], [r["name"] for r in log]
    assert log.total == gold["total"], (log.total, gold["total"])
    assert got == want, [(i, a, b) for i, (a, b) in enumerate(zip(got, want)) if a != b][:5] + [len(got), len(want)]
