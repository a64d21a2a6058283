"""Chunked prefill end to end on a real MI355X, on the decode tests' model: a 96-token prompt as 40 + 40 + 16 under the
decode tests' rule (and tests/test_kvq_e2e_gpu.py's with the MX-fp8 cache), and ``generate(prefill_chunk=40)``."""
import warnings

import pytest
import torch

from test_decode import LM, rule_check, tokens, uncached_logits
from test_kvq_e2e_gpu import _host_side, _on_gpu

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
S, CHUNKS, B = 96, (40, 40, 16), 2


def _chunked(params, tok, put, quant):
    """Logits of the prompt fed chunk by chunk into an empty cache, and the cache."""
    from learning_jax_sharding_amd.models import TransformerLM
    model = TransformerLM(**LM, dtype=BF16)
    cache = model.init_cache(B, 128, quant=quant)
    out, c0 = [], 0
    for n in CHUNKS:
        lg, cache = model.apply({"params": params}, put(tok[:, c0:c0 + n].numpy()), cache=cache, extend="chunk")
        out.append(lg.to_torch().double())
        c0 += n
    return torch.cat(out, 1), cache


def test_chunked_prompt_logits_rule(host_devices, gpu_devices, monkeypatch):
    from learning_jax_sharding_amd.ops import hip
    tok = tokens(B=B, S=S)
    host_params, R = _host_side(host_devices, LM, tok)
    gpu_devices(1)
    params, put = _on_gpu(host_params)
    A = uncached_logits(LM, params, tok, put, BF16)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with hip.launch_log() as log:       # (the log keeps the last 32 launches: the last layer's at least)
            C, cache = _chunked(params, tok, put, None)
        names = [r["name"] for r in log]
        assert "attn_chunk<R64>" in names and "kv_append<rot,q>" in names and "lens_add" in names, names
        assert not [n for n in names if n.startswith(("attn_fwd", "attn_decode", "attn_extend"))], names
        with hip.launch_log() as log:
            C8, cache8 = _chunked(params, tok, put, "mxfp8")
        names = [r["name"] for r in log]
        assert "attn_chunk<R64,mx8>" in names and "kv_append<rot,q,mx8>" in names, names
    assert cache.lens.to_torch().tolist() == [S] * B and cache8.lens.to_torch().tolist() == [S] * B
    rule_check("chunk gpu 40+40+16", list(C), R, A, [S] * B, 0)
    monkeypatch.setenv("LJS_FUSED_DECODE", "0")
    with hip.launch_log() as log:
        C8ref, _ = _chunked(params, tok, put, "mxfp8")
    assert not [r for r in log if r["name"].startswith(("kv_append", "attn_chunk", "lens_add"))], log
    monkeypatch.delenv("LJS_FUSED_DECODE")
    e8, e8ref, ea = ((x - R).abs().max().item() for x in (C8, C8ref, A))
    allowed = e8ref + 4.0 * ea + 2.0 ** -23 * R.abs().max().item()
    print(f"chunk-figures max|C8-R|={e8:.4e} max|C8ref-R|={e8ref:.4e} max|A-R|={ea:.4e} allowed={allowed:.4e}")
    assert torch.isfinite(C8).all() and e8 <= allowed, (e8, e8ref, ea, allowed)


@pytest.mark.parametrize("quant", [None, "mxfp8"], ids=["bf16", "mxfp8"])
def test_generate_prefill_chunk(host_devices, gpu_devices, monkeypatch, quant):
    from learning_jax_sharding_amd.models import TransformerLM, generate
    from learning_jax_sharding_amd.ops import hip
    plens, new = [S, 50], 6
    tok = tokens(B=B, S=S)
    host_params, _ = _host_side(host_devices, LM, tok)
    gpu_devices(1)
    params, put = _on_gpu(host_params)
    model, ids = TransformerLM(**LM), put(tok.numpy())
    caches, init = [], TransformerLM.init_cache
    monkeypatch.setattr(TransformerLM, "init_cache", lambda self, *a, **k: caches.append(init(self, *a, **k)) or caches[-1])
    kw = dict(prompt_lens=plens, max_len=128, cache_quant=quant, prefill_chunk=40)
    eager = generate(model, params, ids, new, capture=False, **kw)
    captured = generate(model, params, ids, new, capture=True, **kw)
    assert eager.shape == (B, new) and torch.equal(eager, captured), (eager, captured)
    # the last token is returned, not appended: new - 1 decode steps follow the prefill
    assert [c.lens.to_torch().tolist() for c in caches] == [[n + new - 1 for n in plens]] * 2
    with hip.launch_log() as log:
        first = generate(model, params, ids, 1, capture=False, **kw)
    names = [r["name"] for r in log]
    assert f"attn_chunk<R64{',mx8' if quant else ''}>" in names and not [n for n in names if n.startswith("attn_fwd")], names
    assert torch.equal(first, eager[:, :1])
