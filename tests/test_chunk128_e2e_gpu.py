"""tests/test_chunk_e2e_gpu.py's chunked prompt and ``generate(prefill_chunk=40)`` on tests/test_decode128_e2e_gpu.py's model (MI355X)."""
import warnings

import pytest
import torch

import test_chunk_e2e_gpu as E64
from learning_jax_sharding_amd.models import TransformerLM, generate
from learning_jax_sharding_amd.ops import hip, kernels
from test_decode import rule_check, tokens, uncached_logits
from test_decode128_e2e_gpu import LM
from test_kvq_e2e_gpu import _host_side, _on_gpu

pytestmark = pytest.mark.gpu
S, B = E64.S, E64.B


@pytest.fixture
def setup(host_devices, gpu_devices, monkeypatch):
    tok = tokens(B=B, S=S)
    host_params, R = _host_side(host_devices, LM, tok)
    gpu_devices(1)
    monkeypatch.setenv("LJS_ATTN_D128", "1")
    monkeypatch.setattr(kernels, "_WARNED_DECODE", set())
    monkeypatch.setattr(kernels, "_WARNED_DH", set())
    monkeypatch.setattr(E64, "LM", LM)              # (_chunked builds its model from its module's LM)
    return (tok, R) + _on_gpu(host_params)


def test_chunked_prompt_logits_rule(setup, monkeypatch):
    tok, R, params, put = setup
    A = uncached_logits(LM, params, tok, put, torch.bfloat16)
    runs = []
    for quant, tag in ((None, ""), ("mxfp8", ",mx8")):
        with warnings.catch_warnings(), hip.launch_log() as log:     # (the last 32 launches: the last layer's at least)
            warnings.simplefilter("error")
            runs.append(E64._chunked(params, tok, put, quant))
        names = [r["name"] for r in log]
        assert f"attn_chunk128<R64{tag}>" in names and f"kv_append128<rot,q{tag}>" in names, names
        assert not [n for n in names if n.startswith(("attn_fwd", "attn_decode", "attn_extend", "attn_chunk<"))], names
        assert runs[-1][1].lens.to_torch().tolist() == [S] * B
    rule_check("chunk128 gpu 40+40+16", list(runs[0][0]), R, A, [S] * B, 0)
    monkeypatch.setenv("LJS_FUSED_DECODE", "0")
    C8, C8ref = runs[1][0], E64._chunked(params, tok, put, "mxfp8")[0]
    monkeypatch.delenv("LJS_FUSED_DECODE")
    e8, e8ref, ea = ((x - R).abs().max().item() for x in (C8, C8ref, A))
    allowed = e8ref + 4.0 * ea + 2.0 ** -23 * R.abs().max().item()
    print(f"chunk128-figures max|C8-R|={e8:.4e} max|C8ref-R|={e8ref:.4e} max|A-R|={ea:.4e} allowed={allowed:.4e}")
    assert torch.isfinite(C8).all() and e8 <= allowed, (e8, e8ref, ea, allowed)


@pytest.mark.parametrize("quant", [None, "mxfp8"], ids=["bf16", "mxfp8"])
def test_generate_prefill_chunk(setup, quant):
    tok, _, params, put = setup
    model, ids = TransformerLM(**LM), put(tok.numpy())
    kw = dict(prompt_lens=[S, 50], max_len=128, cache_quant=quant, prefill_chunk=40)
    with hip.launch_log() as log:
        generate(model, params, ids, 1, capture=False, **kw)
    assert f"attn_chunk128<R64{',mx8' if quant else ''}>" in [r["name"] for r in log], log
    eager, captured = (generate(model, params, ids, 6, capture=c, **kw) for c in (False, True))
    assert eager.shape == (B, 6) and torch.equal(eager, captured), (eager, captured)
