"""Cached decoding at ``dim_head=128`` end to end on a real MI355X, on the two-layer causal RoPE LM of
tests/test_attn128_e2e_gpu.py (dim 256, heads 2, kv_heads 1): with warnings turned into errors, a prefill and four cached
steps at batch 2 run ``kv_append128`` / ``attn_decode128`` in every layer and meet the end-to-end rules of
tests/test_decode.py (bf16 cache) and tests/test_kvq_e2e_gpu.py (MX-fp8 cache), both sides printed; captured ``generate``
equals eager ``generate``; one ``extend=True`` call on 4 positions has the bits of four single steps.
(``LJS_ATTN_D128=1`` only keeps the prompt's own uncached attention off the torch formulation and its warning.)"""
import warnings

import pytest
import torch

from test_decode import rule_check, teacher_forced, tokens, uncached_logits
from test_extend_e2e_gpu import T, _extend_rows, _host_side, _on_gpu
from test_kvq_e2e_gpu import _err, _teacher_forced as teacher_forced_quant

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
LM = dict(vocab_size=512, dim=256, layers=2, heads=2, kv_heads=1, dim_head=128, causal=True, rope_theta=10000.0,
          norm="rms", ff="swiglu")
PLENS, STEPS = [5, 9], 4


@pytest.fixture
def setup(host_devices, gpu_devices, monkeypatch):
    from learning_jax_sharding_amd.ops import kernels
    tok = tokens(B=2)
    host_params, R = _host_side(host_devices, LM, tok)
    gpu_devices(1)
    monkeypatch.setenv("LJS_ATTN_D128", "1")
    monkeypatch.setattr(kernels, "_WARNED_DECODE", set())
    monkeypatch.setattr(kernels, "_WARNED_DH", set())
    return (tok, R) + _on_gpu(host_params)


def _decode_names(log, tag=""):
    names = [r["name"] for r in log]
    assert names.count(f"kv_append128<rot,q{tag}>") >= LM["layers"] and names.count(f"attn_decode128<G2{tag}>") >= LM["layers"], names
    assert not [n for n in names if n.startswith(("kv_append<", "attn_decode<"))], names


def test_cached_steps_rule_bf16(setup):
    from learning_jax_sharding_amd.ops import hip
    tok, R, params, put = setup
    A = uncached_logits(LM, params, tok, put, BF16)
    with warnings.catch_warnings(), hip.launch_log() as log:
        warnings.simplefilter("error")
        rows, _ = teacher_forced(LM, params, tok, PLENS, STEPS, put, max_len=32)
    _decode_names(log)
    rule_check("decode128 gpu bf16", rows, R, A, PLENS, STEPS)


def test_cached_steps_rule_mxfp8(setup, monkeypatch):
    from learning_jax_sharding_amd.ops import hip
    tok, R, params, put = setup
    A = uncached_logits(LM, params, tok, put, BF16)
    with warnings.catch_warnings(), hip.launch_log() as log:
        warnings.simplefilter("error")
        c8, _ = teacher_forced_quant(LM, params, tok, PLENS, STEPS, put, "mxfp8", 32)
    _decode_names(log, ",mx8")
    monkeypatch.setenv("LJS_FUSED_DECODE", "0")
    c8ref, _ = teacher_forced_quant(LM, params, tok, PLENS, STEPS, put, "mxfp8", 32)
    monkeypatch.delenv("LJS_FUSED_DECODE")
    e8, e8ref = _err(c8, R, PLENS, STEPS), _err(c8ref, R, PLENS, STEPS)
    ea = max((A[b, :n + STEPS] - R[b, :n + STEPS]).abs().max().item() for b, n in enumerate(PLENS))
    rmax = max(R[b, :n + STEPS].abs().max().item() for b, n in enumerate(PLENS))
    allowed = e8ref + 4.0 * ea + 2.0 ** -23 * rmax
    print(f"decode128-figures mxfp8 max|C8-R|={e8:.4e} max|C8ref-R|={e8ref:.4e} max|A-R|={ea:.4e} allowed={allowed:.4e} "
          f"max|R|={rmax:.3f}")
    assert all(torch.isfinite(r).all() for r in c8) and e8 <= allowed, (e8, e8ref, ea, allowed)


@pytest.mark.parametrize("quant", [None, "mxfp8"], ids=["bf16", "mxfp8"])
def test_generate_captured_matches_eager(setup, quant):
    from learning_jax_sharding_amd.models import TransformerLM, generate
    tok, _, params, put = setup
    model, ids = TransformerLM(**LM), put(tok[:, :9].numpy())
    eager = generate(model, params, ids, 8, prompt_lens=PLENS, capture=False, cache_quant=quant)
    captured = generate(model, params, ids, 8, prompt_lens=PLENS, capture=True, cache_quant=quant)
    assert eager.shape == (2, 8) and torch.equal(eager, captured), (eager, captured)


@pytest.mark.parametrize("quant", [None, "mxfp8"], ids=["bf16", "mxfp8"])
def test_extend_is_four_single_steps_bit_for_bit(setup, quant):
    from learning_jax_sharding_amd.ops import hip
    tok, _, params, put = setup
    steps, step_cache = teacher_forced_quant(LM, params, tok, PLENS, T, put, quant, 32)
    with hip.launch_log() as log:
        rows, cache = _extend_rows(LM, params, tok, PLENS, put, quant, 32)
    assert f"attn_extend128<G2,P4{',mx8' if quant else ''}>" in [r["name"] for r in log], log
    for b in range(2):
        assert torch.equal(rows[b], steps[b]), (b, (rows[b] - steps[b]).abs().max())
    for a, w in zip(cache.k + cache.v + cache.k_scale + cache.v_scale,
                    step_cache.k + step_cache.v + step_cache.k_scale + step_cache.v_scale):
        assert torch.equal(a.to_torch(), w.to_torch())
