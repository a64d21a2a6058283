"""Multi-token cached steps and greedy speculative decoding end to end on a real MI355X, on the decode tests' model.

* batch 2, T = 4 (``B T <= 16``: every projection on the skinny GEMM, whose rows do not depend on M): the logits and
  the cache rows of ONE ``extend=True`` call are the BITS of four single steps, with the bf16 and the MX-fp8 cache;
* batch 8, T = 4 (the tile launcher's GEMMs): ``max|C - R| <= 4 max|A - R| + 2^-23 max|R|`` (``R``: the float32 uncached
  logits from the host, ``A``: the bf16 uncached logits, ``C``: prefill + one extend call);
* ``generate(draft=...)`` gives plain ``generate``'s tokens: captured and eager, with the bf16 and the MX-fp8 cache, with
  the target as its own draft and with a one-layer draft of other weights, and on two virtual devices with the
  batch sharded;
* the launches of one round (``draft_tokens + 1`` model calls of a single step's launch count each, the target's
  attention an ``attn_extend<`` instance), replays recording nothing, and the default ``generate``'s launches against the
  ones recorded before (tests/golden/kvq_default_generate_launches.json)."""
import json
import os

import numpy as np
import pytest
import torch

from test_decode import LM, lm_params, mesh_setup, rule_check, tokens, uncached_logits
from test_kvq_e2e_gpu import _teacher_forced as teacher_forced_quant

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
PLENS8 = [5, 9, 7, 6, 8, 5, 9, 6]
T = 4
K = 3                          # draft tokens: the target checks K + 1 = 4 positions per call
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


def _extend_rows(lm, params, tok, plens, put, quant, max_len):
    """Cached logits of the real positions: the ragged prefill, then ONE extend call on T tokens; and the cache."""
    from learning_jax_sharding_amd.models import TransformerLM
    model = TransformerLM(**lm, dtype=BF16)
    B, P = tok.shape[0], max(plens)
    cache = model.init_cache(B, max_len, quant=quant)
    logits, cache = model.apply({"params": params}, put(tok[:, :P].numpy()), cache=cache, prompt_lens=plens)
    lp = logits.to_torch().double()
    x = torch.stack([tok[b, n:n + T] for b, n in enumerate(plens)])
    lg, cache = model.apply({"params": params}, put(x.numpy()), cache=cache, extend=True)
    assert cache.lens.to_torch().tolist() == [n + T for n in plens]
    lg = lg.to_torch().double()
    return [torch.cat([lp[b, :plens[b]], lg[b]]) for b in range(B)], cache


@pytest.mark.parametrize("quant", [None, "mxfp8"], ids=["bf16", "mxfp8"])
def test_extend_is_four_single_steps_bit_for_bit(host_devices, gpu_devices, quant):
    from learning_jax_sharding_amd.ops import hip
    plens = PLENS8[:2]
    tok = tokens(B=2)
    host_params, _ = _host_side(host_devices, LM, tok)
    gpu_devices(1)
    params, put = _on_gpu(host_params)
    steps, step_cache = teacher_forced_quant(LM, params, tok, plens, T, put, quant, 32)
    with hip.launch_log() as log:
        rows, cache = _extend_rows(LM, params, tok, plens, put, quant, 32)
    names = [r["name"] for r in log]
    tag = ",mx8" if quant else ""
    # (the log keeps the last 32 launches: the last layer's at least)
    assert f"attn_extend<G2,P4{tag}>" in names and f"kv_append<rot,q{tag}>" in names and "lens_add" in names, names
    assert not [n for n in names if n.startswith("attn_decode")], names
    for b in range(2):
        assert torch.equal(rows[b], steps[b]), (b, (rows[b] - steps[b]).abs().max())
    for a, w in zip(cache.k + cache.v + cache.k_scale + cache.v_scale,
                    step_cache.k + step_cache.v + step_cache.k_scale + step_cache.v_scale):
        assert torch.equal(a.to_torch(), w.to_torch())


def test_extend_rule_at_batch_8(host_devices, gpu_devices):
    tok = tokens(B=8)
    host_params, R = _host_side(host_devices, LM, tok)
    gpu_devices(1)
    params, put = _on_gpu(host_params)
    A = uncached_logits(LM, params, tok, put, BF16)
    rows, _ = _extend_rows(LM, params, tok, PLENS8, put, None, 32)
    rule_check("extend gpu B8 T4", rows, R, A, PLENS8, T)


def _draft(which, host_params, ids):
    """(the target's parameters on the GPU, (draft model, draft parameters))."""
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd.models import TransformerLM
    params, _ = _on_gpu(host_params)
    if which == "self":
        return params, (TransformerLM(**LM), params)
    dlm = dict(LM, layers=1)
    return params, (TransformerLM(**dlm), TransformerLM(**dlm).init(ljs.random.PRNGKey(7), ids)["params"])


@pytest.mark.parametrize("quant", [None, "mxfp8"], ids=["bf16", "mxfp8"])
@pytest.mark.parametrize("which", ["self", "other"])
def test_speculative_generate_is_plain_generate(host_devices, gpu_devices, which, quant):
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd.models import TransformerLM, generate
    plens, new = PLENS8[:2], 9
    tok = tokens(B=2)
    host_params, _ = _host_side(host_devices, LM, tok)
    gpu_devices(1)
    ids = ljs.device_put(tok[:, :9].numpy())
    params, draft = _draft(which, host_params, ids)
    model = TransformerLM(**LM)
    kw = dict(prompt_lens=plens, max_len=32, cache_quant=quant)
    plain = generate(model, params, ids, new, capture=True, **kw)
    for capture in (False, True):
        got, lens, mean = generate(model, params, ids, new, capture=capture, draft=draft, draft_tokens=K,
                                   return_lens=True, stop_poll=1, **kw)
        print(f"extend-figures speculative {which} {quant} capture={capture}: mean tokens per round {mean:.3f}")
        assert got.shape == (2, new) and lens.tolist() == [new, new]
        assert torch.equal(got, plain), (which, quant, capture, got, plain)
        if which == "self":
            assert mean == K + 1, mean


def test_speculative_generate_two_virtual_devices(host_devices, gpu_devices):
    from learning_jax_sharding_amd.models import TransformerLM, generate
    lm = dict(LM, vocab_size=256)
    plens, new = PLENS8[:4], 9
    tok = tokens(B=4, vocab=256)
    host_params, _ = _host_side(host_devices, lm, tok)
    gpu_devices(1)
    params1, put1 = _on_gpu(host_params)
    model = TransformerLM(**lm)
    plain = generate(model, params1, put1(tok[:, :9].numpy()), new, prompt_lens=plens, max_len=32)
    gpu_devices(2)
    params, put, cache_sh, Ctx = mesh_setup((2, 1), lm, tok, host_params)
    with Ctx():
        got = generate(model, params, put(tok[:, :9].numpy()), new, prompt_lens=plens, max_len=32,
                       cache_sharding=cache_sh, draft=(model, params), draft_tokens=K)
    assert torch.equal(got, plain), (got, plain)


def test_round_launches(host_devices, gpu_devices):
    """One round records ``K + 1`` model calls of a single step's launches each (the target as its own draft: the
    draft's extend call on two tokens, ``K - 1`` single steps, the target's extend call), a replay records nothing, and
    the capture's last launches hold the target's ``attn_extend<`` instances."""
    from learning_jax_sharding_amd.models import TransformerLM, generate
    from learning_jax_sharding_amd.ops import hip
    plens = PLENS8[:2]
    tok = tokens(B=2)
    host_params, _ = _host_side(host_devices, LM, tok)
    gpu_devices(1)
    params, put = _on_gpu(host_params)
    model = TransformerLM(**LM)
    ids = put(tok[:, :9].numpy())

    def total(new, **kw):
        with hip.launch_log() as log:
            generate(model, params, ids, new, prompt_lens=plens, max_len=32, **kw)
        torch.cuda.synchronize()
        return log.total, [r["name"] for r in log]

    step = total(3, capture=False)[0] - total(2, capture=False)[0]          # one plain decode step
    spec = dict(draft=(model, params), draft_tokens=K, stop_poll=1)
    rounds = {n: total(1 + n * (K + 1), capture=False, **spec)[0] for n in (1, 2)}
    per_round = rounds[2] - rounds[1]
    print(f"extend-figures launches: {step} per decode step, {per_round} per round of {K} draft tokens")
    assert step > 0 and per_round == (K + 1) * step, (step, per_round)
    two, names = total(1 + 2 * (K + 1), capture=True, **spec)               # an eager round and the capture
    three, _ = total(1 + 3 * (K + 1), capture=True, **spec)                 # ... and a replay
    assert two == rounds[2] and three == two, (rounds, two, three)
    # (the log keeps the last 32 launches: the end of the target's call)
    assert "attn_extend<G2,P4>" in names and not [n for n in names if n.startswith("attn_decode")], names


def test_default_generate_launches_unchanged(host_devices, gpu_devices):
    """``generate`` without a draft records the launches it recorded before ``extend=`` and ``draft=`` existed."""
    from learning_jax_sharding_amd.models import TransformerLM, generate
    from learning_jax_sharding_amd.ops import hip
    tok = tokens(B=8)
    host_params, _ = _host_side(host_devices, LM, tok)
    gpu_devices(1)
    params, put = _on_gpu(host_params)
    with hip.launch_log() as log:
        generate(TransformerLM(**LM), params, put(tok[:, :9].numpy()), 4, prompt_lens=PLENS8, capture=False)
    torch.cuda.synchronize()
    with open(GOLDEN) as f:
        gold = json.load(f)
    assert log.total == gold["total"] and [r["name"] for r in log] == gold["names"], (log.total, gold["total"])
