"""``generate`` with a key, filters and stop tokens end to end on a real MI355X (the sampling step is
``sample_reference``'s torch launches there): captured against eager, two virtual devices with the batch sharded
against one, early stop under capture, and the default call's launches."""
import pytest
import torch

from test_decode import LM, mesh_setup, tokens
from test_decode_e2e_gpu import PLENS8, _host_side, _on_gpu

pytestmark = pytest.mark.gpu

SAMPLING = dict(temperature=0.9, top_k=40, top_p=0.9)


def _key(seed=11):
    import learning_jax_sharding_amd as ljs
    return ljs.random.PRNGKey(seed)


def _gpu_model(host_devices, gpu_devices, lm=LM, vocab=257):
    from learning_jax_sharding_amd.models import TransformerLM
    tok = tokens(B=8, vocab=vocab)
    host_params, _ = _host_side(host_devices, lm, tok)
    gpu_devices(1)
    params, put = _on_gpu(host_params)
    return TransformerLM(**lm), params, put(tok[:, :9].numpy()), tok, host_params


def _logged(fn):
    from learning_jax_sharding_amd.ops import hip
    with hip.launch_log() as log:
        out = fn()
    return out, log


def test_sampled_generate_captured_matches_eager(host_devices, gpu_devices):
    from learning_jax_sharding_amd.models import generate
    model, params, ids, _, _ = _gpu_model(host_devices, gpu_devices)
    gen = lambda n, capture, key=_key(): generate(model, params, ids, n, prompt_lens=PLENS8, capture=capture,  # noqa: E731
                                                  key=key, **SAMPLING)
    full = gen(8, False)
    assert full.shape == (8, 8) and full.dtype == torch.int64 and ((full >= 0) & (full < 257)).all()
    assert torch.equal(gen(3, False), full[:, :3]) and not torch.equal(full, gen(8, False, _key(12)))
    # captured: the same tokens, so a replayed step advances its random stream from the device's lens alone
    assert torch.equal(gen(8, True), full) and torch.equal(gen(4, True), full[:, :4])
    # no key, stop tokens alone: the lowest index of the maximum, captured as eager (bf16 logits do tie at the
    # maximum, where the default call's argmax names no rule, so the two are not compared)
    stop = [generate(model, params, ids, 8, prompt_lens=PLENS8, capture=c, eos_id=256, pad_id=0, stop_poll=0)
            for c in (False, True)]
    assert torch.equal(stop[0], stop[1])


def test_default_call_keeps_its_launches(host_devices, gpu_devices):
    """``key=None``, no eos: a step of ``generate`` records the launches of a teacher-forced decode step and no others,
    as before sampling existed."""
    from learning_jax_sharding_amd.models import generate
    from learning_jax_sharding_amd.ops import hip
    model, params, ids, tok, _ = _gpu_model(host_devices, gpu_devices)
    generate(model, params, ids, 2, prompt_lens=PLENS8, capture=False)      # one-time launches stay out of the counts
    _, log3 = _logged(lambda: generate(model, params, ids, 3, prompt_lens=PLENS8, capture=False))
    _, log2 = _logged(lambda: generate(model, params, ids, 2, prompt_lens=PLENS8, capture=False))
    cache = model.init_cache(8, 32)
    model.apply({"params": params}, ids, cache=cache, prompt_lens=PLENS8)
    n0 = hip.lib().ljs_launch_count()
    model.apply({"params": params}, ids[:, :1], cache=cache)
    step = hip.lib().ljs_launch_count() - n0
    assert step > 0 and log3.total - log2.total == step, (log3.total, log2.total, step)


def test_stop_tokens_under_capture(host_devices, gpu_devices):
    from learning_jax_sharding_amd.models import generate
    model, params, ids, _, _ = _gpu_model(host_devices, gpu_devices)
    key = _key()
    free = generate(model, params, ids, 8, prompt_lens=PLENS8, capture=True, key=key, **SAMPLING)
    eos = [int(free[0, 2]), int(free[1, 0])]
    pad = 256
    want, want_lens = free.clone(), []
    for b in range(8):
        hit = [s for s in range(8) if int(free[b, s]) in eos]
        n = hit[0] + 1 if hit else 8
        want[b, n:] = pad
        want_lens.append(n)
    for capture in (True, False):
        got, lens = generate(model, params, ids, 8, prompt_lens=PLENS8, capture=capture, key=key, eos_id=eos,
                             pad_id=pad, stop_poll=2, return_lens=True, **SAMPLING)
        assert got.shape == (8, 8) and torch.equal(got, want) and lens.tolist() == want_lens, capture
    # every sequence stops on its first token: the early exit pads the rest
    first = sorted(set(free[:, 0].tolist()))
    assert len(first) <= 8
    got, lens = generate(model, params, ids, 8, prompt_lens=PLENS8, capture=True, key=key, eos_id=first, pad_id=pad,
                         stop_poll=1, return_lens=True, **SAMPLING)
    assert got.shape == (8, 8) and torch.equal(got[:, 0], free[:, 0]) and (got[:, 1:] == pad).all()
    assert lens.tolist() == [1] * 8


def test_two_virtual_devices_batch_sharded(host_devices, gpu_devices):
    from learning_jax_sharding_amd.models import TransformerLM, generate
    # float32: the projections of 4 and of 8 rows may take different GEMM instances, whose bf16 logits could differ
    # in the last place and flip a close draw; in float32 the draws are the same unless a gap is ~1e-6
    lm = dict(LM, vocab_size=256)
    _, params1, ids1, tok, host_params = _gpu_model(host_devices, gpu_devices, lm, 256)
    lm = dict(lm, dtype=torch.float32)
    model = TransformerLM(**lm)
    kw = dict(prompt_lens=PLENS8, key=_key(), eos_id=[7, 9], pad_id=0, return_lens=True, **SAMPLING)
    want = generate(model, params1, ids1, 6, **kw)
    gpu_devices(2)
    params, put, cache_sh, Ctx = mesh_setup((2, 1), lm, tok, host_params)
    with Ctx():
        got = generate(TransformerLM(**lm), params, put(tok[:, :9].numpy()), 6, cache_sharding=cache_sh, **kw)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
