"""Decoding with MX-fp8 weights (``ops.linear.weight_quant``, ``generate(..., weight_quant="mxfp8")``) end to end on a real
MI355X, on the model of tests/test_decode.py in its vocabulary-256 form (at 257 the head runs on a copy padded to 264
columns, which has no MX shadow and keeps its ``skinny<`` launch).  Teacher-forced logits: ``R`` float32 uncached (host),
``A`` bf16 uncached, ``Cq`` the decode steps on the kernel, ``Cq_ref`` the same under ``LJS_SKINNY_MX=0`` (the torch reference
on the same shadows), held to the MX cache's form of bound, both sides printed:

    max|Cq - R| <= max|Cq_ref - R| + 4 max|A - R| + 2^-23 max|R|"""
import re

import pytest
import torch

from test_decode import LM as LM257, STEPS, tokens, uncached_logits
from test_kvq_e2e_gpu import PLENS8, _err, _host_side, _on_gpu, _teacher_forced

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
LM = dict(LM257, vocab_size=256)


def _bf16_names(names):
    """Names with ``skinny_mx<W,`` / ``skinny<W,`` as ``skinny<`` (the plans' units of K differ, so the wave counts may)."""
    return [re.sub(r"^skinny(_mx)?<\d+,", "skinny<", n) for n in names]


def _setup(host_devices, gpu_devices):
    tok = tokens(B=8, vocab=256)
    host_params, R = _host_side(host_devices, LM, tok)
    gpu_devices(1)
    params, put = _on_gpu(host_params)
    return tok, params, put, R


def _decode(params, put, tok, mode, step=None):
    """Teacher-forced cached decode, each step under ``weight_quant(mode)`` and its own launch log: (rows, [(launch count,
    names)]).  A call that also makes weight shadows launches more than the log keeps: the tests check the calls they read."""
    from learning_jax_sharding_amd.models import TransformerLM
    from learning_jax_sharding_amd.ops import hip, linear
    model = TransformerLM(**LM, dtype=BF16)
    step = step or (lambda p, x, c: model.apply({"params": p}, x, cache=c))
    calls = []

    def logged(p, x, c):
        with hip.launch_log() as log, linear.weight_quant(mode):
            out = step(p, x, c)
        calls.append((log.total, [r["name"] for r in log]))
        return out

    rows, _ = _teacher_forced(LM, params, tok, PLENS8, STEPS, put, None, 32, step_fn=logged)
    torch.cuda.synchronize()
    return rows, calls


def test_fp8_weight_logits_rule_and_step_launches(host_devices, gpu_devices, monkeypatch):
    monkeypatch.delenv("LJS_SKINNY_MX", raising=False)
    tok, params, put, R = _setup(host_devices, gpu_devices)
    A = uncached_logits(LM, params, tok, put, BF16)
    plain_rows, plain = _decode(params, put, tok, None)
    cq, mx = _decode(params, put, tok, "mxfp8")
    # the default step is untouched; under the mode every skinny< launch is a skinny_mx< one, nothing else moves
    assert all(t == len(ns) for t, ns in plain[1:] + mx[1:]), (plain, mx)
    plain, mx = [ns for _, ns in plain[1:]], [ns for _, ns in mx[1:]]
    assert plain[1:] == plain[:1] * (STEPS - 2) and mx[1:] == mx[:1] * (STEPS - 2), (plain, mx)
    assert sum(n.startswith("skinny<") for n in plain[0]) == 5 * LM["layers"] + 1, plain[0]     # (+ the head)
    assert not [n for n in plain[0] if n.startswith("skinny_mx<")], plain[0]
    assert not [n for n in mx[0] if n.startswith("skinny<")], mx[0]
    assert len(mx[0]) == len(plain[0]) and _bf16_names(mx[0]) == _bf16_names(plain[0]), (plain[0], mx[0])
    monkeypatch.setenv("LJS_SKINNY_MX", "0")
    cq_ref, ref = _decode(params, put, tok, "mxfp8")
    assert not [n for n in ref[1][1] if n.startswith(("skinny<", "skinny_mx<"))], ref[1]
    monkeypatch.delenv("LJS_SKINNY_MX")
    eq, eq_ref = _err(cq, R, PLENS8, STEPS), _err(cq_ref, R, PLENS8, STEPS)
    ea = max((A[b, :n + STEPS] - R[b, :n + STEPS]).abs().max().item() for b, n in enumerate(PLENS8))
    rmax = max(R[b, :n + STEPS].abs().max().item() for b, n in enumerate(PLENS8))
    allowed = eq_ref + 4.0 * ea + 2.0 ** -23 * rmax
    print(f"skinny-mx-figures max|Cq-R|={eq:.4e} max|Cq_ref-R|={eq_ref:.4e} max|A-R|={ea:.4e} allowed={allowed:.4e} "
          f"max|R|={rmax:.3f} max|Cq_ref-R|/max|A-R|={eq_ref / ea:.3f} max|C-R|={_err(plain_rows, R, PLENS8, STEPS):.4e}")
    assert all(torch.isfinite(r).all() for r in cq)
    assert eq <= allowed, (eq, eq_ref, ea, allowed)
    # the prefill (72 rows) read bf16 weights: its logits are the default run's
    assert all(torch.equal(cq[b][:n], plain_rows[b][:n]) for b, n in enumerate(PLENS8))


def test_captured_step_is_keyed_by_the_mode(host_devices, gpu_devices, monkeypatch):
    """ONE jitted step, captured without the mode and then called under it: it is traced and captured again, with as
    many launches, the skinny ones in their MX instance; replays record nothing and give the eager logits."""
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd.models import TransformerLM
    monkeypatch.delenv("LJS_SKINNY_MX", raising=False)
    tok, params, put, _ = _setup(host_devices, gpu_devices)
    model = TransformerLM(**LM, dtype=BF16)
    step = ljs.jit(lambda p, x, c: model.apply({"params": p}, x, cache=c), donate_argnums=(2,), capture=True)
    logs, rows = {}, {}
    for mode in (None, "mxfp8"):
        rows[mode], calls = _decode(params, put, tok, mode, step)
        # call 0 is the eager warm-up of a new signature, call 1 its capture; replays record nothing
        assert calls[1][0] == len(calls[1][1]) > 0 and calls[-1] == (0, []), calls
        logs[mode] = calls[1][1]
    print(f"skinny-mx-figures launches of one captured step: {len(logs[None])} default, {len(logs['mxfp8'])} mxfp8")
    assert [n for n in logs["mxfp8"] if n.startswith("skinny_mx<")] and not [n for n in logs["mxfp8"] if n.startswith("skinny<")]
    assert len(logs["mxfp8"]) == len(logs[None]) and _bf16_names(logs["mxfp8"]) == _bf16_names(logs[None]), logs
    eager, _ = _decode(params, put, tok, "mxfp8")
    assert all(torch.equal(a, b) for a, b in zip(rows["mxfp8"], eager))
    again, calls = _decode(params, put, tok, None, step)            # and back: the first capture, replayed
    assert all(torch.equal(a, b) for a, b in zip(rows[None], again))


def test_generate_captured_matches_eager(host_devices, gpu_devices, monkeypatch):
    from learning_jax_sharding_amd.models import TransformerLM, generate
    monkeypatch.delenv("LJS_SKINNY_MX", raising=False)
    tok, params, put, _ = _setup(host_devices, gpu_devices)
    model = TransformerLM(**LM)
    ids = put(tok[:, :9].numpy())
    kw = dict(prompt_lens=PLENS8, weight_quant="mxfp8")
    eager = generate(model, params, ids, 8, capture=False, **kw)
    captured = generate(model, params, ids, 8, capture=True, **kw)
    assert eager.shape == (8, 8) and torch.equal(eager, captured), (eager, captured)
    plain = generate(model, params, ids, 8, prompt_lens=PLENS8, capture=True)
    assert torch.equal(eager[:, 0], plain[:, 0])                    # the prefill reads bf16 weights
    both = [generate(model, params, ids, 8, capture=c, cache_quant="mxfp8", **kw) for c in (False, True)]
    assert torch.equal(both[0], both[1]) and torch.equal(both[0][:, 0], plain[:, 0])
    with pytest.raises(ValueError):
        generate(model, params, ids, 8, weight_quant="int4")
