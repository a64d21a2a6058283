"""MX-fp8 weights in every dense call (``ops.linear.weight_quant("mxfp8-all")``, ``generate(..., weight_quant="mxfp8-all")``)
end to end on a real MI355X, on tests/test_skinny_mx_e2e_gpu.py's model.  Teacher-forced logits of the prompt
positions: ``R`` float32 uncached (host), ``A`` bf16 uncached, ``Cq`` the prefill on the ``gemm_w8`` kernel, ``Cq_ref`` the same
under ``LJS_GEMM_W8=0`` (the torch reference on the same shadows), held to the project's bound for quantised paths, both
sides printed:

    max|Cq - R| <= max|Cq_ref - R| + 4 max|A - R| + 2^-23 max|R|"""
import numpy as np
import pytest
import torch

from test_decode import uncached_logits
from test_kvq_e2e_gpu import PLENS8, _err, _teacher_forced
from test_skinny_mx_e2e_gpu import BF16, LM, _setup

pytestmark = pytest.mark.gpu

GEMMS = ("gemm_lean<", "gemm_dma<", "gemm_bf16<")


def _prefill(params, put, tok, mode):
    """The cached prefill under ``weight_quant(mode)``: (prompt-position logits per sequence, launch count, kept names)."""
    from learning_jax_sharding_amd.ops import hip, linear
    with hip.launch_log() as log, linear.weight_quant(mode), torch.no_grad():
        rows, _ = _teacher_forced(LM, params, tok, PLENS8, 0, put, None, 32)
    torch.cuda.synchronize()
    return rows, log.total, [r["name"] for r in log]


def test_prefill_logits_rule_and_launches(host_devices, gpu_devices, monkeypatch):
    monkeypatch.delenv("LJS_GEMM_W8", raising=False)
    tok, params, put, R = _setup(host_devices, gpu_devices)
    A = uncached_logits(LM, params, tok, put, BF16)
    _prefill(params, put, tok, "mxfp8-all")                  # (makes the weight shadows: the logs below hold no casts)
    _, n_plain, plain = _prefill(params, put, tok, None)
    cq, n_mx, mx = _prefill(params, put, tok, "mxfp8-all")
    # a gemm_w8< launch where the default run holds a tile GEMM (every projection is eligible at vocabulary 256),
    # nothing else moves; the log keeps the last 32 launches of a call
    assert n_mx == n_plain and len(mx) == len(plain), (n_plain, plain, n_mx, mx)
    assert [n for n in plain if n.startswith(GEMMS)] and not [n for n in mx if n.startswith(GEMMS)], (plain, mx)
    for a, b in zip(plain, mx):
        assert b.startswith("gemm_w8<R64,") if a.startswith(GEMMS) else a == b, (plain, mx)
    monkeypatch.setenv("LJS_GEMM_W8", "0")
    cq_ref, _, ref = _prefill(params, put, tok, "mxfp8-all")
    assert not [n for n in ref if n.startswith(GEMMS + ("gemm_w8<",))], ref
    monkeypatch.delenv("LJS_GEMM_W8")
    eq, eq_ref = _err(cq, R, PLENS8, 0), _err(cq_ref, R, PLENS8, 0)
    ea = max((A[b, :n] - R[b, :n]).abs().max().item() for b, n in enumerate(PLENS8))
    rmax = max(R[b, :n].abs().max().item() for b, n in enumerate(PLENS8))
    allowed = eq_ref + 4.0 * ea + 2.0 ** -23 * rmax
    print(f"gemm-w8-figures max|Cq-R|={eq:.4e} max|Cq_ref-R|={eq_ref:.4e} max|A-R|={ea:.4e} allowed={allowed:.4e} "
          f"max|R|={rmax:.3f}")
    assert all(torch.isfinite(r).all() for r in cq)
    assert eq <= allowed, (eq, eq_ref, ea, allowed)


def test_generate_under_the_mode(host_devices, gpu_devices, monkeypatch):
    from learning_jax_sharding_amd.models import TransformerLM, generate
    monkeypatch.delenv("LJS_GEMM_W8", raising=False)
    tok, params, put, _ = _setup(host_devices, gpu_devices)
    model = TransformerLM(**LM)
    ids = put(tok[:, :9].numpy())
    kw = dict(prompt_lens=PLENS8, weight_quant="mxfp8-all")
    eager = generate(model, params, ids, 8, capture=False, **kw)
    assert eager.shape == (8, 8) and torch.equal(eager, generate(model, params, ids, 8, capture=True, **kw))
    for more in (dict(cache_quant="mxfp8"), dict(prefill_chunk=4), dict(cache_quant="mxfp8", prefill_chunk=4)):
        both = [generate(model, params, ids, 8, capture=c, **kw, **more) for c in (False, True)]
        assert torch.equal(both[0], both[1]), more
    # the pinned behaviour of "mxfp8", next to the new mode: its prefill reads bf16 weights
    plain = generate(model, params, ids, 8, prompt_lens=PLENS8, capture=True)
    steps_only = generate(model, params, ids, 8, prompt_lens=PLENS8, capture=True, weight_quant="mxfp8")
    assert torch.equal(steps_only[:, 0], plain[:, 0])


def test_speculative_tokens_are_plain_greedy_under_the_mode(host_devices, gpu_devices, monkeypatch):
    """batch * (draft_tokens + 1) = 16: the prefill is the same call in both runs and the multi-position steps run
    skinny_mx<, whose rows do not depend on M.  Drafts: the target itself, and a perturbed copy (rejections)."""
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd.models import TransformerLM, generate
    monkeypatch.delenv("LJS_GEMM_W8", raising=False)
    tok, params, put, _ = _setup(host_devices, gpu_devices)
    model = TransformerLM(**LM)
    ids = put(tok[:4, :9].numpy())
    kw = dict(prompt_lens=PLENS8[:4], weight_quant="mxfp8-all", capture=True)
    greedy = generate(model, params, ids, 8, **kw)
    rng = np.random.default_rng(0)
    noisy = ljs.tree_map(lambda a: put(a.to_torch().numpy() + 0.05 * rng.standard_normal(a.shape).astype(np.float32)),
                         params)
    for dparams in (params, noisy):
        assert torch.equal(generate(model, params, ids, 8, draft=(model, dparams), draft_tokens=3, **kw), greedy)
    with pytest.raises(ValueError, match="draft"):
        generate(model, params, ids, 8, draft=(model, params), prompt_lens=PLENS8[:4], weight_quant="mxfp8")
