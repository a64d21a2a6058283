"""The skinny GEMM under the cached decode of ``TransformerLM`` on a real MI355X (tests/test_decode.py's model
and rule, as tests/test_decode_e2e_gpu.py uses them):

* teacher-forced decode at batch 8 and batch 2: every decode step's dense layers are ``skinny<`` launches and
  none is a tile GEMM, the prefill's launches do not depend on the switch, and the model rule

      max|C - R| <= 4 max|A - R| + 2^-23 max|R|

  holds;
* ``LJS_SKINNY_GEMM=0``: the steps' launch names and logits are those recorded from the commit before this
  kernel existed (tests/golden/skinny_parent_decode.json / .npz: the same model, tokens and lengths), launch
  for launch and bit for bit (the prefill's launch names included), and the default run differs from it by no
  more than the rule allows.  The logits fixture ties this test to the bits of the tile GEMMs as they were
  when it was recorded: a later, legitimate change to those kernels (or to anything else in the step)
  needs the two files recorded again from the tree before that change;
* ``hip.linear`` under ``no_grad`` at 3 rows is one ``skinny<`` launch without a padded copy of anything; with
  grad enabled the same 8-row call is the tile GEMM it was."""
import json
import os

import numpy as np
import pytest
import torch

from test_decode import LM, STEPS, rule_check, teacher_forced, tokens, uncached_logits
from test_decode_e2e_gpu import PLENS8, _host_side, _on_gpu

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "skinny_parent_decode")
DENSE = ("gemm_", "skinny<")


def decode_run(params, put, tok, plens):
    """Teacher-forced cached decode with every step under its own launch log: (rows, [(launch count, names)
    per step], (launch count, names) of a prefill of the same prompts)."""
    from learning_jax_sharding_amd.models import TransformerLM
    from learning_jax_sharding_amd.ops import hip
    model = TransformerLM(**LM, dtype=BF16)
    steps = []

    def logged(p, x, c):
        with hip.launch_log() as log:
            out = model.apply({"params": p}, x, cache=c)
        steps.append((log.total, [r["name"] for r in log]))
        return out

    rows, _ = teacher_forced(LM, params, tok, plens, STEPS, put, max_len=32, step_fn=logged)
    cache = model.init_cache(tok.shape[0], 32)
    with hip.launch_log() as log:
        model.apply({"params": params}, put(tok[:, :max(plens)].numpy()), cache=cache, prompt_lens=plens)
    torch.cuda.synchronize()
    return rows, steps, (log.total, [r["name"] for r in log])


def _golden():
    with open(GOLDEN + ".json") as f:
        return json.load(f), np.load(GOLDEN + ".npz")


@pytest.mark.parametrize("B", [8, 2])
def test_decode_steps_run_on_the_skinny_gemm(host_devices, gpu_devices, monkeypatch, B):
    monkeypatch.delenv("LJS_SKINNY_GEMM", raising=False)
    plens = PLENS8[:B]
    tok = tokens(B=B)
    host_params, R = _host_side(host_devices, LM, tok)
    gpu_devices(1)
    params, put = _on_gpu(host_params)
    A = uncached_logits(LM, params, tok, put, BF16)
    rows, steps, prefill = decode_run(params, put, tok, plens)
    for total, names in steps:
        assert total == len(names), (total, names)           # (the log keeps the last 32 launches)
        assert sum(n.startswith("skinny<") for n in names) >= 5 * LM["layers"] + 1, names
        assert not [n for n in names if n.startswith("gemm_")], names
    assert steps[1:] == steps[:1] * (STEPS - 1), steps
    rule_check(f"skinny gpu B{B}", rows, R, A, plens, STEPS)

    monkeypatch.setenv("LJS_SKINNY_GEMM", "0")
    rows0, steps0, prefill0 = decode_run(params, put, tok, plens)
    rule_check(f"skinny gpu B{B} LJS_SKINNY_GEMM=0", rows0, R, A, plens, STEPS)
    # the prefill (72 / 18 rows) does not depend on the switch
    assert prefill == prefill0 and not [n for n in prefill[1] if n.startswith("skinny<")], (prefill, prefill0)
    assert any(n.startswith("gemm_") for n in prefill[1]), prefill
    # switched off: the parent's launches, and the parent's bits
    names, logits = _golden()
    assert prefill0[1] == names[f"B{B}"]["prefill"] and prefill0[0] == names[f"B{B}"]["prefill_total"], prefill0
    assert not [n for _, ns in steps0 for n in ns if n.startswith("skinny<")], steps0
    assert [ns for _, ns in steps0] == names[f"B{B}"]["steps"], (steps0, names[f"B{B}"]["steps"])
    assert [t for t, _ in steps0] == names[f"B{B}"]["totals"]
    want = torch.from_numpy(logits[f"B{B}"]).double()
    for b in range(B):
        assert torch.equal(rows0[b], want[b, :plens[b] + STEPS]), b
    # the default path against it: another equally valid evaluation order, within the rule
    real = [slice(0, n + STEPS) for n in plens]
    diff = max((rows[b] - rows0[b]).abs().max().item() for b in range(B))
    err_a = max((A[b, real[b]] - R[b, real[b]]).abs().max().item() for b in range(B))
    rmax = max(R[b, real[b]].abs().max().item() for b in range(B))
    allowed = 4.0 * err_a + 2.0 ** -23 * rmax
    print(f"skinny-figures B{B} default vs LJS_SKINNY_GEMM=0 max|diff|={diff:.4e} allowed={allowed:.4e}")
    assert diff <= allowed, (diff, allowed)
    # per dense layer of a step: the same number of launches, each a skinny one
    for (_, ns), (_, ns0) in zip(steps, steps0):
        if B == 8:
            assert [n.startswith(DENSE) for n in ns] == [n.startswith(DENSE) for n in ns0], (ns, ns0)
        else:   # (batch 2 left through the padded path, with copies the library does not record)
            assert sum(n.startswith("skinny<") for n in ns) == sum(n.startswith("gemm_") for n in ns0), (ns, ns0)


def _ints(shape, seed, dtype):
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, shape, generator=gen).to(dtype)


def test_hip_linear_small_rows(gpu_devices, monkeypatch):
    from learning_jax_sharding_amd.ops import hip
    monkeypatch.delenv("LJS_SKINNY_GEMM", raising=False)
    gpu_devices(1)
    dev = torch.device("cuda", 0)
    K, N = 128, 64
    w = _ints((K, N), 1, F32).to(dev)
    b = _ints((N,), 2, F32).to(dev)
    x8 = _ints((8, K), 3, BF16).to(dev)
    # small integers: the f32 sums are exact in any order, the bf16 output is their one rounding
    want = (x8.double() @ w.double() + b.double()).clamp_min(0.0).float().bfloat16().double()

    def no_copy(*a, **k):
        raise AssertionError("a padded copy was made")

    with torch.no_grad():
        hip.linear(x8, [w], b, BF16, True, BF16)                          # (the weight's shadow is made here)
        monkeypatch.setattr(torch.nn.functional, "pad", no_copy)
        monkeypatch.setattr(hip, "_linear_padded", no_copy)
        for M in (3, 1, 7, 8, 13, 16):
            x = torch.cat([x8, x8])[:M].contiguous()
            with hip.launch_log() as log:
                y = hip.linear(x, [w], b, BF16, True, BF16)[0]
            assert log.total == 1 and log[0]["name"].startswith("skinny<") and "bias,relu" in log[0]["name"], (M, log)
            assert y.shape == (M, N) and y.dtype == BF16
            assert torch.equal(y.double().cpu(), torch.cat([want, want])[:M].cpu()), M
        # an f32 activation: the usual rounding pass, then the same launch; a fused pair: one launch, two views
        w2 = w.flip(1).contiguous()
        hip.linear(x8[:3], [w, w2], None, BF16, False, F32)                # (the stacked shadow is made here)
        with hip.launch_log() as log:
            ys = hip.linear(x8[:3].float(), [w, w2], None, BF16, False, F32)
        # (the rounding pass of x is an elementwise kernel, which the launch log does not record)
        assert log.total == 1 and log[0]["name"].startswith("skinny<") and log[0]["blocks"] == 2 * N // 16, log
        plain = x8[:3].double() @ w.double()
        assert ys[0].dtype == F32 and torch.equal(ys[0].double().cpu(), plain.cpu())
        assert torch.equal(ys[1].double().cpu(), plain.flip(1).cpu())
        assert ys[0].data_ptr() + 4 * N == ys[1].data_ptr()
        # a residual: in the epilogue
        res = _ints((3, N), 4, BF16).to(dev)
        with hip.launch_log() as log:
            y = hip.linear(x8[:3], [w], None, BF16, False, BF16, residual=res)[0]
        assert log.total == 1 and log[0]["name"].endswith(",res>"), log
        assert torch.equal(y.double().cpu(), (plain.bfloat16().double() + res.double()).bfloat16().double().cpu())
        # above 16 rows, and with the switch off: the tile GEMM
        with hip.launch_log() as log:
            hip.linear(torch.cat([x8, x8, x8]), [w], b, BF16, True, BF16)
        assert log[-1]["name"].startswith("gemm_"), log
        monkeypatch.setenv("LJS_SKINNY_GEMM", "0")
        with hip.launch_log() as log:
            y0 = hip.linear(x8, [w], b, BF16, True, BF16)[0]
        off_name = log[-1]["name"]
        assert log.total == 1 and off_name.startswith("gemm_"), log
        assert torch.equal(y0.double().cpu(), want.cpu())
        monkeypatch.delenv("LJS_SKINNY_GEMM")
    # grad enabled: the same 8-row call is the parent's GEMM
    with torch.enable_grad():
        with hip.launch_log() as log:
            y = hip.linear(x8, [w], b, BF16, True, BF16)[0]
        assert log.total == 1 and log[0]["name"] == off_name, (log, off_name)
        assert torch.equal(y.detach().double().cpu(), want.cpu())
