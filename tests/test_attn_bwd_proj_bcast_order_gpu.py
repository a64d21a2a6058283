"""attn_bwd_proj's broadcast-row instance after its weight stream was reordered (all sixteen stages
issued before the K / V / Q / O pieces, a group's fragment reads ahead of its MFMAs): dq / dk / dv
bit-equal to the general instance on the same call (LJS_ATTN_BWD_PROJ_BCAST=0, whose code did not
change), at the tile counts where the new ring takes another path (run on a real MI355X: -m gpu).
No tolerance appears: the two instances run the same MFMA sequence per element.

The kernel takes 256 queries and keys, not causal, one K / V head per query head (attn_bwd_proj_plan
rejects everything else), so there is no ragged, causal or grouped-query shape to run here."""
import pytest
import torch

pytestmark = pytest.mark.gpu

dev = torch.device("cuda", 0)
B, H, S, D = 2, 3, 256, 64
# K-tiles of 32: M = 96 is one partial group (3 tiles); 512 = 16 tiles, exactly the stages issued before
# the loop (nothing is issued in it but past-the-end tiles); 544 = 17: the first tile that goes into a
# stage the loop has read, and a last group of one; 640: the workload's (20: a whole reissued group)
MS = [96, 512, 544, 640]


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from learning_jax_sharding_amd.ops import hip as H_
    H_.lib()
    return H_


@pytest.fixture
def forced(hip, monkeypatch):
    monkeypatch.delenv("LJS_ATTN_BWD_PROJ_BCAST", raising=False)
    hip.set_attention_bwd_fused(True)
    hip.set_attention_bwd_proj(True)
    yield hip
    hip.set_attention_bwd_fused(None)
    hip.set_attention_bwd_proj(None)


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16).to(dev)


def _row(M):
    """Mixed signs and magnitudes (2^-8 .. 2^8), one zero and one entry that is subnormal as bf16."""
    g = torch.Generator(device="cpu").manual_seed(41)
    mag = torch.exp2(torch.randint(-8, 9, (M,), generator=g).float())
    row = (torch.randn(M, generator=g) * mag).to(torch.bfloat16)
    row[3] = 0.0
    row[M - 2] = -(2.0 ** -130)
    assert row[M - 2].item() == -(2.0 ** -130) and (row < 0).any() and (row > 0).any()
    return row.to(dev)


def _nan_outs():
    return tuple(torch.full((B, S, H, D), float("nan"), dtype=torch.bfloat16, device=dev) for _ in range(3))


_CASES = {}


def _case(hip, monkeypatch, M):
    """Inputs and the general instance's result on the broadcast row, computed once and left unchanged."""
    if M not in _CASES:
        qkv = _rand(B, S, 3, H, D, seed=23)
        q, k, v = (qkv[:, :, i] for i in range(3))
        o, lse = hip.attn_fwd_lse(q, k, v, D ** -0.5)
        w = _rand(H * D, M, seed=24, scale=M ** -0.5)
        row = _row(M)
        monkeypatch.setenv("LJS_ATTN_BWD_PROJ_BCAST", "0")
        gen = hip.attn_bwd_proj_block(q, k, v, o, row, 0, w, lse, D ** -0.5, outs=_nan_outs())
        assert hip.last_launch()["name"] == "attn_bwd_proj" and hip.attn_bwd_proj_last_path() == 0
        monkeypatch.delenv("LJS_ATTN_BWD_PROJ_BCAST")
        torch.cuda.synchronize()
        assert not any(torch.isnan(t.float()).any().item() for t in gen)
        _CASES[M] = (q, k, v, o, lse, w, row, gen)
    return _CASES[M]


@pytest.mark.parametrize("M", MS)
def test_reordered_broadcast_phase_equals_the_general_instance(forced, monkeypatch, M):
    hip = forced
    q, k, v, o, lse, w, row, gen = _case(hip, monkeypatch, M)
    got = hip.attn_bwd_proj_block(q, k, v, o, row, 0, w, lse, D ** -0.5, outs=_nan_outs())
    rec = hip.last_launch()
    assert rec["name"] == "attn_bwd_proj" and rec["grid"] == (B * H, 1, 1) and rec["block"] == 512, rec
    assert hip.attn_bwd_proj_last_path() == 1
    torch.cuda.synchronize()
    for a, b, name in zip(got, gen, ("dq", "dk", "dv")):
        # bits, not values: -0 and +0 are told apart
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), (M, name, (a.float() - b.float()).abs().max().item())
