"""The cache descriptor (csrc/kernels/cache_common.h) at the three C entries that take it, on a real MI355X: a kind
that does not match the scale bases, or is neither bf16 nor MX-fp8, is refused with nothing launched; the good calls
of both kinds launch what they always did.  The smallest shape: one sequence, one head, one key tile, one position."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SCALE = 0.125
BF16, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
INVALID = 1             # hipErrorInvalidValue


def _hip():
    from learning_jax_sharding_amd.ops import hip
    return hip


@pytest.fixture(scope="module")
def ops():
    hip = _hip()
    cap = hip.decode_key_tile()
    z = lambda *s, dt=BF16: torch.zeros(*s, dtype=dt).cuda()   # noqa: E731
    t = dict(q=z(1, 1, 1, 64), k=z(1, 1, 1, 64), o=z(1, 1, 1, 64), lse=z(1, 1, 1, dt=F32), lens=z(1, dt=torch.int32),
             kc=z(1, cap, 1, 64), vc=z(1, cap, 1, 64), k8=z(1, cap, 1, 64, dt=U8), v8=z(1, cap, 1, 64, dt=U8),
             ks=z(1, cap, 1, 2, dt=U8), vs=z(1, cap, 1, 2, dt=U8))
    torch.cuda.synchronize()
    return t


def _entries(t):
    """name -> the descriptor-level call of each entry on the module's operands."""
    hip = _hip()
    return {"kv_append": lambda d: hip._kv_append_desc(d, t["k"], t["k"], t["lens"]),
            "attn_decode": lambda d: hip._attn_decode_desc(d, t["q"], t["o"], t["lse"], None, t["lens"], SCALE, 1),
            "attn_chunk": lambda d: hip._attn_chunk_desc(d, t["q"], t["o"], t["lse"], t["lens"], SCALE)}


def _refused(call, desc):
    hip = _hip()
    with hip.launch_log() as log:
        rc = call(desc)
    return rc == INVALID and log.total == 0 and not log


@pytest.mark.parametrize("entry", ["kv_append", "attn_decode", "attn_chunk"])
def test_kind_and_scales_must_agree(ops, entry):
    hip, t = _hip(), ops
    call = _entries(t)[entry]
    assert _refused(call, hip._cache_desc(hip.CACHE_MX8, t["k8"], t["v8"], None, t["vs"]))       # MX-fp8, no k scales
    assert _refused(call, hip._cache_desc(hip.CACHE_MX8, t["k8"], t["v8"], t["ks"], None))       # MX-fp8, no v scales
    assert _refused(call, hip._cache_desc(hip.CACHE_BF16, t["kc"], t["vc"], t["ks"], None))      # bf16 with a k scale
    assert _refused(call, hip._cache_desc(hip.CACHE_BF16, t["kc"], t["vc"], None, t["vs"]))      # bf16 with a v scale
    for kind in (-1, 2):                                                                          # no such kind
        assert _refused(call, hip._cache_desc(kind, t["kc"], t["vc"]))
        assert _refused(call, hip._cache_desc(kind, t["k8"], t["v8"], t["ks"], t["vs"]))
    torch.cuda.synchronize()


@pytest.mark.parametrize("entry,names", [("kv_append", ("kv_append<copy>", "kv_append<copy,mx8>")),
                                         ("attn_decode", ("attn_decode<G1>", "attn_decode<G1,mx8>")),
                                         ("attn_chunk", ("attn_chunk<R64>", "attn_chunk<R64,mx8>"))])
def test_good_calls_launch_what_they_did(ops, entry, names):
    hip, t = _hip(), ops
    call = _entries(t)[entry]
    for desc, name in zip((hip._cache_desc(hip.CACHE_BF16, t["kc"], t["vc"]),
                           hip._cache_desc(hip.CACHE_MX8, t["k8"], t["v8"], t["ks"], t["vs"])), names):
        with hip.launch_log() as log:
            assert call(desc) == 0
        assert [r["name"] for r in log] == [name], log
    torch.cuda.synchronize()
