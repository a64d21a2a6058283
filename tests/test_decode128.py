"""Head dim 128 in the cached-decoding entries, on the host: the descriptor carries the width without growing, the
width queries answer for 64 and 128, and the table of which operation exists at which width says no to chunk at 128.
Only host-callable entries of the library are reached."""
import ctypes

import pytest
import torch


@pytest.mark.parametrize("dim", [64, 128])
def test_descriptor_carries_the_width(dim):
    from learning_jax_sharding_amd.ops import hip
    kc = torch.zeros(2, 8, 3, dim, dtype=torch.bfloat16)
    d = hip._cache_desc(hip.CACHE_BF16, kc, kc)
    assert (d.kind, d.cap, d.Hkv, d.dim) == (hip.CACHE_BF16, 8, 3, dim)
    assert d.k == kc.data_ptr() and list(d.sk) == list(kc.stride()[:3]) and not d.ks
    # the width sits in the padding before the first pointer: the size and the offsets are the 64-only struct's
    assert ctypes.sizeof(hip._CacheDesc) == hip.lib().ljs_cache_desc_size() == 144 and hip._CacheDesc.k.offset == 16


def test_width_queries_and_table():
    from learning_jax_sharding_amd.ops import hip
    assert (hip.decode_key_tile(), hip.decode_key_tile(64), hip.decode_key_tile(128)) == (32, 32, 16)
    assert (hip.decode_part_floats(), hip.decode_part_floats(128)) == (72, 136)
    assert hip.decode_key_tile(96) == 0 and hip.decode_part_floats(96) == 0
    for op in ("append", "decode", "extend", "kv_append_q8", "attn_decode", "attn_extend_q8"):
        assert hip.cache_op_supported(op, 64) and hip.cache_op_supported(op, 128) and not hip.cache_op_supported(op, 96)
    for op in ("chunk", "attn_chunk", "attn_chunk_q8"):
        assert hip.cache_op_supported(op, 64) and not hip.cache_op_supported(op, 128)
