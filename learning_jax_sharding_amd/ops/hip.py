"""ctypes bindings of the gfx950 HIP kernel library + autograd wrappers.

The library (``_lib/libljs_kernels.so``, built by ``csrc/build.py``) exposes a plain C
ABI; every launcher takes the current torch HIP stream, so kernels interleave with torch
ops, RCCL collectives and HIP-graph capture.  There is no fallback: if the library is
missing on a GPU machine every op raises (``LJS_ALLOW_TORCH_FALLBACK=1`` is a debugging
escape hatch that routes to the torch reference implementations instead).
"""
from __future__ import annotations

import contextlib
import ctypes
import math
import os
import threading
from typing import Dict, List, Optional, Sequence

import torch

__all__ = ["lib", "available", "gemm", "bmm_nt", "linear", "attention", "cast", "sum_all", "softmax_lastdim",
           "adam", "rng_fill", "colsum", "supports_cast", "norm", "xent", "xent_stats", "embed",
           "embed_grad", "rope", "swiglu", "kv_append", "attn_decode", "kv_append_q8", "attn_decode_q8", "plan_decode",
           "lens_add", "attn_extend", "attn_extend_q8", "skinny",
           "skinny_plan", "skinny_supported", "set_skinny_waves"]

_HERE = os.path.dirname(os.path.abspath(__file__))
# LJS_KERNELS_LIB: an alternative build of the library (A/B timing of kernel variants)
_LIBPATH = os.environ.get("LJS_KERNELS_LIB") or os.path.join(os.path.dirname(_HERE), "_lib", "libljs_kernels.so")
_LIB = None
_LOCK = threading.Lock()

c_void_p, c_int, c_long, c_float, c_uint = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_uint
c_double = ctypes.c_double
_LP = ctypes.POINTER(ctypes.c_long)

_SIGS = {
    "ljs_pack_rows": [c_void_p, c_int, c_void_p, c_long, c_long, c_long, c_int, c_void_p, c_void_p],
    "ljs_gemm_group_end": [c_void_p],
    "ljs_gemm_bf16": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_long, c_long, c_long, c_long,
                      c_long, c_long, c_long, c_int, c_int, c_int, c_int, c_int, c_float, c_int, c_int, c_void_p,
                      ctypes.POINTER(c_int), c_void_p, c_long, c_long, c_void_p],
    "ljs_gemm_plan": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_long, c_long, c_long, c_long,
                      c_long, c_long, c_long, c_int, c_int, c_int, c_int, c_int, c_float, c_int, c_int, c_void_p,
                      ctypes.POINTER(c_int), c_void_p, c_long, c_long, c_int, ctypes.POINTER(c_int), ctypes.c_char_p,
                      c_int],
    "ljs_sum_partials": [c_void_p, c_int, c_void_p, c_int, c_void_p],
    "ljs_mse_colsum_ws_bytes": [c_int, c_int],
    "ljs_gemm_f32": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_long, c_long, c_long, c_long, c_long,
                     c_long, c_long, c_long, c_int, c_void_p],
    "ljs_attn_fwd": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, _LP, _LP, _LP, _LP,
                     c_float, c_int, c_int, c_void_p],
    "ljs_attn_set_trace": [c_void_p],
    "ljs_attn_set_trace_steps": [c_void_p],
    "ljs_qkv_attn_fwd": [c_void_p, c_long, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float,
                         c_void_p, c_void_p],
    "ljs_attn_fwd_acc": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, _LP, _LP, _LP,
                         _LP, c_float, c_int, c_int, c_void_p, _LP, c_int, c_void_p],
    "ljs_attn_bwd": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                     c_void_p, c_int, c_int, c_int, c_int, _LP, _LP, _LP, _LP, _LP, _LP, _LP, _LP, c_float, c_int,
                     c_int, c_void_p],
    "ljs_attn_bwd_proj": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_void_p, c_int, c_void_p,
                          c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, _LP, _LP, _LP, _LP, _LP, _LP, _LP,
                          c_float, c_int, c_void_p],
    "ljs_attn_fwd_gqa": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, _LP, _LP,
                         _LP, _LP, c_float, c_int, c_int, c_void_p],
    "ljs_attn_fwd_acc_gqa": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, _LP,
                             _LP, _LP, _LP, c_float, c_int, c_int, c_void_p, _LP, c_int, c_void_p],
    "ljs_attn_bwd_gqa": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                         c_void_p, c_int, c_int, c_int, c_int, c_int, _LP, _LP, _LP, _LP, _LP, _LP, _LP, _LP, c_float,
                         c_int, c_int, c_void_p],
    "ljs_gqa_reduce": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, _LP, _LP, _LP, _LP,
                       c_void_p],
    "ljs_gqa_set_max_blocks": [c_int],
    "ljs_kv_append": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                      _LP, _LP, _LP, _LP, _LP, _LP, c_void_p, c_void_p, c_void_p, c_long, c_void_p],
    "ljs_attn_decode": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_void_p, c_int, c_int,
                        c_int, c_int, _LP, _LP, _LP, _LP, c_float, c_int, c_void_p],
    "ljs_kv_append_q8": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                         c_int, c_int, c_int, _LP, _LP, _LP, _LP, _LP, _LP, _LP, _LP, c_void_p, c_void_p, c_void_p, c_long,
                         c_void_p],
    "ljs_attn_decode_q8": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_long,
                           c_void_p, c_int, c_int, c_int, c_int, _LP, _LP, _LP, _LP, _LP, _LP, c_float, c_int, c_void_p],
    "ljs_attn_extend": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_void_p, c_int, c_int,
                        c_int, c_int, c_int, _LP, _LP, _LP, _LP, c_float, c_void_p],
    "ljs_attn_extend_q8": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_long,
                           c_void_p, c_int, c_int, c_int, c_int, c_int, _LP, _LP, _LP, _LP, _LP, _LP, c_float, c_void_p],
    "ljs_extend_max_positions": [],
    "ljs_decode_plan": [c_int, c_int, c_int, c_int, ctypes.POINTER(c_int)],
    "ljs_decode_launch_plan": [c_int, c_int, c_int, ctypes.POINTER(c_int)],
    "ljs_decode_set_splits": [c_int, c_int],
    "ljs_skinny_set_waves": [c_int],
    "ljs_skinny_plan": [c_int, c_int, c_int, c_int, ctypes.POINTER(c_int)],
    "ljs_skinny_bf16": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_long, c_long, c_long,
                        c_long, c_int, c_int, c_int, c_int, c_void_p],
    "ljs_decode_key_tile": [],
    "ljs_decode_part_floats": [],
    "ljs_decode_max_group": [],
    "ljs_lens_add": [c_void_p, c_int, c_int, c_void_p],
    "ljs_attn_bwd_proj_enabled": [c_int, c_int],
    "ljs_attn_bwd_proj_last_path": [],
    "ljs_cast_f32_bf16": [c_void_p, c_void_p, c_long, c_void_p],
    "ljs_cast_bf16_f32": [c_void_p, c_void_p, c_long, c_void_p],
    "ljs_swap01_bf16": [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p],
    "ljs_transpose_bf16": [c_void_p, c_void_p, c_int, c_int, c_long, c_long, c_void_p],
    "ljs_sum_n": [ctypes.POINTER(c_void_p), c_int, c_int, c_long, c_void_p, c_void_p],
    "ljs_rows_sum_f32": [c_void_p, c_int, c_int, c_long, c_void_p, c_void_p],
    "ljs_cast_transpose_f32_bf16": [c_void_p, c_void_p, c_int, c_int, c_long, c_long, c_void_p],
    "ljs_sum_all": [c_void_p, c_int, c_long, c_void_p, c_int, c_void_p, c_void_p],
    "ljs_colsum": [c_void_p, c_int, c_int, c_int, c_long, c_void_p, c_int, c_void_p, c_void_p],
    "ljs_fill_row_bf16": [c_void_p, c_int, c_void_p, c_long, c_void_p],
    "ljs_relu_bwd_colsum": [c_void_p, c_void_p, c_int, c_int, c_long, c_long, c_void_p, c_void_p, c_void_p, c_void_p],
    "ljs_relu_bwd": [c_void_p, c_void_p, c_int, c_int, c_long, c_long, c_void_p, c_void_p],
    "ljs_bcast_scalar": [c_void_p, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p],
    "ljs_pad_box": [c_void_p, c_void_p, c_int, _LP, _LP, _LP, _LP,
                    c_int, c_void_p],
    "ljs_slab_reduce": [c_void_p, c_int, c_long, c_int, c_int, c_void_p, c_int, c_long, c_int, c_void_p, c_void_p,
                        c_void_p, c_int, c_float, c_int, c_void_p],
    "ljs_softmax_rows_f32": [c_void_p, c_void_p, c_long, c_int, c_void_p],
    "ljs_adam_f32": [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_long,
                     c_float, c_float, c_float, c_float, c_float, c_void_p],
    "ljs_adam_multi": [_LP, c_int, c_void_p, c_int, c_void_p, c_float, c_float, c_float, c_float, c_float,
                       c_void_p, c_void_p, c_long, c_void_p],
    "ljs_adam_multi_dyn": [_LP, c_int, c_void_p, c_int, c_void_p, c_float, c_float, c_float, c_float,
                           c_void_p, c_void_p, c_long, c_void_p],
    "ljs_grad_sumsq": [_LP, c_int, c_void_p, c_int, c_void_p],
    "ljs_grad_sumsq_ws_words": [],
    "ljs_grad_sumsq_slot_word": [],
    "ljs_grad_sumsq_slots": [],
    "ljs_step_hyper": [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_double, c_int,
                       c_double, c_double, c_double, c_double, c_double, c_void_p, c_void_p],
    "ljs_step_add": [c_void_p, c_int, c_void_p],
    "ljs_adam_set_rows": [c_int],
    "ljs_clock_probe": [c_void_p, c_void_p, c_uint, c_uint, c_void_p],
    "ljs_mse_loss": [c_void_p, c_void_p, c_int, c_long, c_float, c_void_p, c_void_p, c_void_p, c_void_p],
    "ljs_mse_colsum": [c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p,
                       c_void_p],
    "ljs_rng_fill": [c_void_p, c_int, c_int, _LP, _LP, _LP, c_uint, c_uint, c_int, c_float, c_float, c_float,
                     c_float, c_void_p],
    "ljs_dropout": [c_void_p, c_void_p, c_int, c_int, _LP, _LP, _LP, c_uint, c_uint, c_float, c_void_p],
    "ljs_norm_fwd": [c_void_p, c_int, c_long, c_void_p, c_void_p, c_void_p, c_int, c_long, c_void_p, c_void_p, c_int,
                     c_int, c_float, c_int, c_void_p],
    "ljs_norm_bwd": [c_void_p, c_int, c_long, c_void_p, c_int, c_long, c_void_p, c_void_p, c_void_p, c_void_p, c_long,
                     c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p],
    "ljs_norm_bwd_ws_bytes": [c_int, c_int],
    "ljs_xent_fwd": [c_void_p, c_int, c_long, c_void_p, c_int, c_long, c_void_p, c_void_p, c_void_p, c_void_p, c_long,
                     c_int, c_void_p],
    "ljs_xent_bwd": [c_void_p, c_int, c_long, c_void_p, c_int, c_long, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                     c_long, c_long, c_int, c_void_p],
    "ljs_xent_wave_max_v": [],
    "ljs_embed_fwd": [c_void_p, c_int, c_long, c_void_p, c_int, c_long, c_void_p, c_int, c_long, c_int, c_int, c_void_p],
    "ljs_embed_index": [c_void_p, c_int, c_long, c_long, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                        c_void_p],
    "ljs_embed_scan": [c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p],
    "ljs_embed_bwd": [c_void_p, c_int, c_long, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                      c_void_p],
    "ljs_embed_chunk": [],
    "ljs_embed_allpairs_max_tokens": [],
    "ljs_embed_work_cap": [c_long],
    "ljs_rope": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, _LP, _LP, _LP, _LP,
                 c_void_p, c_void_p, c_long, c_long, c_int, c_void_p],
    "ljs_rope_set_max_blocks": [c_int],
    "ljs_swiglu": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, _LP, _LP, _LP, c_void_p],
    "ljs_swiglu_bwd": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, _LP, _LP,
                       _LP, _LP, _LP, c_void_p],
    "ljs_swiglu_set_max_blocks": [c_int],
    "ljs_launch_count": [],
    "ljs_launch_get": [c_long, ctypes.c_char_p, c_int],
    "ljs_attn_set": [c_int, c_int],
    "ljs_attn_get": [c_int],
    "ljs_attn_plan": [c_int, c_int, c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(c_void_p), _LP, c_int, c_long,
                      c_int, c_int, ctypes.POINTER(c_int), ctypes.c_char_p, c_int],
}


def lib():
    global _LIB
    if _LIB is None:
        with _LOCK:
            if _LIB is None:
                if not os.path.exists(_LIBPATH):
                    raise RuntimeError(
                        f"HIP kernel library not found at {_LIBPATH}: build it with "
                        "`python -m learning_jax_sharding_amd.csrc.build` (or __graft_entry__.build())")
                L = ctypes.CDLL(_LIBPATH)
                for name, argt in _SIGS.items():
                    fn = getattr(L, name)
                    fn.argtypes = argt
                    fn.restype = c_int
                L.ljs_mse_colsum_ws_bytes.restype = c_long
                L.ljs_norm_bwd_ws_bytes.restype = c_long
                L.ljs_launch_count.restype = c_long
                for name in ("ljs_grad_sumsq_ws_words", "ljs_grad_sumsq_slot_word", "ljs_grad_sumsq_slots"):
                    getattr(L, name).restype = c_long
                _LIB = L
    return _LIB


def _launch_at(i: int) -> Optional[dict]:
    buf = ctypes.create_string_buffer(256)
    if lib().ljs_launch_get(i, buf, len(buf)) < 0:
        return None
    rec = {}
    for item in buf.value.decode().split(" "):
        k, v = item.split("=", 1)
        if k == "name":
            rec[k] = v
        elif k == "grid":
            rec[k] = tuple(int(t) for t in v.split(","))
        else:
            rec[k] = None if int(v) < 0 else int(v)   # -1: the field does not apply to this kernel
    rec["blocks"] = rec["grid"][0] * rec["grid"][1] * rec["grid"][2]
    return rec


def last_launch() -> dict:
    """The host-side record of the last GEMM / attention / MX-fp8 kernel the library launched:

    ``name`` (the kernel instance, e.g. ``gemm_lean<256,192,4,2,2>``, ``gemm_dma<128,128,2,2,4,kc,kc,bf16>``,
    ``gemm_bf16<64,64,kc,mn,f32>``, ``attn_fwd_res<8>``, ``attn_bwd_fused<dma=1,sw=1>``, ``qkv_attn_fwd``, ``rope<bf16,bf16>`` / ``rope<bf16,bf16,inv>``,
    ``gemm_mx_fp8<128,2,fix=1>``, ``gemm_mx8<256,160,4,bf16,2>``, ``quant_mx_rows``, ``quant_mx_cols<tiled>`` /
    ``quant_mx_cols<generic>``, ``quant_mx_both<bf16>`` / ``quant_mx_both<f32>``, ``bcast_scalar_mx`` / ``bcast_scalar_mx2``,
    ``grad_sumsq``, ``step_hyper``, ``adam_f32``, ``adam_multi<32>`` / ``adam_multi_dyn<32>`` (the launch's tile height), ``kv_append<rot,q>`` / ``kv_append<rot>`` / ``kv_append<copy>``,
    ``attn_decode<G4>``, ``kv_append<rot,q,mx8>``, ``attn_decode<G4,mx8>`` (an MX-fp8 cache), ``attn_extend<G4,P2>`` / ``attn_extend<G4,P2,mx8>`` (heads per group, positions per block), ``decode_merge``, ``lens_add``, ``skinny<8,bf16,bias,relu,res>`` (waves per block, output type and
    the epilogue parts present)),
    ``grid`` (x, y, z), ``blocks`` (their product), ``block`` (threads); for the bf16 and MX-fp8 GEMMs
    ``requested_tile`` / ``resolved_tile`` (the tile code passed in and the one the launcher turned
    it into), ``splitk`` (the launched split count; ``splitk1``: the second GEMM's in a grouped pair)
    and ``variant`` (the LDS-DMA / lean kernels' epilogue instance; the 4-wave MX-fp8 kernel's
    compile-time epilogue ``FIX``, None on the 8-wave tiles); for the attention forward
    ``acc_mode``.  Fields that do not apply are None.

    The record is made where the launch is issued, so under graph capture it is made when the
    launch is *recorded* into the graph, not when the graph is replayed.  Launches of every host
    thread (autograd's backward thread included) go into one ring of the last 32."""
    n = lib().ljs_launch_count()
    rec = _launch_at(n - 1) if n > 0 else None
    if rec is None:
        raise RuntimeError("no kernel launch recorded yet")
    return rec


class LaunchLog(list):
    """The records :func:`launch_log` collected; ``total`` counts the launches made inside it (only
    the last 32 of them are kept)."""
    total = 0


@contextlib.contextmanager
def launch_log():
    """Context manager yielding a list that, on exit, holds the records (see :func:`last_launch`) of
    the launches made inside it, oldest first.  Like the record itself it sees launches as they are
    issued: a graph replay adds nothing, the capture that recorded the graph does."""
    log = LaunchLog()
    start = lib().ljs_launch_count()
    try:
        yield log
    finally:
        end = lib().ljs_launch_count()
        log.total = end - start
        log.extend(r for r in (_launch_at(i) for i in range(max(start, end - 32), end)) if r is not None)


# the `which` of ljs_attn_set / ljs_attn_get: the rows of LJS_ATTN_SWITCHES (csrc/kernels/attention.hip)
_ATTN_SWITCHES = ("bwd_pair", "dkv32", "dq32", "vst", "cus", "fwd_res", "bwd_kv_dma", "bwd_fused", "bwd_proj")


def _attn_set(which: str, value, flag: bool = True):
    """One kernel-variant switch of attention.hip: None restores the library's default (as any
    negative number does), ``flag`` switches take True / False, the others a number."""
    lib().ljs_attn_set(_ATTN_SWITCHES.index(which), -1 if value is None else int(bool(value) if flag else value))


def set_attention_cus(n: Optional[int]):
    """Grid of the fused Q/K/V projection + attention forward: ``n`` blocks instead of one per CU
    (tests: many items per block on small shapes); None or <= 0 = the device's CU count."""
    _attn_set("cus", n, flag=False)


def set_attention_fwd_resident(waves: int):
    """Forward kernel for key lengths <= 256: 0 = tiled (K/V tiles through registers), 4 or 8 =
    K/V-resident (whole K/V of a head in LDS by one LDS-DMA burst; waves x 16 queries per block),
    -1 = the default (8, or 4 below 256 blocks)."""
    _attn_set("fwd_res", waves, flag=False)


def set_attention_bwd_kv_dma(enabled: Optional[bool]):
    """Fused short-key backward: K / V land in LDS by LDS-DMA in flight with the first query block
    (True) or through registers (False); None = automatic (LDS-DMA when a block sweeps at most
    128 queries).  Bit-identical either way."""
    _attn_set("bwd_kv_dma", enabled)


def set_attention_vst(enabled: Optional[bool]):
    """Attention output row tiles (forward O, backward dK / dV) stored through an LDS image as
    whole 128-byte rows with 16-byte stores (True, the default via None), or per lane as 8-byte
    pieces (False).  Bit-identical either way."""
    _attn_set("vst", enabled)


def set_attention_bwd_fused(enabled: Optional[bool]):
    """Select the attention backward for key lengths <= 256: the single-pass fused kernel
    (True), the split dQ + dK/dV kernels (False; always used above 256 keys), or None for the
    automatic choice by grid size (the default)."""
    _attn_set("bwd_fused", enabled)


def set_attention_bwd_proj(enabled: Optional[bool]):
    """The fused backward that forms its own dO from the out-projection's dY (``attn_bwd_proj``):
    whenever its shape gate holds (True), never (False), or None for the automatic choice: where the
    fused backward itself is chosen and there are at least 192 (batch, head) pairs."""
    _attn_set("bwd_proj", enabled)


def set_attention_dkv32(enabled: Optional[bool]):
    """Split attention backward with 128-key dK/dV blocks (4 waves x 32 keys): True / None (the
    default) or False (64-key blocks)."""
    _attn_set("dkv32", enabled)


def set_attention_dq32(enabled: Optional[bool]):
    """With 128-key dK/dV blocks: 128-query dQ blocks (True / None, the default) or 64 (False)."""
    _attn_set("dq32", enabled)


def set_attention_bwd_pair(enabled: Optional[bool]):
    """Split attention backward as ONE launch of dQ and dK/dV blocks (True, the default via
    None) or as two launches ordered by the dQ kernel's delta output (False)."""
    _attn_set("bwd_pair", enabled)


def available() -> bool:
    try:
        lib()
        return True
    except (RuntimeError, OSError):
        return False


def _stream(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


_DEBUG_SYNC = os.environ.get("LJS_DEBUG_SYNC", "0") == "1"


def _ck(rc: int, name: str):
    if rc != 0:
        raise RuntimeError(f"{name} failed with hipError {rc}")
    if _DEBUG_SYNC or os.environ.get("LJS_DEBUG_SYNC") == "1":
        from ..profiler import after_kernel
        after_kernel(name)


_WS = {}


def _workspace(dev: torch.device, name: str, nbytes: int) -> torch.Tensor:
    """Persistent zero-initialised per-device scratch for in-launch last-arriver reductions:
    its ticket words are re-armed by the kernels themselves, so no per-call memset.  (Keyed
    by device only: a HIP graph captures on a side stream, and a workspace first created
    inside a capture would replay its zero-fill every step.  The kernels using one
    workspace are never run concurrently on two streams.)"""
    key = (dev.index, name)
    t = _WS.get(key)
    if t is None or t.numel() * 4 < nbytes:
        t = torch.zeros((nbytes + 3) // 4, dtype=torch.float32, device=dev)
        _WS[key] = t
    return t


_COLSUM_WS_BYTES = 4 << 20  # = ljs_colsum_ws_floats() * 4


def _p(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _longs(vals) -> ctypes.Array:
    arr = (ctypes.c_long * len(vals))(*[int(v) for v in vals])
    return arr


# ============================================================================ GEMM
def _gemm_flags(relu, bias_dtype, accumulate, zero_c, slabs, res_dtype, res_mode) -> int:
    """ljs_gemm_bf16's flag word (gemm.hip GemmArgs).  32: output stores with sc1, always on (they
    drop the written lines from L2, so the output stream does not evict the operand panels that
    neighbouring blocks re-read)."""
    flags = (1 if relu else 0) | (2 if bias_dtype is not None else 0) | (4 if bias_dtype == torch.float32 else 0) | \
        (8 if accumulate else 0) | (16 if zero_c else 0) | 32 | (512 if slabs else 0) | \
        (8192 if (slabs and _SLAB_VST) else 0)
    if res_dtype is not None:
        assert res_dtype in (torch.bfloat16, torch.float32), res_dtype
        flags |= (64 if res_mode == "add" else 128) | (256 if res_dtype == torch.float32 else 0)
    return flags


def gemm(A: torch.Tensor, B: torch.Tensor, C: torch.Tensor, M: int, N: int, K: int, lda: int, ldb: int, ldc: int,
         a_kc: bool, b_kc: bool, batch: int = 1, sA: int = 0, sB: int = 0, sC: int = 0,
         bias: Optional[torch.Tensor] = None, sBias: int = 0, relu: bool = False, alpha: float = 1.0,
         accumulate: bool = False, splitk: int = 1, tile: Optional[int] = None, a_off: int = 0, b_off: int = 0,
         c_off: int = 0, zero_c: bool = False, psum: Optional[torch.Tensor] = None,
         res: Optional[torch.Tensor] = None, res_ld: int = 0, res_mode: str = "add", sR: int = 0,
         slabs: bool = False, b_list: Optional[Sequence[torch.Tensor]] = None) -> int:
    """Raw launcher.  A/B bf16; C bf16 or f32 (split-K/accumulate need f32 C; a split-K or slab
    call with a bias or a ReLU is rejected: they apply to the sum, which no split holds).

    ``lda``/``ldb`` may be 0 for an operand that repeats one row (a broadcast gradient).
    ``zero_c`` zeroes C inside the launch sequence (needed before split-K accumulation).
    ``psum`` (f32, >= :func:`psum_slots` floats): the LDS-DMA kernels with bf16 output also write
    per-(tile, wave) sums of the stored values there.  Returns the number of partials written
    (0 when the chosen kernel does not produce them).
    ``res`` (bf16 or f32, element [row][col] at ``row * res_ld + col``; ``res_ld`` 0 = one
    broadcast row; bf16 C only) is an epilogue operand: ``res_mode="add"`` adds it as a residual
    (``bf16(bf16(y) + bf16(res))``, bit-exact with the unfused add), ``"mask"`` keeps the outputs
    where ``res > 0`` (a ReLU backward fused into the dX GEMM).
    ``b_list`` (slab mode, batch <= 4): batch b's B operand is ``b_list[b]`` (separate tensors).
    ``slabs`` (f32 C, m/n-contiguous operands, an LDS-DMA tile): split s of batch b's K range
    writes its own slab ``C + (s * batch + b) * sC``; ``splitk`` must be :func:`slab_count`-consistent (the
    last split may run past K, where it reads zeros), so the split need not divide the K-tiles.
    """
    assert A.dtype == torch.bfloat16 and B.dtype == torch.bfloat16, (A.dtype, B.dtype)
    assert not slabs or C.dtype == torch.float32, "split-K slabs are f32"
    out_f32 = C.dtype == torch.float32
    assert res is None or not out_f32, (C.dtype, res.dtype)
    # a split's partial is no output: the kernels drop the bias and would apply the ReLU per partial
    assert not ((slabs or min(max(1, splitk), -(-K // 64)) > 1) and (relu or bias is not None)), \
        "split-K / slab GEMMs take no bias and no ReLU"
    if tile is None:
        tile = pick_tile(M, N, K, batch, a_kc, b_kc, out_f32, splitk, ldc, bias, res, sA, sB, sC, ldb)
    flags = _gemm_flags(relu, None if bias is None else bias.dtype, accumulate, zero_c, slabs,
                        None if res is None else res.dtype, res_mode)
    eA = A.element_size()
    cnt = c_int(0)
    b_arg = ctypes.c_void_p(B.data_ptr() + b_off * eA)
    if b_list is not None:
        # slab mode over a batch of separate B tensors (each laid out like B): pointers by value
        assert slabs and len(b_list) == batch <= 4 and all(t.dtype == torch.bfloat16 for t in b_list)
        flags |= 4096
        b_keep = (c_void_p * len(b_list))(*[t.data_ptr() + b_off * eA for t in b_list])
        b_arg = ctypes.cast(b_keep, c_void_p)
    rc = lib().ljs_gemm_bf16(ctypes.c_void_p(A.data_ptr() + a_off * eA), b_arg,
                             ctypes.c_void_p(C.data_ptr() + c_off * C.element_size()), _p(bias), M, N, K, lda, ldb,
                             ldc, sA, sB, sC, sBias, batch, int(a_kc), int(b_kc), int(out_f32), flags, alpha,
                             splitk, tile, _p(psum), ctypes.byref(cnt), _p(res), res_ld, sR, _stream(C))
    _ck(rc, "ljs_gemm_bf16")
    return cnt.value


_PLAN_FIELDS = ("err", "resolved_tile", "family", "BM", "BN", "WM", "WN", "NST", "a_kc", "b_kc", "out_f32", "variant",
                "splitk", "kt_per_split", "N", "batch", "grid_x", "grid_y", "block", "psum_count", "mfast")
_PLAN_FAMILIES = ("register-staged", "lds-dma", "lean", "slab")


def gemm_plan(M: int, N: int, K: int, lda: int, ldb: int, ldc: int, a_kc: bool, b_kc: bool, out_f32: bool,
              batch: int = 1, sA: int = 0, sB: int = 0, sC: int = 0, bias_dtype=None, relu: bool = False,
              alpha: float = 1.0, accumulate: bool = False, splitk: int = 1, tile: int = 128, zero_c: bool = False,
              psum: bool = False, res_dtype=None, res_ld: int = 0, res_mode: str = "add", sR: int = 0,
              slabs: bool = False, c_addr: int = 4096, res_addr: int = 4096, cus: int = 256) -> dict:
    """What :func:`gemm` would launch for these arguments on a device of ``cus`` compute units
    (``ljs_gemm_plan``: the launcher's own plan step; needs the library, not a GPU).  Tensors are
    given by what the plan reads of them: dtypes, and the addresses of C and ``res`` for their
    alignment.  Returns the fields of a launch record (``name``, ``grid``, ``blocks``, ``block``,
    ``resolved_tile``, ``splitk``, ``variant``) plus ``family``, the instance's ``BM`` ... ``NST``,
    ``kt_per_split``, the launched ``N`` and ``batch`` (a folded batch is one GEMM), ``psum_count``
    and ``mfast``; ``err`` is the launcher's error code (0: it would launch)."""
    flags = _gemm_flags(relu, bias_dtype, accumulate, zero_c, slabs, res_dtype, res_mode)
    out, cnt, name = (c_int * len(_PLAN_FIELDS))(), c_int(0), ctypes.create_string_buffer(64)
    fake = c_void_p(4096)   # operand addresses the plan never reads
    res = c_void_p(res_addr) if res_dtype is not None else None
    lib().ljs_gemm_plan(fake, fake, c_void_p(c_addr), fake if bias_dtype is not None else None, M, N, K, lda, ldb, ldc,
                        sA, sB, sC, 0, batch, int(a_kc), int(b_kc), int(out_f32), flags, alpha, splitk, tile,
                        fake if psum else None, ctypes.byref(cnt), res, res_ld, sR, cus, out, name, len(name))
    plan = dict(zip(_PLAN_FIELDS, out))
    plan.update(name=name.value.decode(), family=_PLAN_FAMILIES[plan["family"]], grid=(out[16], out[17], 1),
                blocks=out[16] * out[17], variant=None if out[11] < 0 else out[11])
    return plan


def gemm_group_begin():
    """Open a grouped launch: the plain f32 slab GEMMs (weight gradients) that :func:`gemm` is
    asked for until :func:`gemm_group_end` are recorded instead of launched."""
    fn = lib().ljs_gemm_group_begin
    fn.argtypes = []
    fn.restype = None
    fn()


def gemm_group_end(dev_tensor: torch.Tensor):
    """Launch what the open group recorded on ``dev_tensor``'s current stream: two GEMMs of one
    kernel instance as ONE grid (one block per work item of either; the same kernel body per
    item, so bit-identical to separate launches), anything else one by one."""
    rc = lib().ljs_gemm_group_end(_stream(dev_tensor))
    _ck(rc, "ljs_gemm_group_end")


def psum_slots(M: int, N: int, batch: int = 1) -> int:
    """Upper bound on the fused output-sum partials of one bf16 GEMM (128-row tiles, 8 waves)."""
    return -(-M // 128) * -(-N // 128) * batch * 8


# Fused output sums: a bf16 GEMM output registered here (weakly) carries the per-wave sums of
# its values computed in the GEMM epilogue, so a following whole-array sum (the loss y.sum())
# reduces a few thousand partials in one tiny kernel instead of re-reading the output.  The
# entry is used only while the output tensor is alive, unmodified (version counter) and
# summed whole (same storage, numel, contiguous).
_PSUM = {}


def _register_psum(y: torch.Tensor, partials: torch.Tensor, count: int) -> None:
    import weakref
    key = y.data_ptr()
    ref = weakref.ref(y, lambda _r, k=key: _PSUM.pop(k, None) if _PSUM.get(k, (None,))[0] is _r else None)
    _PSUM[key] = (ref, y._version, partials, count, y.numel())


def _psum_for(t: torch.Tensor):
    ent = _PSUM.get(t.data_ptr())
    if ent is None:
        return None
    ref, ver, partials, count, numel = ent
    y = ref()
    if y is None or count <= 0 or t.numel() != numel or not t.is_contiguous() or t._version != ver \
            or y.data_ptr() != t.data_ptr():
        return None
    return partials, count


# slab-mode GEMMs: the last item's f32 tile leaves through LDS as whole rows (kSlabVst; the GPU
# tests switch it off to check the per-lane form bit-exact)
_SLAB_VST = True


def pick_tile(M: int, N: int, K: int, batch: int, a_kc: bool, b_kc: bool, out_f32: bool, splitk: int = 1,
              ldc: int = 0, bias=None, res=None, sA: int = 0, sB: int = 0, sC: int = 0, ldb: int = 0) -> int:
    """Kernel/tile choice (measured on MI355X at the bench shapes, ``scripts/gemm_one.py``): the
    LDS-DMA kernels (codes 2562 = 256x192 8 waves, 2561 = 256x128 8 waves, 1602 = 128x160 4 waves,
    1282 = 128x128 4 waves x 2 blocks/CU, ...; the k-contiguous ones run the lean K-loop kernel)
    whenever K is a multiple of 64, else the register-staged 128/64 tiles."""
    tiles128 = -(-M // 128) * -(-N // 128) * batch * max(1, splitk)
    # 128x160 tiles when they (and not 128x128 tiles) fill whole rounds of 512 resident blocks
    if (K % 64 == 0 and a_kc and b_kc and not out_f32 and splitk <= 1 and N % 160 == 0
            and ldc % 8 == 0 and tiles128 % 512 and (-(-M // 128) * (N // 160) * batch) % 512 == 0):
        return 1602
    if K % 64 == 0 and tiles128 >= 96 and (out_f32 or (N % 8 == 0 and ldc % 8 == 0)):
        # 256x192 (8 waves of 64x96, 2 stages; a weight-major batch folded into one GEMM): fewer DMA
        # pieces and fragment reads per MFMA than 256x128, one stage less in flight (lean K-loop
        # kernel: QKV 33.5 vs 39.2 us isolated, B=64 step 0.2124 / 0.2159 vs 0.2250 / 0.2189 ms)
        if (a_kc and b_kc and not out_f32 and res is None and M >= 4096 and splitk <= 1
                and (N * batch) % 192 == 0 and (batch == 1 or (bias is None and sA == 0 and sB == N * ldb
                                                                and sC == N and ldc == N * batch))):
            return 2562
        # 256x128 for large k-contiguous bf16 GEMMs: beats 128x128 x 2/CU at the QKV projection (37.9
        # vs 40.4 us) and the FF up-projection (60.7 vs 65.2 us; scripts/gemm_tiles_out.py)
        if a_kc and b_kc and not out_f32 and M >= 4096 and N * batch >= 1024 and N % 128 == 0:
            return 2561
        if a_kc and b_kc and not out_f32 and tiles128 < 256 and splitk <= 1:
            # under one round of 128x128 blocks (the 2048-token QKV projection: 192 tiles): the
            # 8-wave, 3-stage tile (qkv3 10.3 -> 9.5 us; scripts/gemm_small.py)
            return 12883
        return 1282
    if K % 64 == 0 and a_kc and b_kc and (out_f32 or (N % 8 == 0 and ldc % 8 == 0)):
        # few 128x128 tiles (the 2048-token reference shape): the 64x64 LDS-DMA tile, 4 stages
        # (out-projection 7.8 -> 7.0 us, its dX 8.0 -> 6.3 us vs the register-staged 64x64 tile;
        # scripts/gemm_small.py)
        return 644
    return 128 if tiles128 >= 160 else 64


# ... the slab traffic's weight in the split count of a weight-gradient GEMM launched on its own
# (not paired): its slabs are then always read back by a separate slab_reduce (a data-parallel
# step) or a lone deferred combine, so they weigh more -- dW_o at 16384 tokens 16 splits instead
# of 24: fake-4 dp rehearsal 0.2147-0.2172 vs 0.2211-0.2224 ms x3
# (profiles/r5bm_dw_single_traffic_lines.txt); the pair's model weighs them 1
_DW_SINGLE_TRAFFIC_W = 4.0
_DW_TRAFFIC_W = 1.0


def slab_count(nkt: int, S: int) -> int:
    """Splits actually launched for ``S`` requested over ``nkt`` K-tiles (ceil-sized splits)."""
    kps = -(-nkt // max(1, S))
    return -(-nkt // kps)


def _cus() -> int:
    try:
        return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    except Exception:
        return 256


def _dw_single(K: int, N: int, T: int, traffic_w: Optional[float] = None):
    """(tile, K-chunks, slab mode) of a weight-gradient slab GEMM [K, N] = X^T dY over T tokens.

    T > 4096: 128x128 tiles (2 blocks per CU) in slab mode, the split count chosen by a cost
    model -- rounds of resident blocks x K-tiles per split, plus the slab reduction's extra f32
    traffic -- instead of a power of two dividing the K-tiles: the FF weight gradients (100
    tiles) ran 400 items on 512 block slots (78 %), now 5 x 52 K-tiles = 500 items; dW_o (20
    tiles) 16 x 16 -> 24 x 11.  At T <= 4096 the 8-wave 128x128 tile (one block per CU) in slab
    mode."""
    w = _DW_SINGLE_TRAFFIC_W if traffic_w is None else traffic_w
    if K % 64 or N % 64 or T % 64:
        return 1282, pick_splitk_dma(K, N, T, 1), False, None
    nkt, tiles = T // 64, -(-K // 128) * -(-N // 128)
    best, best_cost = 1, None
    if T > 4096:
        slots = 2 * _cus()
        for S in range(1, min(64, nkt) + 1):
            if slab_count(nkt, S) != S:
                continue
            kps = -(-nkt // S)
            # ~1.2 us per K-tile round of a full chip of 128x128 blocks, ~1 us per round of
            # prologue/epilogue, and the reduction reads each f32 slab once (~5 TB/s)
            rounds = -(-tiles * S // slots)
            cost = rounds * (kps * 1.2 + 1.0) + w * S * K * N * 4 / 5e6
            if best_cost is None or cost < best_cost - 1e-9:
                best, best_cost = S, cost
        return 1282, best, True, best_cost
    # T <= 4096: 8-wave 128x128, 4 stages, one block per CU, uneven slab splits (0.1033-0.1053 ms
    # vs 0.1071-0.1076 for the 64x64 tile with power-of-two batched slabs at B = 8)
    for S in range(1, min(32, nkt) + 1):
        if slab_count(nkt, S) != S:
            continue
        cost = -(-tiles * S // _cus()) * (-(-nkt // S) * 1.2 + 1.0) + w * S * K * N * 4 / 5e6
        if best_cost is None or cost < best_cost - 1e-9:
            best, best_cost = S, cost
    return 12884, best, True, best_cost


def pick_dw_slabs(K: int, N: int, T: int):
    """(tile, K-chunks, slab mode) of a weight-gradient slab GEMM (see :func:`_dw_single`, which
    also returns the cost model's estimate in us, or None where no model applies)."""
    return _dw_single(K, N, T)[:3]


_PAIR_PICKS: Dict[tuple, Optional[tuple]] = {}
# "S0,S1[,tile]": force the pair's split counts (tests)
_DW_PAIR = ""


def pick_dw_pair(K0: int, N0: int, K1: int, N1: int, T: int):
    """(tile, S0, S1) for two weight-gradient slab GEMMs [K, N] over the same T tokens launched
    as ONE grid (ops.linear._hold_dw), or None when no pair of split counts fits one round of
    resident blocks or the two separate launches' estimate (:func:`_dw_single`) is lower.

    The 128x128 tile at 2 blocks per CU; the pair's items all start together, so the grid takes
    about its LONGEST item (~1.2 us per K-tile + ~1 us prologue / epilogue) plus the slab traffic
    (written here, read back by the combine or the fused Adam, ~5 TB/s) -- minimised over split
    pairs with tiles0 * S0 + tiles1 * S1 <= resident slots.  At the step shapes (dW_o 20 tiles,
    dW_qkv 60): 6 + 6 splits, 480 items of 43 K-tiles at T = 16384: 52.1 us for the pair vs 59.7
    for the 24 + 8-split launches back to back, and half the slab bytes
    (profiles/r5ah_dw_pair_probe.txt).  The FF block's pair (two 100-tile GEMMs) would need
    items of 128 K-tiles for one round and stays separate (bf16 layer 0.6475 / 0.6503 ms paired vs
    0.6314 / 0.6333, profiles/r5an_layer_pair_lines.txt)."""
    tiles0, size0 = -(-K0 // 128) * -(-N0 // 128), K0 * N0
    tiles1, size1 = -(-K1 // 128) * -(-N1 // 128), K1 * N1
    key = (K0, N0, K1, N1, T, _cus())
    if key in _PAIR_PICKS:
        return _PAIR_PICKS[key]
    nkt = T // 64
    # T <= 4096: the 8-wave 128x128 tile at one block per CU, as for a single weight gradient there
    # (B = 8 pair at 3 + 3 splits: 12.66 us vs 14.49 for the 1282 pair at 6 + 6, and half the slabs;
    # at T = 16384 72.0 vs 53.8, profiles/r5au_dw_pair_8w_probe.txt)
    tile, slots = (12884, _cus()) if T <= 4096 else (1282, 2 * _cus())
    best, best_cost = None, None
    if _DW_PAIR:
        v = [int(t) for t in _DW_PAIR.split(",")]
        best = (v[2] if len(v) > 2 else tile, slab_count(nkt, v[0]), slab_count(nkt, v[1]))
    else:
        for s0 in range(1, min(64, nkt) + 1):
            if tiles0 * s0 > slots:
                break
            if slab_count(nkt, s0) != s0:
                continue
            for s1 in range(1, min(64, nkt) + 1):
                if tiles0 * s0 + tiles1 * s1 > slots:
                    break
                if slab_count(nkt, s1) != s1:
                    continue
                kps = max(-(-nkt // s0), -(-nkt // s1))
                cost = kps * 1.2 + 1.0 + _DW_TRAFFIC_W * (s0 * size0 + s1 * size1) * 4 / 5e6
                if best_cost is None or cost < best_cost - 1e-9:
                    best, best_cost = (tile, s0, s1), cost
        c0, c1 = _dw_single(K0, N0, T, _DW_TRAFFIC_W)[3], _dw_single(K1, N1, T, _DW_TRAFFIC_W)[3]
        if best is not None and c0 is not None and c1 is not None and c0 + c1 <= best_cost:
            best = None
    _PAIR_PICKS[key] = best
    return best


def pick_splitk_dma(M: int, N: int, K: int, batch: int) -> int:
    """Split of the reduction for the 128x128 LDS-DMA kernel (weight-grad GEMMs): a divisor of
    the K-tiles giving ~512 work items (2 resident blocks per CU on 256 CUs), >= 4 K-tiles each."""
    if K % 64:
        return 1
    nkt = K // 64
    tiles = -(-M // 128) * -(-N // 128) * batch
    if tiles >= 384:
        return 1
    best, score = 1, None
    for s in range(1, min(16, nkt // 4) + 1):
        if nkt % s:
            continue
        sc = abs(tiles * s - 512)
        if score is None or sc < score:
            best, score = s, sc
    return best


def _choose_splitk(M: int, N: int, K: int, batch: int) -> int:
    """Split the reduction when the output tiles cannot fill MI355X's 256 CUs (weight-grad GEMMs)."""
    tiles = -(-M // 64) * -(-N // 64) * batch
    if tiles >= 256:
        return 1
    s = max(1, min(16, 512 // max(1, tiles), K // 512))
    return s


def _bmm_raw(A, B, out_dtype, a_kc, b_kc, M, N, K, batch, lda, ldb, sA, sB):
    C = torch.empty((batch, M, N), dtype=out_dtype, device=A.device)
    gemm(A, B, C, M, N, K, lda, ldb, N, a_kc, b_kc, batch, sA, sB, M * N)
    return C


def _gemm_f32(A, B, C, M, N, K, a_rs, a_cs, b_rs, b_cs, c_rs, sA, sB, sC, batch):
    rc = lib().ljs_gemm_f32(_p(A), _p(B), _p(C), M, N, K, a_rs, a_cs, b_rs, b_cs, c_rs, sA, sB, sC, batch,
                            _stream(C))
    _ck(rc, "ljs_gemm_f32")


class _BmmNT(torch.autograd.Function):
    """C[b] = A[b] @ Bt[b]^T for A (B,M,K), Bt (B,N,K)."""

    @staticmethod
    def forward(ctx, A, Bt, out_dtype):
        ctx.save_for_backward(A, Bt)
        ctx.out_dtype = out_dtype
        return _bmm_nt_fwd(A, Bt, out_dtype)

    @staticmethod
    def backward(ctx, dC):
        A, Bt = ctx.saved_tensors
        dC = dC.contiguous()
        dA = dB = None
        if ctx.needs_input_grad[0]:
            dA = _bmm_nn(dC.to(A.dtype) if A.dtype != dC.dtype else dC, Bt, A.dtype)       # dC @ Bt
        if ctx.needs_input_grad[1]:
            dB = _bmm_tn(dC.to(Bt.dtype) if Bt.dtype != dC.dtype else dC, A, Bt.dtype)     # dC^T @ A
        return dA, dB, None


def _bmm_nt_fwd(A, Bt, out_dtype):
    Bn, M, K = A.shape
    N = Bt.shape[1]
    if A.dtype == torch.float32 and Bt.dtype == torch.float32:
        A = A.contiguous()
        Bt = Bt.contiguous()
        C = torch.empty((Bn, M, N), dtype=torch.float32, device=A.device)
        _gemm_f32(A, Bt, C, M, N, K, K, 1, 1, K, N, M * K, N * K, M * N, Bn)
        return C.to(out_dtype)
    A = A.to(torch.bfloat16).contiguous()
    Bt = Bt.to(torch.bfloat16).contiguous()
    if K % 8:
        # pad the contraction to the kernel's 16-byte granularity
        pad = 8 - K % 8
        A = torch.nn.functional.pad(A, (0, pad))
        Bt = torch.nn.functional.pad(Bt, (0, pad))
        K += pad
    od = out_dtype if out_dtype in (torch.bfloat16, torch.float32) else torch.float32
    C = _bmm_raw(A, Bt, od, True, True, M, N, K, Bn, K, K, M * K, N * K)
    return C.to(out_dtype)


def _bmm_nn(dC, Bt, out_dtype):
    """(B,M,N) @ (B,N,K) -> (B,M,K)."""
    Bn, M, N = dC.shape
    K = Bt.shape[2]
    if dC.dtype == torch.float32:
        out = torch.empty((Bn, M, K), dtype=torch.float32, device=dC.device)
        _gemm_f32(dC, Bt.contiguous(), out, M, K, N, N, 1, K, 1, K, M * N, N * K, M * K, Bn)
        return out.to(out_dtype)
    if N % 8 == 0 and K % 8 == 0:
        # B[k=n][n'=k] = Bt[n][k] is n'-contiguous: read in place through the transposing LDS read
        dC = dC.to(torch.bfloat16).contiguous()
        od = out_dtype if out_dtype in (torch.bfloat16, torch.float32) else torch.float32
        out = torch.empty((Bn, M, K), dtype=od, device=dC.device)
        gemm(dC, Bt.to(torch.bfloat16).contiguous(), out, M, K, N, N, K, K, True, False, Bn, M * N, N * K, M * K)
        return out.to(out_dtype)
    return _bmm_nt_fwd(dC, Bt.transpose(1, 2).contiguous(), out_dtype)


def _bmm_tn(dC, A, out_dtype):
    """(B,M,N)^T @ (B,M,K) -> (B,N,K)."""
    Bn, M, N = dC.shape
    K = A.shape[2]
    if dC.dtype == torch.float32:
        out = torch.empty((Bn, N, K), dtype=torch.float32, device=dC.device)
        _gemm_f32(dC, A.contiguous(), out, N, K, M, 1, N, K, 1, K, M * N, M * K, N * K, Bn)
        return out.to(out_dtype)
    if N % 8 == 0 and K % 8 == 0 and M % 8 == 0:
        out = torch.empty((Bn, N, K), dtype=torch.float32 if out_dtype == torch.float32 else torch.bfloat16,
                          device=dC.device)
        gemm(dC.to(torch.bfloat16).contiguous(), A.to(torch.bfloat16).contiguous(), out, N, K, M, N, K, K, False,
             False, Bn, M * N, M * K, N * K)
        return out.to(out_dtype)
    return _bmm_nt_fwd(dC.transpose(1, 2).contiguous(), A.transpose(1, 2).contiguous(), out_dtype)


def bmm_nt(A: torch.Tensor, Bt: torch.Tensor, out_dtype: torch.dtype) -> torch.Tensor:
    return _BmmNT.apply(A, Bt, out_dtype)


# ============================================================================ casts
def supports_cast(src: torch.dtype, dst: torch.dtype) -> bool:
    return (src, dst) in ((torch.float32, torch.bfloat16), (torch.bfloat16, torch.float32))


class _Cast(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, dtype):
        ctx.src = t.dtype
        return _cast_raw(t, dtype)

    @staticmethod
    def backward(ctx, g):
        return _cast_raw(g.contiguous(), ctx.src) if supports_cast(g.dtype, ctx.src) else g.to(ctx.src), None


def _cast_raw(t: torch.Tensor, dtype: torch.dtype, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``t`` in ``dtype`` by one HIP launch (into ``out``, a contiguous tensor of t's shape, when
    given: a persistent buffer - e.g. a weight's bf16 shadow - is refreshed in place)."""
    if out is not None and not (t.dtype != dtype and supports_cast(t.dtype, dtype) and t.is_contiguous()
                                and out.is_contiguous() and out.dtype == dtype and out.shape == t.shape):
        out.copy_(t)
        return out
    if t.dtype == dtype:
        return t
    if not supports_cast(t.dtype, dtype) or not t.is_contiguous():
        return t.to(dtype)
    if out is None:
        out = torch.empty(t.shape, dtype=dtype, device=t.device)
    n = t.numel()
    if n == 0:
        return out
    if t.dtype == torch.float32:
        rc = lib().ljs_cast_f32_bf16(_p(t), _p(out), n, _stream(t))
    else:
        rc = lib().ljs_cast_bf16_f32(_p(t), _p(out), n, _stream(t))
    _ck(rc, "cast")
    return out


def swap01_bf16(x: torch.Tensor) -> torch.Tensor:
    """bf16 [S][B][K] (contiguous) from a contiguous f32 / bf16 [B][S][K]: the seq-major copy of
    an activation, rounded in the same pass (one HIP launch)."""
    B, S, K = x.shape
    out = torch.empty((S, B, K), dtype=torch.bfloat16, device=x.device)
    rc = lib().ljs_swap01_bf16(_p(x), int(x.dtype == torch.bfloat16), _p(out), B, S, K, _stream(x))
    _ck(rc, "swap01_bf16")
    return out


def sum_n(ts: Sequence[torch.Tensor], out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Elementwise sum of same-shape dense f32 / bf16 tensors on one GPU (f32 accumulation) in one
    launch - the loopback reduction over virtual devices.  Falls back to torch adds otherwise."""
    t0 = ts[0]
    ok = (t0.is_cuda and t0.dtype in (torch.float32, torch.bfloat16) and 1 <= len(ts) <= 128
          and all(t.shape == t0.shape and t.dtype == t0.dtype and t.device == t0.device and is_dense(t)
                  and t.stride() == t0.stride() and t.data_ptr() % 16 == 0 for t in ts))
    if not ok:
        acc = None
        for t in ts:
            v = t.float()
            acc = v if acc is None else acc + v
        return acc.to(t0.dtype)
    if out is None:
        out = torch.empty_like(t0)
    arr = (c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    rc = lib().ljs_sum_n(arr, len(ts), int(t0.dtype == torch.bfloat16), t0.numel(), _p(out), _stream(t0))
    _ck(rc, "sum_n")
    return out


def rows_sum(t2d: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """f32 [C] = sum over the rows of a SHORT f32 [R][C] (e.g. per-row-tile partial column sums a
    GEMM epilogue wrote): one memory round trip (rows_sum_f32_kernel); torch on the CPU."""
    R, C = t2d.shape
    if not t2d.is_cuda:
        s = t2d.float().sum(0)
        return s if out is None else out.copy_(s)
    assert t2d.dtype == torch.float32 and t2d.stride(1) == 1
    if out is None:
        out = torch.empty((C,), dtype=torch.float32, device=t2d.device)
    rc = lib().ljs_rows_sum_f32(_p(t2d), R, C, t2d.stride(0), _p(out), _stream(t2d))
    _ck(rc, "rows_sum_f32")
    return out


def sum_ptrs(ptrs: Sequence[int], out: torch.Tensor) -> torch.Tensor:
    """out (dense f32 / bf16) = sum of ``len(ptrs)`` <= 128 dense arrays of out's dtype and element
    count at the given device addresses (16-byte aligned) - e.g. every device's split-K weight
    gradient slabs, summed in one pass (parallel/weight_gather.py)."""
    assert 1 <= len(ptrs) <= 128 and out.is_cuda and is_dense(out) and all(p % 16 == 0 for p in ptrs)
    arr = (c_void_p * len(ptrs))(*ptrs)
    rc = lib().ljs_sum_n(arr, len(ptrs), int(out.dtype == torch.bfloat16), out.numel(), _p(out), _stream(out))
    _ck(rc, "sum_n")
    return out


def transpose_bf16(t: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[C][R] bf16 transpose of a bf16 [R][C] matrix (unit column stride), one HIP launch."""
    R, C = t.shape
    assert t.dtype == torch.bfloat16 and t.stride(1) == 1
    if out is None:
        out = torch.empty((C, R), dtype=torch.bfloat16, device=t.device)
    rc = lib().ljs_transpose_bf16(_p(t), _p(out), R, C, t.stride(0), out.stride(0), _stream(t))
    _ck(rc, "transpose_bf16")
    return out


def cast_into(src: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
    """dst[...] = src converted to dst.dtype (f32 <-> bf16 on the HIP kernel; both contiguous)."""
    assert src.numel() == dst.numel() and dst.is_contiguous(), (src.shape, dst.shape)
    if src.dtype == dst.dtype:
        dst.copy_(src)
        return dst
    if not supports_cast(src.dtype, dst.dtype) or not src.is_contiguous() or not dst.is_cuda:
        dst.copy_(src.reshape(dst.shape))
        return dst
    n = src.numel()
    if n:
        fn = lib().ljs_cast_f32_bf16 if src.dtype == torch.float32 else lib().ljs_cast_bf16_f32
        _ck(fn(_p(src), _p(dst), n, _stream(dst)), "cast")
    return dst


def cast(t: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    if t.requires_grad and torch.is_grad_enabled():
        return _Cast.apply(t, dtype)
    return _cast_raw(t, dtype)


def cast_transpose_bf16(w: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bf16 W^T ([N][K]) from an f32 [K][N] matrix (row stride w.stride(0))."""
    K, N = w.shape
    assert w.dtype == torch.float32 and w.stride(1) == 1
    if out is None:
        out = torch.empty((N, K), dtype=torch.bfloat16, device=w.device)
    rc = lib().ljs_cast_transpose_f32_bf16(_p(w), _p(out), K, N, w.stride(0), out.stride(0), _stream(w))
    _ck(rc, "cast_transpose")
    return out


# ============================================================================ reductions
def _sum_all_raw(t: torch.Tensor, out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    t = t.contiguous()
    out_bf16 = out_dtype == torch.bfloat16 and t.data_ptr() % 16 == 0
    out = torch.empty((), dtype=torch.bfloat16 if out_bf16 else torch.float32, device=t.device)
    ps = _psum_for(t)
    if ps is not None:  # the producing GEMM already summed its output tile by tile
        rc = lib().ljs_sum_partials(_p(ps[0]), ps[1], _p(out), int(out_bf16), _stream(t))
        _ck(rc, "sum_partials")
        return out
    ws = _workspace(t.device, "sum_all", 1089 * 4)
    rc = lib().ljs_sum_all(_p(t), int(t.dtype == torch.bfloat16), t.numel(), _p(out), int(out_bf16), _p(ws),
                           _stream(t))
    _ck(rc, "sum_all")
    return out


# constant f32 gradient seeds (spmd.api._seed) -> their bf16 rounding, so the backward of a bf16
# sum fed by a cached seed needs no cast kernel
_SEEDS_BF16 = {}


def register_seed_bf16(seed: torch.Tensor, seed_bf16: torch.Tensor, value: Optional[float] = None) -> None:
    _SEEDS_BF16[seed.data_ptr()] = (seed, seed_bf16)
    if value is not None:
        bv = float(torch.tensor(value, dtype=torch.float32).to(torch.bfloat16).float())
        _SEED_CONST[seed.data_ptr()] = (seed, bv)
        _SEED_CONST[seed_bf16.data_ptr()] = (seed_bf16, bv)


def register_seed_const(seed: torch.Tensor, value: float) -> None:
    """A cached 1-element bf16 seed holding bf16(value) (spmd.api._seed)."""
    assert seed.dtype == torch.bfloat16 and seed.numel() == 1
    _SEED_CONST[seed.data_ptr()] = (seed, float(torch.tensor(value, dtype=torch.float32).to(torch.bfloat16).float()))


# constant seeds -> bf16(value) known on the host: a dense layer fed by one (the cotangent of a
# loss sum) takes its broadcast dY row from a cached constant and writes its bias gradient
# R * bf16(g) inside the weight-gradient combine -- no launch of its own (bcast_scalar)
_SEED_CONST = {}
_CONST_ROWS = {}


def seed_constant(g: torch.Tensor) -> Optional[float]:
    """bf16(value) of ``g`` when it is (a 1-element view of) a registered constant seed."""
    ent = _SEED_CONST.get(g.data_ptr())
    if ent is not None and ent[0].data_ptr() == g.data_ptr() and ent[0].dtype == g.dtype and ent[0].numel() == 1:
        return ent[1]
    return None


def const_row_bf16(value: float, n: int, device) -> Optional[torch.Tensor]:
    """A cached bf16 [n] row filled with ``value`` (None while a graph capture is running and
    the row does not exist yet: it is never allocated from a capture's private pool)."""
    key = (value, n, str(device))
    row = _CONST_ROWS.get(key)
    if row is None:
        if torch.cuda.is_current_stream_capturing():
            return None
        row = torch.full((n,), value, dtype=torch.bfloat16, device=device)
        _CONST_ROWS[key] = row
    return row


def _seed_bf16(g: torch.Tensor) -> torch.Tensor:
    ent = _SEEDS_BF16.get(g.data_ptr())
    if ent is not None and ent[0].data_ptr() == g.data_ptr() and ent[0].numel() == 1:
        return ent[1].reshape(())
    return _cast_raw(g.reshape(1), torch.bfloat16).reshape(())


class _SumAll(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, acc_dtype):
        ctx.shape, ctx.dtype = t.shape, t.dtype
        r = _sum_all_raw(t, acc_dtype)
        return r if r.dtype == acc_dtype else r.to(acc_dtype)

    @staticmethod
    def backward(ctx, g):
        if ctx.dtype == torch.bfloat16 and g.dtype in (torch.bfloat16, torch.float32) and g.is_cuda \
                and g.numel() == 1 and len(ctx.shape) >= 1:
            # the scalar itself, broadcast with all strides 0: a dense layer's backward turns it
            # into its bf16 row + bias gradient in one launch (bcast_scalar).  An f32 seed (the
            # f32 partial sum of a sharded loss) is rounded to bf16 first (one 1-element cast).
            gb = g.reshape(()) if g.dtype == torch.bfloat16 else _seed_bf16(g)
            return gb.expand(ctx.shape), None
        if ctx.dtype == torch.bfloat16 and g.dtype in (torch.float32, torch.bfloat16) and g.is_cuda \
                and len(ctx.shape) >= 1:
            # one bf16 row holding g, broadcast (stride 0) over every leading dim: the consumers
            # (GEMMs, column sums) read it with ld = 0 and nothing of the full shape is written
            n = ctx.shape[-1]
            row = torch.empty((n,), dtype=torch.bfloat16, device=g.device)
            rc = lib().ljs_fill_row_bf16(_p(g), int(g.dtype == torch.bfloat16), _p(row), n, _stream(g))
            _ck(rc, "fill_row")
            return row.expand(ctx.shape), None
        return g.to(ctx.dtype).expand(ctx.shape), None


def sum_all(t: torch.Tensor, acc_dtype: torch.dtype) -> torch.Tensor:
    if t.dtype not in (torch.float32, torch.bfloat16):
        return t.sum(dtype=acc_dtype)
    return _SumAll.apply(t, acc_dtype)


# gradients whose column sums a producer already computed (the fused MSE): data_ptr ->
# (weakref, version, f32 [C] sums); the dense backward takes its bias gradient from here
_COLSUMS = {}


def register_colsum(g: torch.Tensor, sums: torch.Tensor) -> None:
    import weakref
    key = g.data_ptr()
    ref = weakref.ref(g, lambda _r, k=key: _COLSUMS.pop(k, None) if _COLSUMS.get(k, (None,))[0] is _r else None)
    _COLSUMS[key] = (ref, g._version, sums, g.numel())


def colsum_for(t: torch.Tensor, C: int) -> Optional[torch.Tensor]:
    """Precomputed column sums of the [R][C] gradient ``t`` (any view of the registered storage
    with the same element count), or None."""
    ent = _COLSUMS.get(t.data_ptr())
    if ent is None:
        return None
    g = ent[0]()
    if g is None or g._version != ent[1] or ent[3] != t.numel():
        return None
    sums = ent[2]() if callable(ent[2]) else ent[2]   # (a lazy reduction, computed on first use)
    return sums if sums.numel() == C else None


class _MSELoss(torch.autograd.Function):
    """scale * sum((y - t)^2) of one shard (bf16 y, f32 / bf16 t).  When y needs a gradient the
    SAME kernel pass writes dY = bf16(2 * scale * (y - t)) and dY's column sums - the bias gradient
    of the dense layer that produced y (csrc/kernels/loss.hip): the loss's backward is then free
    for the constant seed grad() feeds it, a scalar multiply otherwise."""

    @staticmethod
    def forward(ctx, y, t, scale):
        want_dy = ctx.needs_input_grad[0]
        order = storage_order(y)
        if order is None or order[-1] != y.dim() - 1:
            y, order = y.contiguous(), tuple(range(y.dim()))
        yp = y.permute(order)                                    # contiguous: y's storage order
        tp = t.permute(order).contiguous()                       # the target in the same order
        out = torch.empty((), dtype=torch.float32, device=y.device)
        dy = torch.empty_like(yp).permute(_inv(order)) if want_dy else None
        C = y.shape[-1]
        R = y.numel() // max(1, C)
        sums = None
        if want_dy and C % 64 == 0 and y.dim() >= 2:
            sums = torch.empty((C,), dtype=torch.float32, device=y.device)
            nb = lib().ljs_mse_colsum_ws_bytes(R, C)
            # keyed by geometry: the ticket words sit at an offset that depends on (R, C), so a
            # workspace shared across geometries could hand a call a non-zero "ticket" left in
            # another call's partial-sum area (the last arriver would never be found)
            ws = _workspace(y.device, f"mse_colsum/{R}x{C}", nb)
            rc = lib().ljs_mse_colsum(_p(yp), _p(tp), int(tp.dtype == torch.bfloat16), R, C, float(scale), _p(dy),
                                      _p(sums), _p(out), _p(ws), _stream(y))
            _ck(rc, "mse_colsum")
        else:
            ws = _workspace(y.device, "mse", (1024 + 33) * 4)
            rc = lib().ljs_mse_loss(_p(yp), _p(tp), int(tp.dtype == torch.bfloat16), y.numel(), float(scale),
                                    _p(dy), _p(out), _p(ws), _stream(y))
            _ck(rc, "mse_loss")
        ctx.save_for_backward(dy, sums)
        ctx.t_dtype = t.dtype
        return out

    @staticmethod
    def backward(ctx, g):
        dy, sums = ctx.saved_tensors
        if dy is None:
            return None, None, None
        if seed_constant(g) == 1.0:
            gy = dy
            if sums is not None:
                register_colsum(gy, sums)
        else:
            gy = (dy.float() * g.float()).to(dy.dtype)
        gt = (-gy).to(ctx.t_dtype) if ctx.needs_input_grad[1] else None
        return gy, gt, None


def mse_loss(y: torch.Tensor, t: torch.Tensor, scale: float) -> torch.Tensor:
    ok = (y.dtype == torch.bfloat16 and t.dtype in (torch.float32, torch.bfloat16) and y.shape == t.shape
          and y.data_ptr() % 16 == 0 and t.data_ptr() % 16 == 0 and y.shape[-1] % 8 == 0)
    if not ok:
        return ((y.float() - t.float()) ** 2).sum() * scale
    return _MSELoss.apply(y, t, scale)


def colsum(t2d: torch.Tensor, out: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    R, C = t2d.shape
    if t2d.stride(1) != 1:
        t2d = t2d.contiguous()
    if out is None:
        out = torch.empty((C,), dtype=torch.float32, device=t2d.device)
    ws = _workspace(t2d.device, "colsum", _COLSUM_WS_BYTES)
    rc = lib().ljs_colsum(_p(t2d), int(t2d.dtype == torch.bfloat16), R, C, t2d.stride(0), _p(out), int(accumulate),
                          _p(ws), _stream(t2d))
    _ck(rc, "colsum")
    return out


class _Softmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        y = torch.empty_like(x)
        L = x.shape[-1]
        rc = lib().ljs_softmax_rows_f32(_p(x), _p(y), x.numel() // L, L, _stream(x))
        _ck(rc, "softmax")
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        return y * (dy - (dy * y).sum(-1, keepdim=True))


def softmax_lastdim(x: torch.Tensor) -> torch.Tensor:
    return _Softmax.apply(x)


# ============================================================================ layer / rms norm
_NORM_KINDS = {"layer": 0, "rms": 1}
_NORM_DTYPES = (torch.float32, torch.bfloat16)


def norm_supported(D: int, dtype: torch.dtype) -> bool:
    """Whether the fused norm kernels (csrc/kernels/norm.hip) take rows of ``D`` features of ``dtype``."""
    return D % 8 == 0 and 8 <= D <= 8192 and dtype in _NORM_DTYPES


def _norm_in_place(t: torch.Tensor) -> bool:
    """Whether the kernels can take ``t`` as it is: dense (rows of ``t.shape[-1]`` contiguous elements
    with no gaps, in any row order - a seq-major activation) and 16-byte aligned."""
    return t.stride(-1) == 1 and t.data_ptr() % 16 == 0 and storage_order(t) is not None


def _norm_param(p: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    if p is None:
        return None
    p = p.detach()
    if p.dtype != torch.float32 or not p.is_contiguous() or p.data_ptr() % 16:
        p = p.float().contiguous().clone()
    return p


def _norm_ws(t: torch.Tensor, nbytes: int) -> torch.Tensor:
    """The backward's ticket / partial-row workspace: one per device, stream and size, so launches
    that could overlap (two streams) never share ticket words; virtual devices that share a GPU
    issue on one stream, in order.  A capture takes the device's ``graph`` workspace: captures are
    made on fresh streams, and a workspace first made inside one would replay its zero-fill.  Never
    regrown: a captured graph keeps the address it recorded."""
    tag = "graph" if torch.cuda.is_current_stream_capturing() else str(_stream(t))
    return _workspace(t.device, f"norm/{tag}/{nbytes}", nbytes)


class _Norm(torch.autograd.Function):
    """LayerNorm / RMSNorm of one shard over its last dim: one HIP launch forward (y, and the rows'
    mean / rstd for the backward), one backward (dx, d(scale), d(bias); whichever are not needed are
    skipped).  Rows are independent, so a dense shard is processed in storage order, whatever its
    row order, and ``y`` / ``dx`` take ``x``'s strides."""

    @staticmethod
    def forward(ctx, x, scale, bias, eps, kind, out_dtype):
        D = x.shape[-1]
        if not _norm_in_place(x):
            x = x.contiguous()
        R = x.numel() // D
        y = torch.empty_strided(x.shape, x.stride(), dtype=out_dtype, device=x.device)
        layer = kind == "layer"
        rstd = torch.empty((R,), dtype=torch.float32, device=x.device)
        mean = torch.empty((R,), dtype=torch.float32, device=x.device) if layer else None
        sc, bi = _norm_param(scale), _norm_param(bias) if layer else None
        rc = lib().ljs_norm_fwd(_p(x), int(x.dtype == torch.bfloat16), D, _p(sc), _p(bi), _p(y),
                                int(out_dtype == torch.bfloat16), D, _p(mean), _p(rstd), R, D, float(eps),
                                _NORM_KINDS[kind], _stream(x))
        _ck(rc, "norm_fwd")
        ctx.save_for_backward(x, sc, mean, rstd)
        ctx.meta = (kind, R, out_dtype, scale.dtype if scale is not None else None,
                    bias.dtype if bias is not None else None)
        return y

    @staticmethod
    def backward(ctx, g):
        x, sc, mean, rstd = ctx.saved_tensors
        kind, R, out_dtype, sdt, bdt = ctx.meta
        D = x.shape[-1]
        need_dx = ctx.needs_input_grad[0]
        need_ds = sdt is not None and ctx.needs_input_grad[1]
        need_db = bdt is not None and kind == "layer" and ctx.needs_input_grad[2]
        zero_db = bdt is not None and kind != "layer" and ctx.needs_input_grad[2]
        if g.dtype != out_dtype or g.stride() != x.stride() or g.data_ptr() % 16:
            # the cotangent in y's dtype and row order
            g = torch.empty_strided(x.shape, x.stride(), dtype=out_dtype, device=x.device).copy_(g)
        dx = ds = db = None
        if need_dx:
            dx = torch.empty_strided(x.shape, x.stride(), dtype=x.dtype, device=x.device)
        if need_ds:
            ds = torch.empty((D,), dtype=torch.float32, device=x.device)
        if need_db:
            db = torch.empty((D,), dtype=torch.float32, device=x.device)
        if need_dx or need_ds or need_db:
            ws = _norm_ws(x, lib().ljs_norm_bwd_ws_bytes(R, D)) if need_ds or need_db else None
            rc = lib().ljs_norm_bwd(_p(x), int(x.dtype == torch.bfloat16), D, _p(g),
                                    int(out_dtype == torch.bfloat16), D, _p(sc), _p(mean), _p(rstd), _p(dx), D, R, D,
                                    _NORM_KINDS[kind], _p(ws), _p(ds), _p(db), _stream(x))
            _ck(rc, "norm_bwd")
        if ds is not None and sdt != torch.float32:
            ds = ds.to(sdt)
        if db is not None and bdt != torch.float32:
            db = db.to(bdt)
        if zero_db:
            db = torch.zeros((D,), dtype=bdt, device=x.device)
        return dx, ds, db, None, None, None


def norm(x: torch.Tensor, scale: Optional[torch.Tensor], bias: Optional[torch.Tensor], eps: float,
         kind: str = "layer", out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """``kind`` = ``layer``: ``(x - mean) rsqrt(var + eps) scale + bias``; ``rms``: ``x rsqrt(mean(x^2) + eps)
    scale`` (``bias`` ignored) over the last dim of one shard, statistics in f32; ``x`` and the result f32 or
    bf16 independently, ``scale`` / ``bias`` ``[D]`` or None."""
    out_dtype = out_dtype or x.dtype
    if kind not in _NORM_KINDS:
        raise ValueError(f"norm kind must be 'layer' or 'rms', got {kind!r}")
    if not norm_supported(x.shape[-1], x.dtype) or out_dtype not in _NORM_DTYPES:
        raise NotImplementedError(f"norm kernel: f32 / bf16 rows of 8..8192 features (a multiple of 8), got "
                                  f"{x.dtype} -> {out_dtype}, D = {x.shape[-1]}")
    return _Norm.apply(x, scale, bias, float(eps), kind, out_dtype)


# ============================================================================ softmax cross-entropy
_XENT_DTYPES = (torch.float32, torch.bfloat16)
_XENT_LABELS = (torch.int32, torch.int64)


def __getattr__(name):
    # XENT_WAVE_MAX_V: the widest row (elements) that takes the one-wave-per-row mapping of the
    # cross-entropy kernels; wider rows take one block each.  Read from the library, not repeated.
    if name == "XENT_WAVE_MAX_V":
        return int(lib().ljs_xent_wave_max_v())
    # EMBED_CHUNK: tokens of one table row's list that one wave of the embedding backward sums (a
    # longer list is cut into chunks of this many); EMBED_ALLPAIRS_MAX_TOKENS: most tokens whose
    # inverted index the all-pairs rank kernel builds (above: a stable torch.sort).
    if name == "EMBED_CHUNK":
        return int(lib().ljs_embed_chunk())
    if name == "EMBED_ALLPAIRS_MAX_TOKENS":
        return int(lib().ljs_embed_allpairs_max_tokens())
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def xent_supported(logits: torch.Tensor, labels: torch.Tensor) -> bool:
    """Whether the fused cross-entropy kernels (csrc/kernels/xent.hip) take these: f32 or bf16 logits
    of any vocabulary size >= 1, int32 or int64 labels of the logits' leading shape, not empty."""
    return (logits.dim() >= 1 and logits.dtype in _XENT_DTYPES and labels.dtype in _XENT_LABELS
            and tuple(labels.shape) == tuple(logits.shape[:-1]) and 1 <= logits.shape[-1] < 2 ** 31
            and logits.numel() > 0)


def _xent_rows(x: torch.Tensor):
    """``x`` as rows of its last dim for the kernels: (tensor kept alive, row count, row stride).
    A matrix whose rows are contiguous is taken as it is, whatever its row stride; anything else
    as its contiguous copy."""
    V = x.shape[-1]
    if x.dim() == 2 and x.stride(1) == 1 and (x.stride(0) >= V or x.shape[0] == 1):
        return x, x.shape[0], max(x.stride(0), V)
    x = x.contiguous()
    return x, x.numel() // V, V


def _xent_fwd(x: torch.Tensor, labels: torch.Tensor, vocab_offset: int, want_loss: bool):
    xr, R, ld = _xent_rows(x.detach())
    V = x.shape[-1]
    lab = labels.detach().reshape(-1).contiguous()
    m, s, t = (torch.empty((R,), dtype=torch.float32, device=x.device) for _ in range(3))
    loss = torch.empty((R,), dtype=torch.float32, device=x.device) if want_loss else None
    rc = lib().ljs_xent_fwd(_p(xr), int(xr.dtype == torch.bfloat16), ld, _p(lab), int(lab.dtype == torch.int64),
                            int(vocab_offset), _p(m), _p(s), _p(t), _p(loss), R, V, _stream(x))
    _ck(rc, "xent_fwd")
    return xr, ld, lab, m, s, t, loss


def _xent_bwd(xr: torch.Tensor, ld: int, lab: torch.Tensor, vocab_offset: int, m, s, a, b, shape) -> torch.Tensor:
    """dx = a exp(x - m) / s - b onehot(label), a fresh contiguous tensor of ``shape`` in x's dtype."""
    V = shape[-1]
    R = lab.numel()
    dx = torch.empty(shape, dtype=xr.dtype, device=xr.device)
    a = a.detach().reshape(-1).to(torch.float32).contiguous()
    b = b.detach().reshape(-1).to(torch.float32).contiguous()
    rc = lib().ljs_xent_bwd(_p(xr), int(xr.dtype == torch.bfloat16), ld, _p(lab), int(lab.dtype == torch.int64),
                            int(vocab_offset), _p(m), _p(s), _p(a), _p(b), _p(dx), V, R, V, _stream(xr))
    _ck(rc, "xent_bwd")
    return dx


class _Xent(torch.autograd.Function):
    """Softmax cross-entropy rows of one shard that holds the whole vocabulary: one HIP launch
    forward (the loss rows, and the rows' max / sum-exp for the backward), one backward (dx in the
    logits' dtype from the logits, the two statistics and the loss rows' cotangent)."""

    @staticmethod
    def forward(ctx, logits, labels):
        xr, ld, lab, m, s, _, loss = _xent_fwd(logits, labels, 0, True)
        ctx.save_for_backward(xr, lab, m, s)
        ctx.meta = (ld, tuple(logits.shape))
        return loss.view(logits.shape[:-1])

    @staticmethod
    def backward(ctx, g):
        xr, lab, m, s = ctx.saved_tensors
        ld, shape = ctx.meta
        if not ctx.needs_input_grad[0]:
            return None, None
        return _xent_bwd(xr, ld, lab, 0, m, s, g, g, shape), None


class _XentStats(torch.autograd.Function):
    """The statistics of one vocabulary shard: ``(m, log s, t)`` per row, ``m`` the shard's row maximum
    (not differentiable: the loss does not depend on it), ``s = sum exp(x - m)``, ``t = x[label] - m`` where
    the shard owns the label, else 0.  With ``m`` held constant d(log s)/dx = exp(x - m) / s and
    dt/dx = onehot(label), so the cotangents of ``log s`` and ``t`` are the backward kernel's two
    row coefficients."""

    @staticmethod
    def forward(ctx, logits, labels, vocab_offset):
        xr, ld, lab, m, s, t, _ = _xent_fwd(logits, labels, vocab_offset, False)
        ctx.save_for_backward(xr, lab, m, s)
        ctx.meta = (ld, tuple(logits.shape), int(vocab_offset))
        lead = logits.shape[:-1]
        m = m.view(lead)
        ctx.mark_non_differentiable(m)
        return m, torch.log(s).view(lead), t.view(lead)

    @staticmethod
    def backward(ctx, gm, gls, gt):
        xr, lab, m, s = ctx.saved_tensors
        ld, shape, vocab_offset = ctx.meta
        if not ctx.needs_input_grad[0]:
            return None, None, None
        a = gls if gls is not None else torch.zeros_like(m)
        b = -gt if gt is not None else torch.zeros_like(m)
        return _xent_bwd(xr, ld, lab, vocab_offset, m, s, a, b, shape), None, None


def _xent_check(logits: torch.Tensor, labels: torch.Tensor):
    if not xent_supported(logits, labels):
        raise NotImplementedError(f"xent kernels: f32 / bf16 logits [..., V >= 1] with int32 / int64 labels [...], got "
                                  f"{logits.dtype} {tuple(logits.shape)} and {labels.dtype} {tuple(labels.shape)}")


def xent(logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """``logsumexp(logits) - logits[label]`` per row over the last dim (the whole vocabulary), f32 of shape
    ``logits.shape[:-1]``; a label < 0 marks an ignored row (loss 0, zero gradient row)."""
    _xent_check(logits, labels)
    return _Xent.apply(logits, labels)


def xent_stats(logits: torch.Tensor, labels: torch.Tensor, vocab_offset: int = 0):
    """``(m, log s, t)`` of one vocabulary shard whose column 0 is global column ``vocab_offset`` (see
    :class:`_XentStats`); shards merge with ``M = max m_i``, ``S = sum s_i e^(m_i - M)``,
    ``loss = log S - sum own_i (t_i + m_i - M)``."""
    _xent_check(logits, labels)
    return _XentStats.apply(logits, labels, int(vocab_offset))


# ============================================================================ embedding lookup
_EMBED_DTYPES = (torch.float32, torch.bfloat16)
_EMBED_IDS = (torch.int32, torch.int64)


def embed_supported(table: torch.Tensor, ids: torch.Tensor, out_dtype: Optional[torch.dtype] = None) -> bool:
    """Whether the fused embedding kernels (csrc/kernels/embed.hip) take these: an f32 or bf16 table
    ``[V, D]`` with D a multiple of 8 in 8..8192 (the norm kernels' rule), int32 or int64 ids of any
    shape, not empty, an f32 or bf16 output."""
    if table.dim() != 2 or table.dtype not in _EMBED_DTYPES or ids.dtype not in _EMBED_IDS:
        return False
    V, D = table.shape
    return ((out_dtype or table.dtype) in _EMBED_DTYPES and D % 8 == 0 and 8 <= D <= 8192 and 1 <= V < 2 ** 31
            and 0 < ids.numel() < 2 ** 31 - 1024)


def _embed_ws(t: torch.Tensor, nbytes: int) -> torch.Tensor:
    """The index build's histogram: zero between launches (the scan kernel re-zeroes it), under the
    rules of :func:`_norm_ws`: one per device, stream and size, a ``graph`` one under capture,
    never regrown."""
    tag = "graph" if torch.cuda.is_current_stream_capturing() else str(_stream(t))
    return _workspace(t.device, f"embed/{tag}/{nbytes}", nbytes)


def _embed_index(ids: torch.Tensor, vocab_offset: int, V: int):
    """The inverted index of flat ``ids`` over table rows ``vocab_offset .. vocab_offset + V``:
    (start ``[V + 1]``, list ``[T]``, work list, its capacity), all int32.  Up to
    ``EMBED_ALLPAIRS_MAX_TOKENS`` tokens by the rank / scan / fill kernels; above, the list is the
    permutation of a stable ``torch.sort`` and only the scan kernel runs.  Either way each row's
    tokens come out in ascending order."""
    T, dev = ids.numel(), ids.device
    cap = int(lib().ljs_embed_work_cap(T))
    i32 = dict(dtype=torch.int32, device=dev)
    start, work = torch.empty(V + 1, **i32), torch.empty(2 + 2 * cap, **i32)
    vpad = (V + 3) // 4 * 4
    if T <= int(lib().ljs_embed_allpairs_max_tokens()):
        lst, rank = torch.empty(T, **i32), torch.empty(T, **i32)
        hist = _embed_ws(ids, vpad * 4)
        rc = lib().ljs_embed_index(_p(ids), int(ids.dtype == torch.int64), int(vocab_offset), T, V, _p(hist),
                                   _p(rank), _p(start), _p(lst), _p(work), cap, _stream(ids))
        _ck(rc, "embed_index")
        return start, lst, work, cap
    loc = ids.long() - int(vocab_offset)
    loc = torch.where((loc >= 0) & (loc < V), loc, torch.full_like(loc, V))  # unowned tokens sort last
    lst = torch.sort(loc, stable=True)[1].to(torch.int32)
    hist = torch.zeros(vpad + 4, **i32)
    hist.index_add_(0, loc, torch.ones(T, **i32))  # integer adds: the counts do not depend on their order
    hist[V:].zero_()
    rc = lib().ljs_embed_scan(_p(hist), V, _p(start), _p(work), cap, _stream(ids))
    _ck(rc, "embed_scan")
    return start, lst, work, cap


def embed_grad(dy: torch.Tensor, ids: torch.Tensor, num_rows: int, vocab_offset: int = 0,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The table gradient of :func:`embed`: f32 ``[num_rows, D]`` with row ``v`` the sum of the ``dy`` rows
    (f32 or bf16, ``[*ids.shape, D]``) of the tokens whose id is ``vocab_offset + v``, added in f32 in
    ascending token order (lists longer than ``EMBED_CHUNK`` per chunk, then the chunks in order).
    No float atomics; every row of ``out`` (given, or fresh) is written, unchosen rows as zeros."""
    D = dy.shape[-1]
    ids = ids.detach().reshape(-1).contiguous()
    T = ids.numel()
    dy = dy.detach().reshape(T, D)
    if dy.dtype not in _EMBED_DTYPES:
        dy = dy.float()
    if not dy.is_contiguous() or dy.data_ptr() % 16:
        dy = dy.contiguous().clone() if dy.is_contiguous() else dy.contiguous()
    if out is None:
        out = torch.empty((num_rows, D), dtype=torch.float32, device=dy.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (num_rows, D) or not out.is_contiguous():
        raise ValueError(f"embed_grad: out must be a contiguous f32 [{num_rows}, {D}] tensor")
    start, lst, work, cap = _embed_index(ids, vocab_offset, num_rows)
    partial = torch.empty((cap, D), dtype=torch.float32, device=dy.device) if cap else None
    rc = lib().ljs_embed_bwd(_p(dy), int(dy.dtype == torch.bfloat16), T, D, num_rows, _p(start), _p(lst), _p(work),
                             cap, _p(partial), _p(out), _stream(dy))
    _ck(rc, "embed_bwd")
    return out


class _Embed(torch.autograd.Function):
    """Rows of one table shard by id: one HIP launch forward; backward the inverted index of the ids
    (three launches) and the sum pass (one, and one more that adds the chunks of long lists), or
    with ``fused_bwd`` off torch's ``index_add_`` (float atomics: the sum order is not fixed)."""

    @staticmethod
    def forward(ctx, table, ids, vocab_offset, out_dtype, fused_bwd):
        V, D = table.shape
        tab = table.detach()
        es = tab.element_size()
        if tab.stride(1) != 1 or tab.stride(0) < D or (tab.stride(0) * es) % 16 or tab.data_ptr() % 16:
            tab = tab.contiguous()
        idf = ids.detach().reshape(-1).contiguous()
        out = torch.empty(tuple(ids.shape) + (D,), dtype=out_dtype, device=table.device)
        rc = lib().ljs_embed_fwd(_p(tab), int(tab.dtype == torch.bfloat16), tab.stride(0), _p(idf),
                                 int(idf.dtype == torch.int64), int(vocab_offset), _p(out),
                                 int(out_dtype == torch.bfloat16), idf.numel(), V, D, _stream(table))
        _ck(rc, "embed_fwd")
        ctx.save_for_backward(idf)
        ctx.meta = (V, D, table.dtype, int(vocab_offset), bool(fused_bwd))
        return out

    @staticmethod
    def backward(ctx, g):
        (idf,) = ctx.saved_tensors
        V, D, tdt, vocab_offset, fused_bwd = ctx.meta
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        if fused_bwd:
            dt = embed_grad(g, idf, V, vocab_offset)
        else:
            loc = idf.long() - vocab_offset
            own = (loc >= 0) & (loc < V)
            gf = torch.where(own.unsqueeze(-1), g.detach().reshape(-1, D).float(), g.new_zeros((), dtype=torch.float32))
            dt = torch.zeros((V, D), dtype=torch.float32, device=g.device).index_add_(0, loc.clamp(0, V - 1), gf)
        return (dt if tdt == torch.float32 else dt.to(tdt)), None, None, None, None


def embed(table: torch.Tensor, ids: torch.Tensor, vocab_offset: int = 0, out_dtype: Optional[torch.dtype] = None,
          fused_bwd: bool = True) -> torch.Tensor:
    """``table[ids - vocab_offset]`` as ``[*ids.shape, D]`` in ``out_dtype`` (default: the table's), a row of
    zeros (and no gradient) for an id outside ``vocab_offset .. vocab_offset + V``: a negative id, one
    past the vocabulary, one that another vocabulary shard owns.  The table's gradient is f32 sums in
    a fixed order (:func:`embed_grad`), cast to the table's dtype."""
    out_dtype = out_dtype or table.dtype
    if not embed_supported(table, ids, out_dtype):
        raise NotImplementedError(f"embed kernels: an f32 / bf16 table [V, D] with D a multiple of 8 in 8..8192, "
                                  f"int32 / int64 ids, f32 / bf16 out; got {table.dtype} {tuple(table.shape)}, "
                                  f"{ids.dtype} {tuple(ids.shape)} -> {out_dtype}")
    return _Embed.apply(table, ids, int(vocab_offset), out_dtype, bool(fused_bwd))


# ============================================================================ rotary embedding
_ROPE_DTYPES = (torch.float32, torch.bfloat16)


def set_rope_max_blocks(n: Optional[int]) -> None:
    """Cap the rope kernel's grid at ``n`` blocks (tests: the grid-stride loop on small shapes);
    None or <= 0 = the default, a fixed number of blocks per compute unit."""
    lib().ljs_rope_set_max_blocks(-1 if n is None else int(n))


def rope_supported(t: torch.Tensor, out_dtype: Optional[torch.dtype] = None) -> bool:
    """Whether csrc/kernels/rope.hip takes ``t`` as it is: f32 / bf16 ``(B, S, H, D)``, D a multiple of
    16 in 16..256 and contiguous, the base and the three outer strides 16-byte aligned."""
    if t.dim() != 4 or t.dtype not in _ROPE_DTYPES or (out_dtype or t.dtype) not in _ROPE_DTYPES or not t.numel():
        return False
    D, es = t.shape[-1], t.element_size()
    return (D % 16 == 0 and 16 <= D <= 256 and t.stride(-1) == 1 and t.data_ptr() % 16 == 0
            and all((t.stride(i) * es) % 16 == 0 for i in range(3)))


def rope_raw(q, k, q_out, k_out, cos, sin, pos_offset: int, inverse: bool = False) -> int:
    """One ``ljs_rope`` launch on the tensors as they are; returns the launcher's code (non-zero:
    rejected, nothing launched) instead of raising."""
    B, S, H, D = q.shape
    return lib().ljs_rope(_p(q), _p(k), _p(q_out), _p(k_out), int(q.dtype == torch.bfloat16),
                          int(q_out.dtype == torch.bfloat16), B, S, H, D, _longs(_strides3(q)),
                          _longs(_strides3(k)) if k is not None else None, _longs(_strides3(q_out)),
                          _longs(_strides3(k_out)) if k_out is not None else None, _p(cos), _p(sin),
                          cos.shape[0], int(pos_offset), int(bool(inverse)), _stream(q))


def _rope_launch(q, k, pos_offset: int, theta: float, out_dtype: torch.dtype, inverse: bool):
    """(q', k') of one launch; the outputs are fresh tensors stored like the inputs' (batch, seq)."""
    from .kernels import rope_table
    B, S, H, D = q.shape
    cos, sin = rope_table(q.device, D, theta, pos_offset + S)
    qo = _bs_like(q.shape, q, out_dtype)
    ko = _bs_like(k.shape, k, out_dtype) if k is not None else None
    _ck(rope_raw(q, k, qo, ko, cos, sin, pos_offset, inverse), "rope")
    return qo, ko


class _Rope(torch.autograd.Function):
    """Rotary embedding of q and k (k may be None) in one HIP launch; the backward is the same
    kernel with the inverse flag on (dq', dk').

    The rotation is out of place even where q and k are column blocks of the fused QKV projection
    buffer: they are two of the several output views of the dense Function, and autograd forbids
    modifying one of a Function's multiple output views in place."""

    @staticmethod
    def forward(ctx, q, k, pos_offset, theta, out_dtype):
        ctx.meta = (pos_offset, theta, q.dtype, tuple(q.shape))
        qo, ko = _rope_launch(q.detach(), None if k is None else k.detach(), pos_offset, theta, out_dtype, False)
        return qo, ko

    @staticmethod
    def backward(ctx, gq, gk):
        pos_offset, theta, in_dtype, shape = ctx.meta
        want_q, want_k = ctx.needs_input_grad[0], ctx.needs_input_grad[1] and gk is not None

        def ready(g):
            # the kernel's cotangent: f32 / bf16 with D contiguous and aligned strides
            g = g.detach()
            if g.dtype not in _ROPE_DTYPES:
                g = g.float()
            return g if rope_supported(g) else g.contiguous().clone()

        gs = [ready(g) for g, w in ((gq, want_q), (gk, want_k)) if w and g is not None]
        if not gs:
            return None, None, None, None, None
        if len(gs) == 2 and gs[0].dtype != gs[1].dtype:
            gs = [g.float() for g in gs]
        outs = list(_rope_launch(gs[0], gs[1] if len(gs) == 2 else None, pos_offset, theta, in_dtype, True))
        dq = outs.pop(0) if want_q and gq is not None else None
        dk = outs.pop(0) if want_k else None
        return dq, dk, None, None, None


def rope(q: torch.Tensor, k: Optional[torch.Tensor] = None, pos_offset: int = 0, theta: float = 10000.0,
         out_dtype: Optional[torch.dtype] = None):
    """Rotary embedding (half-split pairs, see :mod:`.kernels`) of ``(B, S, H, D)`` shards whose first
    position is ``pos_offset``: ``(q', k')`` in ``out_dtype`` (default: the inputs'), ``k'`` None without k."""
    out_dtype = out_dtype or q.dtype
    ts = [q] + ([k] if k is not None else [])
    if any(t.shape != q.shape or t.dtype != q.dtype or not rope_supported(t, out_dtype) for t in ts):
        raise NotImplementedError(f"rope kernel: f32 / bf16 (B, S, H, D) with D a multiple of 16 in 16..256, D "
                                  f"contiguous, 16-byte aligned base and strides; got {q.dtype} {tuple(q.shape)} "
                                  f"strides {q.stride()} -> {out_dtype}")
    return _Rope.apply(q, k, int(pos_offset), float(theta), out_dtype)


# ============================================================================ SwiGLU
_SWIGLU_DTYPES = (torch.float32, torch.bfloat16)


def set_swiglu_max_blocks(n: Optional[int]) -> None:
    """Cap the swiglu kernels' grid at ``n`` blocks (tests: the grid-stride loop on small shapes);
    None or <= 0 = the default, a fixed number of blocks per compute unit."""
    lib().ljs_swiglu_set_max_blocks(-1 if n is None else int(n))


def _bsf(t: torch.Tensor) -> Optional[torch.Tensor]:
    """``t`` as a (B, S, F) view (the kernels' shape), or None where its leading dims do not
    collapse without a copy."""
    if t.dim() == 3:
        return t
    if t.dim() < 3:
        return t.reshape((1,) * (3 - t.dim()) + tuple(t.shape)) if t.dim() else None
    try:
        return t.view(-1, t.shape[-2], t.shape[-1])
    except RuntimeError:
        return None


def _swiglu_operand(t: torch.Tensor) -> bool:
    if t.dim() < 1 or t.dtype not in _SWIGLU_DTYPES or not t.numel():
        return False
    F, es = t.shape[-1], t.element_size()
    if F < 8 or F % 8 or t.stride(-1) != 1 or t.data_ptr() % 16:
        return False
    t3 = _bsf(t)
    return t3 is not None and all((t3.stride(i) * es) % 16 == 0 for i in range(2))


def swiglu_supported(g: torch.Tensor, u: torch.Tensor, out_dtype: Optional[torch.dtype] = None) -> bool:
    """Whether csrc/kernels/swiglu.hip takes ``g`` and ``u`` as they are: f32 / bf16 of one shape and
    dtype, the last dim a multiple of 8 and contiguous, bases and outer strides 16-byte aligned."""
    return (g.shape == u.shape and g.dtype == u.dtype and (out_dtype or g.dtype) in _SWIGLU_DTYPES
            and _swiglu_operand(g) and _swiglu_operand(u))


def _strides2(t: torch.Tensor):
    return [t.stride(0), t.stride(1)]


def _swiglu_raw_ok(g, u, *rest) -> bool:
    # what the C entry cannot see: one (B, S, F) shape for all, F contiguous, one dtype for g and u
    return (g.dim() == 3 and u.dtype == g.dtype and all(
        t.shape == g.shape and t.stride(-1) == 1 and t.dtype in _SWIGLU_DTYPES for t in (g, u) + rest))


def swiglu_raw(g, u, h) -> int:
    """One ``ljs_swiglu`` launch on (B, S, F) tensors as they are; returns the launcher's code
    (non-zero: rejected, nothing launched) instead of raising."""
    if not _swiglu_raw_ok(g, u, h):
        return 1
    B, S, F = g.shape
    return lib().ljs_swiglu(_p(g), _p(u), _p(h), int(g.dtype == torch.bfloat16), int(h.dtype == torch.bfloat16),
                            B, S, F, _longs(_strides2(g)), _longs(_strides2(u)), _longs(_strides2(h)), _stream(g))


def swiglu_bwd_raw(g, u, dh, dg, du) -> int:
    """One ``ljs_swiglu_bwd`` launch on (B, S, F) tensors as they are; the launcher's code."""
    if not _swiglu_raw_ok(g, u, dh, dg, du) or dg.dtype != g.dtype or du.dtype != g.dtype:
        return 1
    B, S, F = g.shape
    return lib().ljs_swiglu_bwd(_p(g), _p(u), _p(dh), _p(dg), _p(du), int(g.dtype == torch.bfloat16),
                                int(dh.dtype == torch.bfloat16), B, S, F, _longs(_strides2(g)),
                                _longs(_strides2(u)), _longs(_strides2(dh)), _longs(_strides2(dg)),
                                _longs(_strides2(du)), _stream(g))


def _bsf_like(ref: torch.Tensor, F: int, dtype: torch.dtype) -> torch.Tensor:
    """Empty (B, S, F) stored like ``ref``'s (batch, position) dims: seq-major when ref is."""
    B, S = ref.shape[0], ref.shape[1]
    if B > 1 and S > 1 and ref.stride(1) > ref.stride(0):
        return torch.empty((S, B, F), dtype=dtype, device=ref.device).permute(1, 0, 2)
    return torch.empty((B, S, F), dtype=dtype, device=ref.device)


class _Swiglu(torch.autograd.Function):
    """``silu(g) * u`` in one HIP launch; the backward is one launch that recomputes the sigmoid from
    g and writes (dg, du).  Where g and u are the two adjacent column blocks of one [T][2F] buffer
    (the fused gate / up projection's output), dg and du are the same column blocks of one fresh
    buffer: the adjacency the projection's backward looks for (ops/linear.py _wgrads)."""

    @staticmethod
    def forward(ctx, g, u, out_dtype):
        g3, u3 = _bsf(g.detach()), _bsf(u.detach())
        h = _bsf_like(g3, g3.shape[-1], out_dtype)
        _ck(swiglu_raw(g3, u3, h), "swiglu")
        ctx.save_for_backward(g3, u3)
        ctx.shape = tuple(g.shape)
        return h.reshape(ctx.shape) if g.dim() != 3 else h

    @staticmethod
    def backward(ctx, dh):
        g3, u3 = ctx.saved_tensors
        F, es = g3.shape[-1], g3.element_size()
        dh = dh.detach()
        if dh.dtype not in _SWIGLU_DTYPES:
            dh = dh.float()
        dh3 = _bsf(dh) if _swiglu_operand(dh) else None
        if dh3 is None:
            dh3 = _bsf(dh.contiguous().clone() if dh.is_contiguous() else dh.contiguous())
        if g3.stride() == u3.stride() and u3.data_ptr() == g3.data_ptr() + F * es:
            both = _bsf_like(g3, 2 * F, g3.dtype)
            dg, du = both[..., :F], both[..., F:]
        else:
            dg, du = _bsf_like(g3, F, g3.dtype), _bsf_like(g3, F, g3.dtype)
        _ck(swiglu_bwd_raw(g3, u3, dh3, dg, du), "swiglu_bwd")
        if len(ctx.shape) != 3:
            dg, du = dg.reshape(ctx.shape), du.reshape(ctx.shape)
        return (dg if ctx.needs_input_grad[0] else None), (du if ctx.needs_input_grad[1] else None), None


def swiglu(g: torch.Tensor, u: torch.Tensor, out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """``silu(g) * u`` of one device's shards in ``out_dtype`` (default: the inputs')."""
    out_dtype = out_dtype or g.dtype
    if not swiglu_supported(g, u, out_dtype):
        raise NotImplementedError(f"swiglu kernels: f32 / bf16 g and u of one shape and dtype, the last dim a "
                                  f"contiguous multiple of 8, 16-byte aligned bases and strides; got {g.dtype} "
                                  f"{tuple(g.shape)} strides {g.stride()} / {u.dtype} {tuple(u.shape)} strides "
                                  f"{u.stride()} -> {out_dtype}")
    return _Swiglu.apply(g, u, out_dtype)


# ============================================================================ dense / linear
def linear(x: torch.Tensor, ws: List[torch.Tensor], b: Optional[torch.Tensor], compute_dtype: torch.dtype,
           relu: bool, out_dtype: torch.dtype, residual: Optional[torch.Tensor] = None) -> List[torch.Tensor]:
    """Fused dense layer (see :mod:`.linear`).  Every GPU shape runs on a HIP GEMM:

    * bf16 compute, K and N multiples of 8, f32 row-major kernels: the fused MFMA path;
    * the same under ``no_grad`` with at most 16 rows (any row count) and ``K % 32 == 0``: one
      weight-streaming ``skinny<`` launch (:func:`skinny`; ``LJS_SKINNY_GEMM=0``: as without it);
    * bf16 compute otherwise: the same path on zero-padded operands (rows M, K and N up to the
      next multiple of 8; zero rows/columns change no sum), result sliced back;
    * f32 compute: the MFMA ``v_mfma_f32_16x16x4f32`` GEMM (:class:`_MatmulF32`, strided
      operands, its own backward), bias and ReLU as elementwise epilogues.

    ``residual`` (same shape as the output) is added after the activation - in the GEMM
    epilogue on the fused path.

    Anything else raises unless ``LJS_ALLOW_TORCH_FALLBACK=1`` (debugging only)."""
    from . import linear as _lin
    # (at most 16 rows without a backward: the skinny GEMM takes any row count, so M = 1 .. 7 and other
    # non-multiples of 8 do not leave through the padded path)
    if compute_dtype == torch.bfloat16:
        sk = _lin.skinny_route(x, ws, b)       # (False at once with grad enabled; evaluated once per call)
        if sk or _lin.supported(x, ws, b):
            return _lin.linear(x, list(ws), b, relu, out_dtype, residual=residual, skinny=sk)
    from . import shadow
    if any(shadow.is_proxy(w) for w in ws):
        # a gathered-weight proxy holds no f32 values; a shape the fused path does not take (M, K
        # or N not a multiple of 8) reads the f32 values bf16(w) recovered from the gathered bf16
        # copy - exactly what a bf16-compute GEMM would round the f32 weight to
        ws = [_ProxyValues.apply(w) if shadow.is_proxy(w) else w for w in ws]
    outs = _linear_any(x, ws, b, compute_dtype, relu, out_dtype)
    if residual is not None:
        outs = [outs[0] + residual.to(outs[0].dtype)] + outs[1:]
    return outs


class _ProxyValues(torch.autograd.Function):
    """f32 values of a gathered-weight proxy (``parallel/weight_gather.py``) from its gathered bf16
    copy (the "T" shadow, [N][K]); the gradient passes through unchanged to the proxy, whose
    backward reduce-scatters it onto the shards."""

    @staticmethod
    def forward(ctx, w):
        from . import shadow
        return shadow.get(w, "T").t().float().contiguous()

    @staticmethod
    def backward(ctx, g):
        return g


def _linear_any(x, ws, b, compute_dtype, relu, out_dtype):
    from . import linear as _lin
    if compute_dtype == torch.bfloat16:
        if all(w.dim() == 2 and w.shape == ws[0].shape and w.dtype == torch.float32 for w in ws) \
                and (b is None or len(ws) == 1):
            return _linear_padded(x, ws, b, relu, out_dtype)
    elif compute_dtype == torch.float32:
        outs = []
        for w in ws:
            lead = x.shape[:-1]
            y = _MatmulF32.apply(x.reshape(-1, x.shape[-1]).float(), w.float())
            if b is not None and len(ws) == 1:
                y = y + b.float()
            if relu:
                y = torch.relu(y)
            outs.append(y.to(out_dtype).reshape(tuple(lead) + (w.shape[-1],)))
        return outs
    if os.environ.get("LJS_ALLOW_TORCH_FALLBACK", "0") != "1":
        raise NotImplementedError(f"no HIP dense path for compute dtype {compute_dtype}, x {tuple(x.shape)}, "
                                  f"w {[tuple(w.shape) for w in ws]} (LJS_ALLOW_TORCH_FALLBACK=1 to use torch)")
    return [_torch_linear(x, w, b if len(ws) == 1 else None, compute_dtype, relu, out_dtype) for w in ws]


def _linear_padded(x, ws, b, relu, out_dtype):
    """bf16 MFMA dense on operands zero-padded to M, K, N multiples of 8 (autograd flows through
    the pads and slices, so the gradients of x, w and b are those of the unpadded layer)."""
    from . import linear as _lin
    K, N = ws[0].shape
    lead = x.shape[:-1]
    x2 = x.reshape(-1, K)
    M = x2.shape[0]
    pm, pk, pn = (-M) % 8, (-K) % 8, (-N) % 8
    xp = torch.nn.functional.pad(x2, (0, pk, 0, pm)) if (pk or pm) else x2
    wps = [torch.nn.functional.pad(w, (0, pn, 0, pk)).contiguous() if (pk or pn) else w.contiguous() for w in ws]
    bp = torch.nn.functional.pad(b, (0, pn)) if (b is not None and pn) else b
    outs = _lin.linear(xp, wps, bp, relu, out_dtype)
    return [o[:M, :N].reshape(tuple(lead) + (N,)) for o in outs]


class _MatmulF32(torch.autograd.Function):
    """``x [M, K] @ w [K, N]`` in f32 on the MFMA f32 GEMM; backward dx = dy w^T, dw = x^T dy on
    the same kernel through transposed strides (nothing is copied)."""

    @staticmethod
    def forward(ctx, x, w):
        x = x.contiguous()
        w = w.contiguous()
        M, K = x.shape
        N = w.shape[1]
        ctx.save_for_backward(x, w)
        y = torch.empty((M, N), dtype=torch.float32, device=x.device)
        _gemm_f32(x, w, y, M, N, K, K, 1, N, 1, N, 0, 0, 0, 1)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = dy.contiguous().float()
        M, K = x.shape
        N = w.shape[1]
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty((M, K), dtype=torch.float32, device=x.device)
            _gemm_f32(dy, w, dx, M, K, N, N, 1, 1, N, K, 0, 0, 0, 1)       # B[n][k] = w[k][n]
        if ctx.needs_input_grad[1]:
            dw = torch.empty((K, N), dtype=torch.float32, device=x.device)
            _gemm_f32(x, dy, dw, K, N, M, 1, K, N, 1, N, 0, 0, 0, 1)        # A[k][m] = x[m][k]
        return dx, dw


def slab_reduce(slabs: torch.Tensor, out: torch.Tensor, cb: int, out_bs: int, accumulate: bool = False,
                out_bf16: Optional[torch.Tensor] = None, tail: Optional[torch.Tensor] = None,
                tail_bf16: Optional[torch.Tensor] = None, tail_val: float = 0.0) -> None:
    """out = sum over the leading dim of f32 ``slabs`` [S][R][C], written as C/cb column blocks of
    width ``cb`` stored ``out_bs`` floats apart (the split-K combine of the weight-grad GEMMs).
    ``out_bf16`` (same layout as ``out``) also receives the sums rounded to bf16.  ``tail`` (f32,
    and ``tail_bf16``) is filled with the constant ``tail_val`` by the same launch."""
    S, R, C = slabs.shape
    assert slabs.dtype in (torch.float32, torch.bfloat16) and out.dtype == torch.float32 and slabs.is_contiguous()
    assert out_bf16 is None or (out_bf16.dtype == torch.bfloat16 and out_bf16.numel() == out.numel())
    tn = 0
    if tail is not None:
        assert tail.dtype == torch.float32 and tail.is_contiguous() and tail.device == out.device
        assert tail_bf16 is None or (tail_bf16.dtype == torch.bfloat16 and tail_bf16.numel() == tail.numel()
                                     and tail_bf16.is_contiguous())
        tn = tail.numel()
    rc = lib().ljs_slab_reduce(_p(slabs), S, R * C, R, C, _p(out), cb, out_bs, int(accumulate), _p(out_bf16),
                               _p(tail), _p(tail_bf16 if tn else None), tn, float(tail_val),
                               int(slabs.dtype == torch.bfloat16), _stream(out))
    _ck(rc, "slab_reduce")


# ============================================================================ collective pack / unpack
def _pack_launch(srcs, dst: torch.Tensor, A: int, B: int, inner: int, mode: int, perm) -> None:
    arr = (c_void_p * len(srcs))(*[s.data_ptr() for s in srcs])
    pa = (c_int * B)(*[int(p) for p in perm]) if perm is not None else None
    rc = lib().ljs_pack_rows(arr, len(srcs), _p(dst), A, B, inner, mode, pa, _stream(dst))
    _ck(rc, "pack_rows")


def _pack_ok(*ts) -> bool:
    return all(t.is_cuda for t in ts)


def storage_order(t: torch.Tensor):
    """The permutation of ``t``'s dims from outermost to innermost in memory when ``t`` is DENSE
    (a permutation of a contiguous tensor: no gaps, no overlap), else None.  Size-1 dims keep
    their logical position.  Activations whose sharded sequence dim is kept outermost in
    storage (``seq-major``: (batch, seq, features) stored [seq][batch][features]) gather and
    scatter over that dim as whole contiguous blocks - no pack / unpack kernels."""
    if t.dim() == 0:
        return ()
    order = sorted(range(t.dim()), key=lambda d: (-t.stride(d) if t.shape[d] > 1 else 0, d))
    # size-1 dims anywhere: move them to their logical slot (their stride is irrelevant)
    big = [d for d in order if t.shape[d] > 1]
    one = [d for d in range(t.dim()) if t.shape[d] <= 1]
    order = sorted(one + big, key=lambda d: (big.index(d) if d in big else -1, d)) if one else big
    exp = 1
    for d in reversed(big):
        if t.stride(d) != exp:
            return None
        exp *= t.shape[d]
    return tuple(order)


def is_dense(t: torch.Tensor) -> bool:
    return storage_order(t) is not None


def dense(t: torch.Tensor) -> torch.Tensor:
    """``t`` itself when dense (any dim order), else a contiguous copy."""
    return t if is_dense(t) else t.contiguous()


def flat(t: torch.Tensor) -> torch.Tensor:
    """1-D view of a dense tensor's storage (in memory order)."""
    assert is_dense(t), "flat() needs a dense tensor"
    return t.as_strided((t.numel(),), (1,))


def _in_order(t: torch.Tensor):
    """(view of t with dims in storage order - contiguous, the order) for a dense t; else
    (t.contiguous(), identity)."""
    o = storage_order(t)
    if o is None or list(o) == list(range(t.dim())):
        return t.contiguous(), tuple(range(t.dim()))
    return t.permute(o), o


def _inv(order):
    inv = [0] * len(order)
    for i, d in enumerate(order):
        inv[d] = i
    return inv


def rank_major(x: torch.Tensor, dim: int, n: int, perm=None) -> torch.Tensor:
    """[.., n*s (dim), ..] -> [n][.., s, ..], chunk ``perm[k]`` in first-axis slot k (the send
    buffer of a reduce-scatter / all-to-all): dense, the chunks in x's own dim order.  When
    ``dim`` is outermost in x's storage (and no perm) this is a VIEW - no kernel; otherwise one
    HIP launch on GPU tensors."""
    if perm is not None and list(perm) == list(range(n)):
        perm = None
    xs, order = _in_order(x)
    pdim = order.index(dim)
    shp = tuple(xs.shape)
    s = shp[pdim] // n
    pshape = (n,) + shp[:pdim] + (s,) + shp[pdim + 1:]
    back = [0] + [1 + i for i in _inv(order)]
    if all(v == 1 for v in shp[:pdim]) and perm is None:
        return xs.reshape(pshape).permute(back)
    if not _pack_ok(x) or n > 64:
        v = xs.reshape(shp[:pdim] + (n, s) + shp[pdim + 1:]).movedim(pdim, 0)
        return (v[list(perm)] if perm is not None else v).contiguous().permute(back)
    A = math.prod(shp[:pdim])
    inner = xs.element_size() * s * math.prod(shp[pdim + 1:])
    out = torch.empty(pshape, dtype=x.dtype, device=x.device)
    _pack_launch([xs], out, A, n, inner, 0, perm)
    return out.permute(back)


def from_rank_major(buf: torch.Tensor, dim: int, perm=None) -> torch.Tensor:
    """[n][.., c (dim), ..] -> [.., n*c, ..]: slot ``perm[k]`` of ``buf`` becomes chunk k along
    ``dim`` (the receive buffer of an all-gather / all-to-all back in the tensor's layout).  The
    result keeps the chunks' dim order; when ``dim`` is outermost in it (and no perm) it is a
    VIEW of ``buf``."""
    n = buf.shape[0]
    if perm is not None and list(perm) == list(range(n)):
        perm = None
    chunk = buf[0]
    o = storage_order(chunk) if n > 0 else None
    dense_slots = o is not None and buf.stride(0) == chunk.numel()
    if not dense_slots:
        buf, o = buf.contiguous(), tuple(range(buf.dim() - 1))
    pbuf = buf.permute([0] + [1 + d for d in o])
    pdim = list(o).index(dim)
    cs = tuple(pbuf.shape[1:])
    out_shape = cs[:pdim] + (n * cs[pdim],) + cs[pdim + 1:]
    inv = _inv(o)
    if all(v == 1 for v in cs[:pdim]) and perm is None:
        return pbuf.reshape(out_shape).permute(inv)
    if not _pack_ok(buf) or n > 64:
        b = pbuf[list(perm)] if perm is not None else pbuf
        return b.movedim(0, pdim).reshape(out_shape).contiguous().permute(inv)
    A = math.prod(cs[:pdim])
    inner = buf.element_size() * math.prod(cs[pdim:])
    out = torch.empty(out_shape, dtype=buf.dtype, device=buf.device)
    _pack_launch([pbuf], out, A, n, inner, 1, perm)
    return out.permute(inv)


def concat_parts(parts, dim: int) -> torch.Tensor:
    """``torch.cat(parts, dim)`` of same-shape parts on one GPU in one HIP launch (a loopback
    all-gather over virtual devices); the result keeps the parts' dim order when they are dense
    in a common order."""
    p0 = parts[0]
    n = len(parts)
    if not _pack_ok(*parts) or n > 64 or any(p.shape != p0.shape or p.dtype != p0.dtype or p.device != p0.device
                                            for p in parts):
        return torch.cat(parts, dim)
    o = storage_order(p0)
    if o is None or any(storage_order(p) != o or p.stride() != p0.stride() for p in parts):
        parts, o = [p.contiguous() for p in parts], tuple(range(p0.dim()))
    pparts = [p.permute(o) for p in parts]
    pdim = list(o).index(dim)
    cs = tuple(pparts[0].shape)
    A = math.prod(cs[:pdim])
    inner = p0.element_size() * math.prod(cs[pdim:])
    out = torch.empty(cs[:pdim] + (n * cs[pdim],) + cs[pdim + 1:], dtype=p0.dtype, device=p0.device)
    _pack_launch(pparts, out, A, n, inner, 2, None)
    return out.permute(_inv(o))


def pad_box(src: torch.Tensor, full, lo) -> torch.Tensor:
    """A dense tensor of shape ``full`` holding ``src`` at offset ``lo`` and zeros elsewhere, in
    one HIP launch (the backward of a box slice; ``src`` may be strided)."""
    nd = len(full)
    assert src.dim() == nd and src.is_cuda and nd <= 6
    out = torch.empty(tuple(full), dtype=src.dtype, device=src.device)
    arr = lambda v: (c_long * nd)(*[int(x) for x in v])  # noqa: E731
    rc = lib().ljs_pad_box(_p(src), _p(out), nd, arr(full), arr(lo), arr(src.shape), arr(src.stride()),
                           src.element_size(), _stream(out))
    _ck(rc, "pad_box")
    return out


class _BoxSlice(torch.autograd.Function):
    """``t[box]`` whose backward is one :func:`pad_box` launch (torch's slice_backward is a fill
    plus a copy kernel)."""

    @staticmethod
    def forward(ctx, t, box):
        ctx.full = tuple(t.shape)
        ctx.lo = tuple(s.start for s in box)
        return t[box]

    @staticmethod
    def backward(ctx, g):
        return pad_box(g, ctx.full, ctx.lo), None


def box_slice(t: torch.Tensor, box) -> torch.Tensor:
    """``t[box]`` (a tuple of unit-step slices with explicit bounds): on a GPU tensor that needs a
    gradient, the backward runs as one HIP launch."""
    if t.is_cuda and t.requires_grad and torch.is_grad_enabled() and t.dtype.itemsize in (2, 4, 8) \
            and t.dim() <= 6 and len(box) == t.dim():
        return _BoxSlice.apply(t, tuple(box))
    return t[box]


def bcast_scalar(g: torch.Tensor, C: int, R: int, want_db: bool, db_out: Optional[torch.Tensor] = None,
                 db_bf16: Optional[torch.Tensor] = None):
    """(bf16 row [C] filled with bf16(g), f32 [C] = R * bf16(g) or None) from the 1-element
    tensor ``g`` (f32 or bf16), in one launch (``db_out``: where to write the f32 result;
    ``db_bf16``: also write it rounded to bf16)."""
    row = torch.empty((C,), dtype=torch.bfloat16, device=g.device)
    db = (db_out if db_out is not None else torch.empty((C,), dtype=torch.float32, device=g.device)) \
        if want_db else None
    rc = lib().ljs_bcast_scalar(_p(g), int(g.dtype == torch.bfloat16), C, float(R), _p(row), _p(db),
                                _p(db_bf16 if want_db else None), _stream(row))
    _ck(rc, "bcast_scalar")
    return row, db


def relu_bwd_colsum(dy: torch.Tensor, y: torch.Tensor, R: int, C: int):
    """(dy * (y > 0) as a new bf16 [R][C], its f32 column sums [C]) in one pass: the fused ReLU
    backward + bias gradient of a dense layer.  dy / y: bf16 [R][C] views with unit column
    stride (row strides may differ)."""
    masked = torch.empty((R, C), dtype=torch.bfloat16, device=dy.device)
    out = torch.empty((C,), dtype=torch.float32, device=dy.device)
    ws = _workspace(dy.device, "colsum", _COLSUM_WS_BYTES)
    rc = lib().ljs_relu_bwd_colsum(_p(dy), _p(y), R, C, dy.stride(0), y.stride(0), _p(masked), _p(out), _p(ws),
                                   _stream(dy))
    _ck(rc, "relu_bwd_colsum")
    return masked, out


def relu_bwd(dy: torch.Tensor, y: torch.Tensor, R: int, C: int) -> torch.Tensor:
    """dy * (y > 0) as a new bf16 [R][C] (the ReLU backward of a bias-free dense; same view
    requirements as :func:`relu_bwd_colsum`)."""
    masked = torch.empty((R, C), dtype=torch.bfloat16, device=dy.device)
    rc = lib().ljs_relu_bwd(_p(dy), _p(y), R, C, dy.stride(0), y.stride(0), _p(masked), _stream(dy))
    _ck(rc, "relu_bwd")
    return masked


def colsum_ld(t: torch.Tensor, R: int, C: int, ld: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Column sums of an [R][C] matrix with row stride ``ld`` (0 = one repeated row)."""
    acc = out is not None
    if out is None:
        out = torch.empty((C,), dtype=torch.float32, device=t.device)
    ws = _workspace(t.device, "colsum", _COLSUM_WS_BYTES)
    rc = lib().ljs_colsum(_p(t), int(t.dtype == torch.bfloat16), R, C, ld, _p(out), int(acc), _p(ws), _stream(t))
    _ck(rc, "colsum")
    return out


# ============================================================================ attention
def _strides3(t: torch.Tensor):
    # (batch, seq, head) strides of a (b, s, h, d) tensor with d contiguous
    return [t.stride(0), t.stride(1), t.stride(2)]


def _bs_like(shape, ref: torch.Tensor, dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """Empty bf16 (or ``dtype``) (B, S, H, D) stored like ``ref``'s (batch, seq) dims: seq-major when
    ref is (the kernels take any batch / seq strides; the result then gathers / scatters over the
    sequence as contiguous blocks)."""
    B, S, H, D = shape
    if B > 1 and S > 1 and ref.stride(1) > ref.stride(0):
        return torch.empty((S, B, H, D), dtype=dtype, device=ref.device).permute(1, 0, 2, 3)
    return torch.empty(shape, dtype=dtype, device=ref.device)


# ---------------------------------------------------------------------------- the launcher's plan
_ATTN_KINDS = ("fwd", "fwd_acc", "bwd", "bwd_proj", "qkv_fwd")     # ljs_attn_plan's `kind`
_ATTN_ADDRS = ("q", "k", "v", "o", "lse", "dout", "delta", "oacc", "dq", "dk", "dv", "dy", "w")
_ATTN_STRIDES = ("q", "k", "v", "o", "dout", "oacc", "dq", "dk", "dv")


def attn_plan(kind: str, B: int, Sq: int, Sk: int, H: int, *, causal: bool = False, q_offset: int = 0,
              acc_mode: int = 0, strides=None, addrs=None, M: int = 0, dy_ld: int = 0, K: int = 0, N=None, ldx=None,
              cus: int = 256) -> dict:
    """What the attention entry point ``kind`` (fwd, fwd_acc, bwd, bwd_proj, qkv_fwd) would launch
    for a call under the current switches, on a device of ``cus`` compute units (``ljs_attn_plan``:
    the launcher's own plan step; needs the library, not a GPU).  ``strides`` / ``addrs``: dicts of
    (batch, seq, head) strides and addresses by operand name (q, k, v, o, lse, dout, delta, oacc, dq,
    dk, dv, dy, w; qkv_fwd: x, w, qkv, o, lse), the rest dense and 16-byte aligned; ``M`` / ``dy_ld``:
    bwd_proj's; qkv_fwd takes T = B * Sq rows, ``K``, ``N`` (64 H) and ``ldx`` (K).  No rule reads
    ``q_offset``.  Returns ``err``, ``launches`` (the :func:`last_launch` keys name, grid, blocks,
    block, acc_mode of each), ``vst`` (of the argument structs), ``flags32``, ``nw`` and ``nqb``."""
    strides, addrs, order = strides or {}, addrs or {}, _ATTN_ADDRS
    if kind == "qkv_fwd":
        M, dy_ld, order = 64 * H if N is None else N, K if ldx is None else ldx, ("x", "w", "qkv", "o", "lse")
    rows = {"k": Sk, "v": Sk, "dk": Sk, "dv": Sk}
    st = [s for n in _ATTN_STRIDES for s in strides.get(n) or (rows.get(n, Sq) * H * 64, H * 64, 64)]
    ad = (c_void_p * len(order))(*[addrs.get(n, 4096) for n in order])
    out, names = (c_int * 16)(), ctypes.create_string_buffer(96)
    lib().ljs_attn_plan(_ATTN_KINDS.index(kind), B, Sq, Sk, H, int(causal), acc_mode, ad, _longs(st), M, dy_ld, K,
                        cus, out, names, len(names))
    launches = [{"name": n, "grid": (out[3 + 4 * i], out[4 + 4 * i], 1), "blocks": out[3 + 4 * i] * out[4 + 4 * i],
                 "block": out[5 + 4 * i], "acc_mode": None if out[15] < 0 else out[15]}
                for i, n in enumerate(names.value.decode().split())]
    return {"err": out[0], "launches": launches, "vst": (out[10], out[11]), "flags32": out[12], "nw": out[13],
            "nqb": out[14]}


# ---------------------------------------------------------------------------- fused projection
# The Q/K/V projection GEMM of a self-attention block with a 256-token sequence can run the
# attention forward of each (batch, head) in the same kernel (ljs_qkv_attn_fwd): ops/linear.py
# launches it when the model announced the attention that follows (linear.attention_next) and
# leaves (o, lse) here, keyed by the Q/K/V buffer; _Attention.forward takes them when it is called
# with exactly the q / k / v views of that buffer, and runs its own kernel otherwise.
_FUSED_ATTN: Dict[tuple, tuple] = {}


def qkv_attn_fwd(xb: torch.Tensor, wt: torch.Tensor, out: torch.Tensor, H: int, scale: float,
                 trace: Optional[torch.Tensor] = None):
    """out [T][3N] = xb [T][K] . wt[i]^T (wt: [3][N][K] bf16) AND the attention forward of every
    (batch, head) over it (sequence 256): returns (o [T][N] bf16, lse [T/256][H][256] f32).
    ``trace``: int64 [blocks][8][8][4] phase stamps (LJS_QA_TRACE builds only; scripts/qkv_attn_phases.py)."""
    T, K = xb.shape
    N = wt.shape[1]
    assert (xb.dtype == torch.bfloat16 and wt.dtype == torch.bfloat16 and out.dtype == torch.bfloat16
            and xb.stride(1) == 1 and wt.is_contiguous() and out.is_contiguous() and out.shape == (T, 3 * N)
            and wt.shape == (3, N, K) and N == 64 * H and T % 256 == 0 and K % 128 == 0)
    o = torch.empty((T, N), dtype=torch.bfloat16, device=xb.device)
    lse = torch.empty((T // 256, H, 256), dtype=torch.float32, device=xb.device)
    _ck(lib().ljs_qkv_attn_fwd(_p(xb), xb.stride(0), _p(wt), _p(out), _p(o), _p(lse), T, K, N, H, float(scale),
                               _p(trace) if trace is not None else None, _stream(xb)), "ljs_qkv_attn_fwd")
    return o, lse


def _fused_key(t: torch.Tensor, scale: float):
    return (t.data_ptr(), t._version, t.device.index, float(scale))


def clear_fused_attention() -> None:
    """Drop a fused forward nobody took (also run when a graph capture ends)."""
    _FUSED_ATTN.clear()


def register_fused_attention(out: torch.Tensor, o: torch.Tensor, lse: torch.Tensor, H: int, scale: float) -> None:
    from ..spmd import graphs as _graphs
    if clear_fused_attention not in _graphs.AFTER_CAPTURE:
        _graphs.AFTER_CAPTURE.append(clear_fused_attention)
    _FUSED_ATTN.clear()   # one pending forward at a time
    _FUSED_ATTN[_fused_key(out, scale)] = (o, lse, tuple(out.shape), H)


def _take_fused_attention(q, k, v, scale, causal, q_offset):
    if not _FUSED_ATTN or causal or q_offset or k.shape[2] != q.shape[2]:
        return None
    ent = _FUSED_ATTN.get(_fused_key(q, scale))
    if ent is None:
        return None
    o, lse, (T, N3), H = ent
    N = N3 // 3
    B, S = T // 256, 256
    es = q.element_size()
    if not (q.shape == (B, S, H, 64) and k.shape == q.shape and v.shape == q.shape
            and q.stride() == (S * N3, N3, 64, 1) and k.stride() == q.stride() and v.stride() == q.stride()
            and k.data_ptr() == q.data_ptr() + N * es and v.data_ptr() == q.data_ptr() + 2 * N * es):
        return None
    del _FUSED_ATTN[_fused_key(q, scale)]
    FUSED_ATTN_STATS["taken"] += 1
    return o.view(B, S, H, 64), lse


FUSED_ATTN_STATS = {"taken": 0}


# ---------------------------------------------------------------------------- out-projection dX hand-over
# The out-projection's input gradient dO = dY . Wo^T has one consumer, the attention backward, which
# slices it per (batch, head).  ops/linear.py's _Linear.backward, when the pre-backward graph walk
# proved that nothing but that attention backward reads it (linear.proj_safe_nodes), does not launch
# the GEMM: it returns the unwritten buffer and leaves (dY, ld, weight shadow) here, keyed by the
# buffer.  _Attention.backward takes the entry when its cotangent IS that buffer and the kernel's
# gate holds (ljs_attn_bwd_proj: dO is never materialised); anything else launches the GEMM first.
# Entries nobody took are materialised when the backward, or a capture segment, ends.
_PROJ_PENDING: Dict[int, tuple] = {}
ATTN_BWD_PROJ_STATS = {"taken": 0, "materialised": 0}


def proj_shape_ok(B: int, Sq: int, Sk: int, H: int, D: int, M: int, dy_ld: int, causal: bool) -> bool:
    """ljs_attn_bwd_proj's gate for dense, aligned operands of this shape under the current switches
    (the head_dim is fixed in the library, so that one test is made here)."""
    return D == 64 and attn_plan("bwd_proj", B, Sq, Sk, H, causal=causal, M=M, dy_ld=dy_ld)["err"] == 0


def attn_bwd_proj_ok(q, k, v, o, dy: torch.Tensor, dy_ld: int, w: torch.Tensor, causal: bool, outs=None) -> bool:
    """Whether ljs_attn_bwd_proj accepts these operands (and the outputs ``outs`` = (dq, dk, dv), else
    dense ones): the entry point's own gate (attn_bwd_proj_plan, the switches included) asked through
    the plan, and here only what the library cannot see -- dtypes, a contiguous head_dim and weight."""
    B, Sq, H, D = q.shape
    ts = dict(zip(("q", "k", "v", "o", "dq", "dk", "dv"), (q, k, v, o) + tuple(outs or ())))
    if k.shape[2] != H or v.shape[2] != H:   # (the kernel is multi-head only: one K/V head per query head)
        return False
    if not (D == 64 and w.shape[0] == H * D and dy.dtype == torch.bfloat16 and w.dtype == torch.bfloat16
            and w.is_contiguous() and all(t.dtype == torch.bfloat16 and t.stride(3) == 1 for t in ts.values())):
        return False
    addrs = {n: t.data_ptr() for n, t in ts.items()}
    addrs.update(dy=dy.data_ptr(), w=w.data_ptr())
    return attn_plan("bwd_proj", B, Sq, k.shape[1], H, causal=causal, M=w.shape[1], dy_ld=dy_ld, addrs=addrs,
                     strides={n: _strides3(t) for n, t in ts.items()})["err"] == 0


def attn_bwd_proj_block(q, k, v, o, dy: torch.Tensor, dy_ld: int, w: torch.Tensor, lse, scale: float,
                        causal: bool = False, outs=None):
    """The fused backward with dO = dy . w^T formed inside the kernel: ``dy`` the [B * 256][M] bf16
    rows of the out-projection's cotangent (row stride ``dy_ld``; 0 = one row for every token), ``w``
    the [H * 64][M] bf16 weight.  Returns (dq, dk, dv) bf16; raises when the entry point's gate
    refuses (nothing is launched then)."""
    B, Sq, H, D = q.shape
    if outs is None:
        outs = tuple(torch.empty((B, Sq, H, D), dtype=torch.bfloat16, device=q.device) for _ in range(3))
    dq, dk, dv = outs
    rc = lib().ljs_attn_bwd_proj(_p(q), _p(k), _p(v), _p(o), _p(dy), int(dy_ld), _p(w), int(w.shape[1]), _p(lse),
                                 _p(dq), _p(dk), _p(dv), B, Sq, k.shape[1], H, _longs(_strides3(q)),
                                 _longs(_strides3(k)), _longs(_strides3(v)), _longs(_strides3(o)),
                                 _longs(_strides3(dq)), _longs(_strides3(dk)), _longs(_strides3(dv)), float(scale),
                                 int(causal), _stream(q))
    _ck(rc, "ljs_attn_bwd_proj")
    return dq, dk, dv


def attn_bwd_proj_last_path() -> int:
    """Which GEMM phase the last ``attn_bwd_proj`` launch ran: 0 the general one, 1 the broadcast-row
    one (``dy_ld`` 0, ``M`` <= 2048 -- the row copy's size in LDS; a wider broadcast row runs the general
    phase -- and ``LJS_ATTN_BWD_PROJ_BCAST`` not 0); -1 before any launch.  The launch record is the same
    for both."""
    return lib().ljs_attn_bwd_proj_last_path()


def defer_out_proj(dy: torch.Tensor, ld: int, wn: torch.Tensor, dx: torch.Tensor, launch) -> None:
    """Leave the out-projection's dX GEMM (``launch()`` writes ``dx`` [T][H * 64] = dy . wn^T) to the
    attention backward that consumes ``dx``."""
    from ..spmd import graphs as _graphs
    if materialise_out_proj not in _graphs.BEFORE_CUT:
        _graphs.BEFORE_CUT.append(materialise_out_proj)
        _graphs.AFTER_CAPTURE.append(materialise_out_proj)
    _PROJ_PENDING[dx.data_ptr()] = (dy, ld, wn, dx, launch)


def materialise_out_proj() -> None:
    """Launch the dX GEMM of every hand-over nobody took."""
    while _PROJ_PENDING:
        _, ent = _PROJ_PENDING.popitem()
        ent[4]()
        ATTN_BWD_PROJ_STATS["materialised"] += 1


def _take_out_proj(do: torch.Tensor, q, k, v, o, outs, causal):
    """The pending hand-over whose buffer ``do`` is, if the fused kernel can run it; a pending entry
    it cannot run is materialised (``do`` is then an ordinary cotangent)."""
    ent = _PROJ_PENDING.pop(do.data_ptr(), None)
    if ent is None:
        return None
    dy, ld, wn, dx, launch = ent
    B, Sq, H, D = q.shape
    if (do.dtype == torch.bfloat16 and tuple(do.shape) == (B, Sq, H, D) and do.is_contiguous()
            and dx.numel() == do.numel() and attn_bwd_proj_ok(q, k, v, o, dy, ld, wn, causal, outs)):
        ATTN_BWD_PROJ_STATS["taken"] += 1
        return dy, ld, wn
    launch()
    ATTN_BWD_PROJ_STATS["materialised"] += 1
    return None


# ---------------------------------------------------------------------------- grouped-query attention
# k / v of (B, Sk, Hkv, 64) with H % Hkv == 0: query head h reads key/value head h // (H // Hkv) inside
# the kernels (ljs_attn_*_gqa); the backward kernels then write per-query-head dK / dV into a scratch
# pair that gqa_reduce folds over each group.  Hkv == H runs the multi-head entry points unchanged.
def _kv_heads(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor) -> int:
    """The key/value head count of a call (``q`` (B, Sq, H, D), ``k`` / ``v`` (B, Sk, Hkv, D)); raises
    a ValueError naming both counts where k's and v's differ or do not divide H."""
    from .kernels import kv_groups
    return q.shape[2] // kv_groups(q, k, v)


def gqa_kernels() -> bool:
    """``LJS_GQA_KERNELS=0`` (A/B, read at every call): grouped-query attention expands K / V to one head
    per query head in torch and runs the multi-head path, autograd summing dK / dV over each group --
    the baseline of scripts/gqa_probe.py."""
    # LJS_GQA_KERNELS=0: K / V of a grouped-query attention are expanded per query head in torch in front
    # of the multi-head kernels (autograd sums dK / dV); default: the kernels look the K/V head up
    return os.environ.get("LJS_GQA_KERNELS", "1") != "0"


def set_gqa_max_blocks(n: Optional[int]) -> None:
    """Cap ``gqa_reduce``'s grid at ``n`` blocks (tests: the grid-stride loop on small shapes); None or
    0 restores the default."""
    lib().ljs_gqa_set_max_blocks(int(n or 0))


def gqa_reduce_raw(dkx, dvx, dk, dv) -> int:
    """``ljs_gqa_reduce``'s return code: dk / dv (B, Sk, Hkv, 64) = the sum of dkx / dvx (B, Sk, H, 64)
    over each group of H // Hkv adjacent heads, f32 adds in ascending order and one rounding to bf16."""
    B, Sk, H, _ = dkx.shape
    return lib().ljs_gqa_reduce(_p(dkx), _p(dvx), _p(dk), _p(dv), B, Sk, H, dk.shape[2], _longs(_strides3(dkx)),
                                _longs(_strides3(dvx)), _longs(_strides3(dk)), _longs(_strides3(dv)), _stream(dkx))


def gqa_reduce(dkx: torch.Tensor, dvx: torch.Tensor, dk: torch.Tensor, dv: torch.Tensor):
    """Fold the per-query-head gradients ``dkx`` / ``dvx`` into ``dk`` / ``dv`` (one launch for both)."""
    ok = all(t.dtype == torch.bfloat16 and t.shape[-1] == 64 and t.stride(3) == 1 for t in (dkx, dvx, dk, dv))
    if not (ok and dkx.shape == dvx.shape and dk.shape == dv.shape and dk.shape[:2] == dkx.shape[:2]):
        raise ValueError(f"gqa_reduce: bf16 (B, Sk, H, 64) -> (B, Sk, Hkv, 64) expected; got {tuple(dkx.shape)}, "
                         f"{tuple(dvx.shape)} -> {tuple(dk.shape)}, {tuple(dv.shape)}")
    _ck(gqa_reduce_raw(dkx, dvx, dk, dv), "ljs_gqa_reduce")
    return dk, dv


def _attn_fwd_call(q, k, v, o, lse, scale, causal, q_offset):
    """ljs_attn_fwd into ``o`` (bf16 [B, Sq, H, 64]) and ``lse`` (f32 [B, H, Sq]); returns both."""
    B, Sq, H, _ = q.shape
    Hkv = _kv_heads(q, k, v)
    if Hkv != H:
        _ck(lib().ljs_attn_fwd_gqa(_p(q), _p(k), _p(v), _p(o), _p(lse), B, Sq, k.shape[1], H, Hkv,
                                   _longs(_strides3(q)), _longs(_strides3(k)), _longs(_strides3(v)),
                                   _longs(_strides3(o)), scale, int(causal), q_offset, _stream(q)), "ljs_attn_fwd_gqa")
        return o, lse
    _ck(lib().ljs_attn_fwd(_p(q), _p(k), _p(v), _p(o), _p(lse), B, Sq, k.shape[1], H, _longs(_strides3(q)),
                           _longs(_strides3(k)), _longs(_strides3(v)), _longs(_strides3(o)), scale, int(causal),
                           q_offset, _stream(q)), "ljs_attn_fwd")
    return o, lse


def _lse_like(q: torch.Tensor) -> torch.Tensor:
    return torch.empty((q.shape[0], q.shape[2], q.shape[1]), dtype=torch.float32, device=q.device)


def _bf16_rows(do: torch.Tensor) -> torch.Tensor:
    """The cotangent as the backward kernels read it: bf16 with a contiguous head_dim."""
    do = do.to(torch.bfloat16)
    return do if do.stride(3) == 1 else do.contiguous()


def _attn_bwd_call(q, k, v, o, do, lse, dq, dk, dv, scale, causal, q_offset):
    """ljs_attn_bwd into dq / dk / dv (``do`` as _bf16_rows gives it); allocates the delta workspace.
    With fewer key/value heads than query heads (dk / dv of Hkv heads) the kernels write per-query-head
    gradients into a scratch pair, allocated here like any other intermediate (inside a graph capture
    it belongs to the graph's pool, so a replay reuses the same addresses), and gqa_reduce folds them
    into dk / dv on the same stream."""
    B, Sq, H, _ = q.shape
    delta = torch.empty((B, H, Sq), dtype=torch.float32, device=q.device)
    Hkv = _kv_heads(q, k, v)
    if Hkv != H:
        Sk = k.shape[1]
        dkx = torch.empty((B, Sk, H, 64), dtype=torch.bfloat16, device=q.device)
        dvx = torch.empty((B, Sk, H, 64), dtype=torch.bfloat16, device=q.device)
        _ck(lib().ljs_attn_bwd_gqa(_p(q), _p(k), _p(v), _p(o), _p(do), _p(lse), _p(delta), _p(dq), _p(dkx), _p(dvx),
                                   B, Sq, Sk, H, Hkv, _longs(_strides3(q)), _longs(_strides3(k)),
                                   _longs(_strides3(v)), _longs(_strides3(o)), _longs(_strides3(do)),
                                   _longs(_strides3(dq)), _longs(_strides3(dkx)), _longs(_strides3(dvx)), scale,
                                   int(causal), q_offset, _stream(q)), "ljs_attn_bwd_gqa")
        gqa_reduce(dkx, dvx, dk, dv)
        return
    _ck(lib().ljs_attn_bwd(_p(q), _p(k), _p(v), _p(o), _p(do), _p(lse), _p(delta), _p(dq), _p(dk), _p(dv), B, Sq,
                           k.shape[1], H, _longs(_strides3(q)), _longs(_strides3(k)), _longs(_strides3(v)),
                           _longs(_strides3(o)), _longs(_strides3(do)), _longs(_strides3(dq)), _longs(_strides3(dk)),
                           _longs(_strides3(dv)), scale, int(causal), q_offset, _stream(q)), "ljs_attn_bwd")


class _Attention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, scale, causal, q_offset):
        pre = _take_fused_attention(q, k, v, scale, causal, q_offset)
        if pre is not None:
            o, lse = pre
        else:
            o, lse = _attn_fwd_call(q, k, v, _bs_like(q.shape, q), _lse_like(q), scale, causal, q_offset)
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.args = (scale, causal, q_offset)
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse = ctx.saved_tensors
        scale, causal, q_offset = ctx.args
        B, Sq, H, D = q.shape
        Sk = k.shape[1]
        do = _bf16_rows(do)
        st = q.stride()
        fused = (Sq == Sk and k.stride() == st and v.stride() == st and st[3] == 1 and st[2] == D
                 and k.data_ptr() - q.data_ptr() == H * D * 2 and v.data_ptr() - q.data_ptr() == 2 * H * D * 2
                 and st[1] == 3 * H * D and st[0] == Sq * st[1])
        Hkv = k.shape[2]
        sk = k.stride()
        if fused and Hkv == H:
            # q/k/v are column blocks of one fused-QKV buffer: write dq/dk/dv the same way so the
            # dense backward sees one [M, 3*H*D] gradient and runs ONE batched weight-grad GEMM
            dqkv = torch.empty((B, Sq, 3, H, D), dtype=torch.bfloat16, device=q.device)
            dq, dk, dv = dqkv[:, :, 0], dqkv[:, :, 1], dqkv[:, :, 2]
        elif (Hkv != H and v.stride() == sk and sk[3] == 1 and sk[2] == D and sk[1] == 2 * Hkv * D
              and sk[0] == Sk * sk[1] and v.data_ptr() - k.data_ptr() == Hkv * D * 2):
            # grouped-query attention with k / v the two column blocks of one [T][2 Hkv D] buffer (the fused
            # K | V projection): dk / dv are the same column blocks of one fresh buffer, the adjacency
            # linear._wgrads looks for, so the projection's weight gradient is one batched launch
            dq = _bs_like((B, Sq, H, D), q)
            dkv = torch.empty((B, Sk, 2, Hkv, D), dtype=torch.bfloat16, device=q.device)
            dk, dv = dkv[:, :, 0], dkv[:, :, 1]
        else:
            dq = _bs_like((B, Sq, H, D), q)
            dk = _bs_like((B, Sk, Hkv, D), k)
            dv = _bs_like((B, Sk, Hkv, D), v)
        proj = _take_out_proj(do, q, k, v, o, (dq, dk, dv), causal) if _PROJ_PENDING else None
        if proj is not None:
            attn_bwd_proj_block(q, k, v, o, proj[0], proj[1], proj[2], lse, scale, causal, outs=(dq, dk, dv))
        else:
            _attn_bwd_call(q, k, v, o, do, lse, dq, dk, dv, scale, causal, q_offset)
        return dq.to(q.dtype), dk.to(k.dtype), dv.to(v.dtype), None, None, None


def attn_fwd_lse(q, k, v, scale: float, causal: bool = False, q_offset: int = 0):
    """Raw flash forward of one (q block, kv block) pair: (o bf16 [B,Sq,H,D], lse f32 [B,H,Sq]).
    lse is log2 of the scaled-score partition function; +inf marks rows with no unmasked key.
    k / v are (B, Sk, Hkv, D) with H % Hkv == 0 (grouped-query attention), here and in attn_fwd_acc,
    attn_bwd_block (dk / dv of Hkv heads) and attention."""
    o = torch.empty(q.shape, dtype=torch.bfloat16, device=q.device)
    return _attn_fwd_call(q, k, v, o, _lse_like(q), scale, causal, q_offset)


def attn_fwd_acc(q, k, v, scale: float, causal: bool, q_offset: int, oacc: torch.Tensor, lse: torch.Tensor, mode: int,
                 out: Optional[torch.Tensor] = None):
    """One key block of a blockwise (ring) forward merged INTO the running result in the kernel's
    epilogue: mode 1 starts (f32 ``oacc`` [B,Sq,H,D] + ``lse``), 2 merges by log-sum-exp, 3 merges
    and writes the final bf16 ``out`` (returned).  No per-hop torch merge kernels."""
    B, Sq, H, D = q.shape
    Sk = k.shape[1]
    assert oacc.dtype == torch.float32 and oacc.stride(3) == 1 and lse.dtype == torch.float32
    if mode == 3 and out is None:
        out = _bs_like((B, Sq, H, D), q)
    o = out if out is not None else q   # (unused unless mode 3)
    Hkv = _kv_heads(q, k, v)
    if Hkv != H:
        rc = lib().ljs_attn_fwd_acc_gqa(_p(q), _p(k), _p(v), _p(o), _p(lse), B, Sq, Sk, H, Hkv, _longs(_strides3(q)),
                                        _longs(_strides3(k)), _longs(_strides3(v)), _longs(_strides3(o)), scale,
                                        int(causal), q_offset, _p(oacc), _longs(_strides3(oacc)), int(mode),
                                        _stream(q))
        _ck(rc, "ljs_attn_fwd_acc_gqa")
        return out
    rc = lib().ljs_attn_fwd_acc(_p(q), _p(k), _p(v), _p(o), _p(lse), B, Sq, Sk, H, _longs(_strides3(q)),
                                _longs(_strides3(k)), _longs(_strides3(v)), _longs(_strides3(o)), scale, int(causal),
                                q_offset, _p(oacc), _longs(_strides3(oacc)), int(mode), _stream(q))
    _ck(rc, "ljs_attn_fwd_acc")
    return out


def attn_bwd_block(q, k, v, o, do, lse, scale: float, causal: bool = False, q_offset: int = 0):
    """Raw flash backward of one kv block given the FINAL output ``o`` and GLOBAL ``lse``
    (blockwise-separable): returns this block's (dq, dk, dv) contributions in bf16."""
    B, Sq, H, D = q.shape
    Sk = k.shape[1]
    dq = torch.empty((B, Sq, H, D), dtype=torch.bfloat16, device=q.device)
    dk = torch.empty((B, Sk, k.shape[2], D), dtype=torch.bfloat16, device=q.device)
    dv = torch.empty((B, Sk, v.shape[2], D), dtype=torch.bfloat16, device=q.device)
    _attn_bwd_call(q, k, v, o, _bf16_rows(do), lse, dq, dk, dv, scale, causal, q_offset)
    return dq, dk, dv


def attention(q, k, v, scale: float, causal: bool = False, q_offset: int = 0) -> torch.Tensor:
    ok = (q.shape[-1] == 64 and k.shape[-1] == 64 and v.shape[-1] == 64 and q.stride(-1) == 1
          and k.stride(-1) == 1 and v.stride(-1) == 1)
    if not ok:
        raise NotImplementedError(f"HIP attention supports head_dim 64 with contiguous head_dim; got {q.shape}")
    qb, kb, vb = (t if t.dtype == torch.bfloat16 else t.to(torch.bfloat16) for t in (q, k, v))
    Hkv = _kv_heads(q, k, v)
    if Hkv != q.shape[2] and not gqa_kernels():
        from .kernels import expand_kv
        kb, vb = expand_kv(kb, q.shape[2] // Hkv), expand_kv(vb, q.shape[2] // Hkv)
    out = _Attention.apply(qb, kb, vb, float(scale), bool(causal), int(q_offset))
    return out if v.dtype == torch.bfloat16 else out.to(v.dtype)


# ============================================================================ KV cache / decode
# csrc/kernels/decode.hip: the cache append (with the rotary embedding at a position read on the
# device) and single-query split-K attention over the cache.  Nothing here takes a gradient.
def set_decode_splits(n: Optional[int], keys: int = 0) -> None:
    """Tests: force ``attn_decode``'s plan to ``n`` splits of ``keys`` keys (a multiple of
    :func:`decode_key_tile`, ``n * keys >= cap``); None or 0 restores :func:`plan_decode`."""
    lib().ljs_decode_set_splits(int(n or 0), int(keys))


def decode_key_tile() -> int:
    """Keys one block of the decode kernel holds per step: ``keys_per_split`` is a multiple of it."""
    return lib().ljs_decode_key_tile()


def decode_max_group() -> int:
    """The largest ``heads // kv_heads`` the decode kernel takes."""
    return lib().ljs_decode_max_group()


def plan_decode(B: int, Hkv: int, cap: int, cus: Optional[int] = None):
    """``(splits, keys_per_split)`` of ``attn_decode`` for ``B`` sequences, ``Hkv`` key/value heads and a
    cache of ``cap`` rows on a device of ``cus`` compute units (default: the current device's).  Pure:
    it depends on nothing else, the lengths least of all, so a captured launch stays valid."""
    out = (c_int * 2)()
    rc = lib().ljs_decode_plan(int(B), int(Hkv), int(cap), int(cus if cus is not None else _cus()), out)
    if rc != 0:
        raise ValueError(f"plan_decode: B={B}, Hkv={Hkv}, cap={cap}, cus={cus} must all be positive")
    return int(out[0]), int(out[1])


def _decode_launch_plan(B: int, Hkv: int, cap: int):
    out = (c_int * 2)()
    _ck(lib().ljs_decode_launch_plan(int(B), int(Hkv), int(cap), out), "ljs_decode_launch_plan")
    return int(out[0]), int(out[1])


def decode_supported(*ts: torch.Tensor) -> bool:
    """Whether decode.hip takes these operands as they are: bf16 ``(B, S, H, 64)`` GPU tensors, the head
    dim contiguous, the base and the three outer strides 16-byte aligned."""
    return all(t.is_cuda and t.dim() == 4 and t.dtype == torch.bfloat16 and t.shape[-1] == 64 and t.numel()
               and t.stride(-1) == 1 and t.data_ptr() % 16 == 0 and all(t.stride(i) % 8 == 0 for i in range(3))
               for t in ts)


def _lens_ok(lens: Optional[torch.Tensor], B: int) -> bool:
    return lens is None or (lens.is_cuda and lens.dtype == torch.int32 and lens.shape == (B,) and lens.is_contiguous())


def kv_append_raw(k, v, kc, vc, lens=None, q=None, q_out=None, cos=None, sin=None) -> int:
    """One ``ljs_kv_append`` launch on the tensors as they are; returns the launcher's code (non-zero:
    rejected, nothing launched) instead of raising."""
    B, T, Hkv, _ = k.shape
    st = lambda t: _longs(_strides3(t)) if t is not None else None   # noqa: E731
    return lib().ljs_kv_append(_p(k), _p(v), _p(q), _p(kc), _p(vc), _p(q_out), B, T, q.shape[2] if q is not None else 0,
                               Hkv, kc.shape[1], st(k), st(v), st(q), st(kc), st(vc), st(q_out), _p(lens), _p(cos),
                               _p(sin), cos.shape[0] if cos is not None else 0, _stream(k))


def kv_append(k, v, kc, vc, lens=None, q=None, theta: Optional[float] = None):
    """``vc[b, p] = v[b, t]`` and ``kc[b, p] = k[b, t]`` for ``p = base[b] + t``, ``base = lens`` (int32 ``[B]`` on
    the device) or 0 without it; with ``theta`` k is rotated by the rotary embedding at position ``p`` on
    its way (rope.hip's bits), and a ``q`` is rotated the same way into the returned tensor.  Rows with
    ``p >= cap`` are not written.  One launch."""
    B = k.shape[0]
    ok = decode_supported(k, v, kc, vc) and (q is None or decode_supported(q)) and _lens_ok(lens, B) \
        and k.shape == v.shape and kc.shape == vc.shape and kc.shape[0] == B and kc.shape[2] == k.shape[2] \
        and (q is None or (theta is not None and q.shape[:2] == k.shape[:2]))
    if not ok:
        raise NotImplementedError(f"kv_append kernel: bf16 (B, T, H, 64) operands with 16-byte aligned bases and "
                                  f"strides and an int32 [B] lens; got k {k.dtype} {tuple(k.shape)} strides "
                                  f"{k.stride()}, cache {kc.dtype} {tuple(kc.shape)} strides {kc.stride()}")
    cos = sin = q_out = None
    if theta is not None:
        from .kernels import rope_table
        cos, sin = rope_table(k.device, 64, theta, kc.shape[1])
    if q is not None:
        q_out = torch.empty(q.shape, dtype=q.dtype, device=q.device)
    _ck(kv_append_raw(k, v, kc, vc, lens, q, q_out, cos, sin), "ljs_kv_append")
    return q_out


def _decode_ws(dev: torch.device, floats: int) -> torch.Tensor:
    """The per-device f32 workspace of the split partials.  It grows outside a capture only: a graph
    holds its address."""
    key = (dev.index, "decode")
    t = _WS.get(key)
    if t is None or t.numel() < floats:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"attn_decode: the split workspace on {dev} has {0 if t is None else t.numel()} floats "
                               f"and {floats} are needed, and it cannot be created during a graph capture: run the "
                               "function once outside the capture first")
        if t is not None:
            _WS[(dev.index, "decode", t.data_ptr())] = t     # a captured graph may still write into it
        t = torch.empty(max(floats, 1 << 16), dtype=torch.float32, device=dev)
        _WS[key] = t
    return t


def attn_decode_raw(q, kc, vc, o, lse, ws, lens, scale: float, extra: int = 1) -> int:
    """One ``ljs_attn_decode`` call (the decode launch, and the merge launch when the plan has more than
    one split) on the tensors as they are; returns the launcher's code instead of raising."""
    B, _, H, _ = q.shape
    return lib().ljs_attn_decode(_p(q), _p(kc), _p(vc), _p(o), _p(lse), _p(ws), ws.numel() if ws is not None else 0,
                                 _p(lens), B, H, kc.shape[2], kc.shape[1], _longs(_strides3(q)),
                                 _longs(_strides3(kc)), _longs(_strides3(vc)), _longs(_strides3(o)), float(scale),
                                 int(extra), _stream(q))


def attn_decode(q, kc, vc, lens, scale: float, extra: int = 1):
    """Single-query attention of ``q`` (B, 1, H, 64) over rows ``[0, min(lens[b] + extra, cap))`` of the caches
    ``kc`` / ``vc`` (B, cap, Hkv, 64): ``(o`` bf16 (B, 1, H, 64), ``lse2`` f32 (B, H, 1)``)``; a sequence without
    keys gets ``o = 0``, ``lse2 = +inf``."""
    B, T, H, _ = q.shape
    Hkv = kc.shape[2]
    ok = decode_supported(q, kc, vc) and T == 1 and kc.shape == vc.shape and kc.shape[0] == B and lens is not None \
        and _lens_ok(lens, B) and H % Hkv == 0 and H // Hkv <= decode_max_group() and scale > 0
    if not ok:
        raise NotImplementedError(f"attn_decode kernel: bf16 q (B, 1, H, 64) and caches (B, cap, Hkv, 64) with 16-byte "
                                  f"aligned bases and strides, H / Hkv <= {decode_max_group()}, int32 [B] lens; got q "
                                  f"{q.dtype} {tuple(q.shape)}, cache {kc.dtype} {tuple(kc.shape)} strides {kc.stride()}")
    splits, _ = _decode_launch_plan(B, Hkv, kc.shape[1])
    ws = _decode_ws(q.device, B * H * splits * lib().ljs_decode_part_floats()) if splits > 1 else None
    o = torch.empty((B, 1, H, 64), dtype=torch.bfloat16, device=q.device)
    lse = torch.empty((B, H, 1), dtype=torch.float32, device=q.device)
    _ck(attn_decode_raw(q, kc, vc, o, lse, ws, lens, scale, extra), "ljs_attn_decode")
    return o, lse


# ---- the MX-fp8 cache: e4m3 bytes (B, cap, Hkv, 64) and e8m0 scale bytes (B, cap, Hkv, 2), both uint8
def decode_q8_supported(*ts: torch.Tensor) -> bool:
    """Whether decode.hip takes these MX-fp8 cache buffers as they are: uint8 ``(B, S, H, 64)`` GPU tensors (e4m3
    bytes), the head dim contiguous, the base and the three outer strides multiples of 16 bytes."""
    return all(t.is_cuda and t.dim() == 4 and t.dtype == torch.uint8 and t.shape[-1] == 64 and t.numel()
               and t.stride(-1) == 1 and t.data_ptr() % 16 == 0 and all(t.stride(i) % 16 == 0 for i in range(3))
               for t in ts)


def decode_scale_supported(*ts: torch.Tensor) -> bool:
    """Whether decode.hip takes these e8m0 scale buffers as they are: uint8 ``(B, S, H, 2)`` GPU tensors, the
    last dim contiguous, the base and the three outer strides even (one 2-byte store writes a row's two)."""
    return all(t.is_cuda and t.dim() == 4 and t.dtype == torch.uint8 and t.shape[-1] == 2 and t.numel()
               and t.stride(-1) == 1 and t.data_ptr() % 2 == 0 and all(t.stride(i) % 2 == 0 for i in range(3))
               for t in ts)


def _q8_cache_ok(kc, vc, kcs, vcs) -> bool:
    return decode_q8_supported(kc, vc) and decode_scale_supported(kcs, vcs) and kc.shape == vc.shape \
        and kcs.shape == vcs.shape == kc.shape[:3] + (2,)


def kv_append_q8_raw(k, v, kc, vc, kcs, vcs, lens=None, q=None, q_out=None, cos=None, sin=None) -> int:
    """One ``ljs_kv_append_q8`` launch on the tensors as they are; returns the launcher's code (non-zero:
    rejected, nothing launched) instead of raising."""
    B, T, Hkv, _ = k.shape
    st = lambda t: _longs(_strides3(t)) if t is not None else None   # noqa: E731
    return lib().ljs_kv_append_q8(_p(k), _p(v), _p(q), _p(kc), _p(vc), _p(kcs), _p(vcs), _p(q_out), B, T,
                                  q.shape[2] if q is not None else 0, Hkv, kc.shape[1], st(k), st(v), st(q), st(kc),
                                  st(vc), st(kcs), st(vcs), st(q_out), _p(lens), _p(cos), _p(sin),
                                  cos.shape[0] if cos is not None else 0, _stream(k))


def kv_append_q8(k, v, kc, vc, kcs, vcs, lens=None, q=None, theta: Optional[float] = None):
    """:func:`kv_append` into an MX-fp8 cache: the row :func:`kv_append` would store at ``p`` (k rotated with
    ``theta``: rope.hip's bits; v as it is) goes through ``fp8.quantize_mx_ref``'s rule into 64 e4m3 bytes of ``kc``
    / ``vc`` and two e8m0 bytes of ``kcs`` / ``vcs`` (uint8 ``(B, cap, Hkv, 64)`` and ``(B, cap, Hkv, 2)``); rows with
    ``p >= cap`` write neither.  Returns the rotated ``q`` in bf16, as :func:`kv_append` does.  One launch."""
    B = k.shape[0]
    ok = decode_supported(k, v) and (q is None or decode_supported(q)) and _lens_ok(lens, B) \
        and _q8_cache_ok(kc, vc, kcs, vcs) and k.shape == v.shape and kc.shape[0] == B \
        and kc.shape[2] == k.shape[2] and (q is None or (theta is not None and q.shape[:2] == k.shape[:2]))
    if not ok:
        raise NotImplementedError(f"kv_append_q8 kernel: bf16 (B, T, H, 64) k / v / q, uint8 (B, cap, Hkv, 64) caches "
                                  f"with 16-byte aligned bases and strides, uint8 (B, cap, Hkv, 2) scales with even "
                                  f"strides and an int32 [B] lens; got k {k.dtype} {tuple(k.shape)} strides {k.stride()}, "
                                  f"cache {kc.dtype} {tuple(kc.shape)} strides {kc.stride()}, scales {kcs.dtype} "
                                  f"{tuple(kcs.shape)} strides {kcs.stride()}")
    cos = sin = q_out = None
    if theta is not None:
        from .kernels import rope_table
        cos, sin = rope_table(k.device, 64, theta, kc.shape[1])
    if q is not None:
        q_out = torch.empty(q.shape, dtype=q.dtype, device=q.device)
    _ck(kv_append_q8_raw(k, v, kc, vc, kcs, vcs, lens, q, q_out, cos, sin), "ljs_kv_append_q8")
    return q_out


def attn_decode_q8_raw(q, kc, vc, kcs, vcs, o, lse, ws, lens, scale: float, extra: int = 1) -> int:
    """One ``ljs_attn_decode_q8`` call (the decode launch, and the merge launch when the plan has more than
    one split) on the tensors as they are; returns the launcher's code instead of raising."""
    B, _, H, _ = q.shape
    st = lambda t: _longs(_strides3(t)) if t is not None else None   # noqa: E731
    return lib().ljs_attn_decode_q8(_p(q), _p(kc), _p(vc), _p(kcs), _p(vcs), _p(o), _p(lse), _p(ws),
                                    ws.numel() if ws is not None else 0, _p(lens), B, H, kc.shape[2], kc.shape[1],
                                    st(q), st(kc), st(vc), st(kcs), st(vcs), st(o), float(scale), int(extra), _stream(q))


def attn_decode_q8(q, kc, vc, kcs, vcs, lens, scale: float, extra: int = 1):
    """:func:`attn_decode` over an MX-fp8 cache (e4m3 bytes ``kc`` / ``vc``, e8m0 scale bytes ``kcs`` / ``vcs``): the
    attention of bf16 ``q`` over the dequantised rows ``[0, min(lens[b] + extra, cap))``, which are exact bf16
    values; the same plan, workspace and merge launch.  ``(o`` bf16, ``lse2`` f32``)``."""
    B, T, H, _ = q.shape
    Hkv = kc.shape[2]
    ok = decode_supported(q) and _q8_cache_ok(kc, vc, kcs, vcs) and T == 1 and kc.shape[0] == B and lens is not None \
        and _lens_ok(lens, B) and H % Hkv == 0 and H // Hkv <= decode_max_group() and scale > 0
    if not ok:
        raise NotImplementedError(f"attn_decode_q8 kernel: bf16 q (B, 1, H, 64), uint8 caches (B, cap, Hkv, 64) with "
                                  f"16-byte aligned bases and strides and uint8 scales (B, cap, Hkv, 2) with even strides, "
                                  f"H / Hkv <= {decode_max_group()}, int32 [B] lens; got q {q.dtype} {tuple(q.shape)}, "
                                  f"cache {kc.dtype} {tuple(kc.shape)} strides {kc.stride()}, scales {kcs.dtype} "
                                  f"{tuple(kcs.shape)} strides {kcs.stride()}")
    splits, _ = _decode_launch_plan(B, Hkv, kc.shape[1])
    ws = _decode_ws(q.device, B * H * splits * lib().ljs_decode_part_floats()) if splits > 1 else None
    o = torch.empty((B, 1, H, 64), dtype=torch.bfloat16, device=q.device)
    lse = torch.empty((B, H, 1), dtype=torch.float32, device=q.device)
    _ck(attn_decode_q8_raw(q, kc, vc, kcs, vcs, o, lse, ws, lens, scale, extra), "ljs_attn_decode_q8")
    return o, lse


# ---- several query positions per sequence over the cache (attn_extend: decode.hip's EXT instances)
def extend_max_positions() -> int:
    """The most query positions per sequence one ``attn_extend`` call takes."""
    return lib().ljs_extend_max_positions()


def attn_extend_raw(q, kc, vc, o, lse, ws, lens, scale: float) -> int:
    """One ``ljs_attn_extend`` call (the launch, and the merge launch when the plan has more than one split) on
    the tensors as they are (``lse``: f32 ``(B, T, H)``); returns the launcher's code instead of raising."""
    B, T, H, _ = q.shape
    return lib().ljs_attn_extend(_p(q), _p(kc), _p(vc), _p(o), _p(lse), _p(ws), ws.numel() if ws is not None else 0,
                                 _p(lens), B, T, H, kc.shape[2], kc.shape[1], _longs(_strides3(q)),
                                 _longs(_strides3(kc)), _longs(_strides3(vc)), _longs(_strides3(o)), float(scale),
                                 _stream(q))


def attn_extend_q8_raw(q, kc, vc, kcs, vcs, o, lse, ws, lens, scale: float) -> int:
    """One ``ljs_attn_extend_q8`` call on the tensors as they are; returns the launcher's code instead of raising."""
    B, T, H, _ = q.shape
    st = lambda t: _longs(_strides3(t)) if t is not None else None   # noqa: E731
    return lib().ljs_attn_extend_q8(_p(q), _p(kc), _p(vc), _p(kcs), _p(vcs), _p(o), _p(lse), _p(ws),
                                    ws.numel() if ws is not None else 0, _p(lens), B, T, H, kc.shape[2], kc.shape[1],
                                    st(q), st(kc), st(vc), st(kcs), st(vcs), st(o), float(scale), _stream(q))


def _extend_out(q, Hkv: int, cap: int):
    """(o, lse (B, T, H), ws) of an extend call on ``q``: the workspace holds ``B T H`` partials per split."""
    B, T, H, _ = q.shape
    splits, _ = _decode_launch_plan(B, Hkv, cap)
    ws = _decode_ws(q.device, B * T * H * splits * lib().ljs_decode_part_floats()) if splits > 1 else None
    o = torch.empty((B, T, H, 64), dtype=torch.bfloat16, device=q.device)
    lse = torch.empty((B, T, H), dtype=torch.float32, device=q.device)
    return o, lse, ws


def attn_extend(q, kc, vc, lens, scale: float):
    """Attention of ``q`` (B, T, H, 64), ``1 <= T <= 64`` positions that a :func:`kv_append` has just written at rows
    ``lens[b] .. lens[b] + T - 1``, over the caches: row ``(b, t, h)`` attends to rows ``[0, min(lens[b] + t + 1, cap))``
    and has the bits :func:`attn_decode` gives ``(b, h)`` with ``extra = t + 1``.  ``(o`` bf16 (B, T, H, 64), ``lse2`` f32
    (B, H, T)``)``; ``T == 1`` is :func:`attn_decode`'s launches."""
    B, T, H, _ = q.shape
    Hkv = kc.shape[2]
    ok = decode_supported(q, kc, vc) and 1 <= T <= extend_max_positions() and kc.shape == vc.shape \
        and kc.shape[0] == B and lens is not None and _lens_ok(lens, B) and H % Hkv == 0 \
        and H // Hkv <= decode_max_group() and scale > 0
    if not ok:
        raise NotImplementedError(f"attn_extend kernel: bf16 q (B, T <= {extend_max_positions()}, H, 64) and caches (B, cap, "
                                  f"Hkv, 64) with 16-byte aligned bases and strides, H / Hkv <= {decode_max_group()}, int32 "
                                  f"[B] lens; got q {q.dtype} {tuple(q.shape)}, cache {kc.dtype} {tuple(kc.shape)} strides "
                                  f"{kc.stride()}")
    o, lse, ws = _extend_out(q, Hkv, kc.shape[1])
    _ck(attn_extend_raw(q, kc, vc, o, lse, ws, lens, scale), "ljs_attn_extend")
    return o, lse.permute(0, 2, 1)


def attn_extend_q8(q, kc, vc, kcs, vcs, lens, scale: float):
    """:func:`attn_extend` over an MX-fp8 cache: the bits of :func:`attn_decode_q8` with ``extra = t + 1``."""
    B, T, H, _ = q.shape
    Hkv = kc.shape[2]
    ok = decode_supported(q) and _q8_cache_ok(kc, vc, kcs, vcs) and 1 <= T <= extend_max_positions() \
        and kc.shape[0] == B and lens is not None and _lens_ok(lens, B) and H % Hkv == 0 \
        and H // Hkv <= decode_max_group() and scale > 0
    if not ok:
        raise NotImplementedError(f"attn_extend_q8 kernel: bf16 q (B, T <= {extend_max_positions()}, H, 64), uint8 caches (B, "
                                  f"cap, Hkv, 64) with 16-byte aligned bases and strides and uint8 scales (B, cap, Hkv, 2) "
                                  f"with even strides, H / Hkv <= {decode_max_group()}, int32 [B] lens; got q {q.dtype} "
                                  f"{tuple(q.shape)}, cache {kc.dtype} {tuple(kc.shape)} strides {kc.stride()}, scales "
                                  f"{kcs.dtype} {tuple(kcs.shape)} strides {kcs.stride()}")
    o, lse, ws = _extend_out(q, Hkv, kc.shape[1])
    _ck(attn_extend_q8_raw(q, kc, vc, kcs, vcs, o, lse, ws, lens, scale), "ljs_attn_extend_q8")
    return o, lse.permute(0, 2, 1)


def lens_add(lens: torch.Tensor, n: int = 1) -> torch.Tensor:
    """``lens += n`` in place (int32 on the device): one small launch, after the last layer of a step."""
    if not (lens.is_cuda and lens.dtype == torch.int32 and lens.is_contiguous() and lens.numel()):
        raise NotImplementedError(f"lens_add: a contiguous int32 GPU tensor, got {lens.dtype} on {lens.device}")
    _ck(lib().ljs_lens_add(_p(lens), lens.numel(), int(n), _stream(lens)), "ljs_lens_add")
    return lens


# ============================================================================ skinny GEMM (M <= 16)
# csrc/kernels/skinny.hip: the decode projections' weight-streaming GEMM, forward only.
SKINNY_MAX_M = 16
SKINNY_WAVES = (1, 2, 4, 8, 16)     # the block sizes the kernel takes, in waves


def set_skinny_waves(n: Optional[int]) -> None:
    """Tests: force ``skinny``'s blocks to ``n`` waves (one of :data:`SKINNY_WAVES`); None or <= 0 restores
    :func:`skinny_plan`."""
    if lib().ljs_skinny_set_waves(int(n or 0)) != 0:
        raise ValueError(f"set_skinny_waves: {n} is not one of {SKINNY_WAVES}")


def skinny_plan(M: int, N: int, K: int, cus: int = 256):
    """``(waves_per_block, blocks)`` of :func:`skinny` for ``x [M][K] @ Wt [N][K]^T`` on a device of ``cus``
    compute units (``ljs_skinny_plan``: needs the library, not a GPU).  Pure: of the shape and the CU count
    alone, and ``M`` only has to lie in 1 .. 16.  ValueError outside ``1 <= M <= 16, K % 32 == 0, N % 8 == 0``."""
    out = (c_int * 2)()
    if lib().ljs_skinny_plan(int(M), int(N), int(K), int(cus), out) != 0:
        raise ValueError(f"skinny_plan: M={M}, N={N}, K={K}, cus={cus}: 1 <= M <= {SKINNY_MAX_M}, K % 32 == 0, "
                         "N % 8 == 0 and cus >= 1 are required")
    return int(out[0]), int(out[1])


def skinny_supported(M: int, N: int, K: int, lda: int, ldb: int, ldc: int, out_dtype: torch.dtype, x_addr: int = 0,
                     wt_addr: int = 0, out_addr: int = 0, bias_dtype: Optional[torch.dtype] = None, bias_addr: int = 0,
                     res_dtype: Optional[torch.dtype] = None, res_ld: int = 0, res_addr: int = 0,
                     x_dtype: torch.dtype = torch.bfloat16, wt_dtype: torch.dtype = torch.bfloat16) -> bool:
    """``ljs_skinny_bf16``'s gate as a pure predicate of shapes, dtypes, leading dimensions (elements) and
    byte addresses: ``1 <= M <= 16``, ``K % 32 == 0``, ``N % 8 == 0``; bf16 x and Wt with 16-byte aligned
    rows; a bf16 or f32 output (and a bf16 or f32 residual, bf16 output only) aligned to a lane's four
    values, 8 bytes of bf16 or 16 of f32; an f32 or bf16 bias."""
    if not (1 <= M <= SKINNY_MAX_M and N >= 8 and N % 8 == 0 and K >= 32 and K % 32 == 0):
        return False
    if x_dtype != torch.bfloat16 or wt_dtype != torch.bfloat16 or out_dtype not in (torch.bfloat16, torch.float32):
        return False
    if lda < K or ldb < K or ldc < N or lda % 8 or ldb % 8 or ldc % 4 or x_addr % 16 or wt_addr % 16:
        return False
    if out_addr % (16 if out_dtype == torch.float32 else 8):
        return False
    if bias_dtype is not None and (bias_dtype not in (torch.bfloat16, torch.float32)
                                   or bias_addr % (4 if bias_dtype == torch.float32 else 2)):
        return False
    if res_dtype is not None and (res_dtype not in (torch.bfloat16, torch.float32) or out_dtype != torch.bfloat16
                                  or res_ld < N or res_ld % 4
                                  or res_addr % (16 if res_dtype == torch.float32 else 8)):
        return False
    return True


def skinny_raw(x, wt, out, M: int, N: int, K: int, lda: int, ldc: int, bias=None, relu: bool = False, res=None,
               res_ld: int = 0, ldb: Optional[int] = None) -> int:
    """One ``ljs_skinny_bf16`` call on the operands as they are (``wt`` may be None: a null operand); returns
    the launcher's code (non-zero: rejected, nothing launched or recorded) instead of raising."""
    f32 = torch.float32
    return lib().ljs_skinny_bf16(_p(x), _p(wt), _p(out), _p(bias), _p(res), int(M), int(N), int(K), int(lda),
                                 int(K if ldb is None else ldb), int(ldc), int(res_ld), int(out.dtype == f32),
                                 int(bias is not None and bias.dtype == f32), int(res is not None and res.dtype == f32),
                                 int(bool(relu)), _stream(out))


def skinny(x: torch.Tensor, wt: torch.Tensor, out: torch.Tensor, M: int, N: int, K: int, lda: int, ldc: int,
           bias: Optional[torch.Tensor] = None, relu: bool = False, res: Optional[torch.Tensor] = None,
           res_ld: int = 0, ldb: Optional[int] = None) -> None:
    """``out[m][n] = epi(sum_k x[m][k] wt[n][k])`` for ``1 <= M <= 16`` (csrc/kernels/skinny.hip): bf16 ``x`` (row
    stride ``lda``) and ``wt`` (the ``[N][K]`` transposed weight shadow, row stride ``ldb``, default ``K``), ``out`` bf16
    or f32 with row stride ``ldc >= N``.  Epilogue: ``+ bias`` (f32 or bf16) in f32, ReLU, the rounding, then
    ``bf16(bf16(y) + bf16(res))`` for a residual (f32 or bf16, row stride ``res_ld``; bf16 output only).  One launch,
    deterministic, no workspace.  Raises for anything :func:`skinny_supported` refuses."""
    ok = all(t is None or t.is_cuda for t in (x, wt, out, bias, res)) and skinny_supported(
        M, N, K, lda, K if ldb is None else ldb, ldc, out.dtype, x.data_ptr(), wt.data_ptr(), out.data_ptr(),
        None if bias is None else bias.dtype, 0 if bias is None else bias.data_ptr(),
        None if res is None else res.dtype, res_ld, 0 if res is None else res.data_ptr(), x.dtype, wt.dtype)
    if not ok:
        raise NotImplementedError(f"skinny kernel: bf16 GPU x [M <= 16][K % 32 == 0] and wt [N % 8 == 0][K] with 16-byte "
                                  f"aligned rows, a bf16 / f32 output; got M={M} N={N} K={K} lda={lda} ldb={ldb} "
                                  f"ldc={ldc} x {x.dtype} wt {wt.dtype} out {out.dtype}")
    _ck(skinny_raw(x, wt, out, M, N, K, lda, ldc, bias, relu, res, res_ld, ldb), "ljs_skinny_bf16")


# ============================================================================ optimizer
def adam(p, g, m, v, step, lr, b1, b2, eps, wd, inplace):
    assert p.dtype == torch.float32 and m.dtype == torch.float32 and v.dtype == torch.float32
    g = g.contiguous()
    if g.dtype not in (torch.float32, torch.bfloat16):
        g = g.float()
    pc, mc, vc = p.contiguous(), m.contiguous(), v.contiguous()
    if inplace and pc.data_ptr() == p.data_ptr():
        po, mo, vo = p, m, v
    else:
        po, mo, vo = torch.empty_like(pc), torch.empty_like(mc), torch.empty_like(vc)
    step_i = step if step.dtype == torch.int32 else step.to(torch.int32)
    rc = lib().ljs_adam_f32(_p(pc), _p(g), int(g.dtype == torch.bfloat16), _p(mc), _p(vc), _p(po), _p(mo), _p(vo),
                            _p(step_i), p.numel(), lr, b1, b2, eps, wd, _stream(p))
    _ck(rc, "ljs_adam_f32")
    return po.view(p.shape), mo.view(m.shape), vo.view(v.shape)


class SlabGrad:
    """A weight gradient not yet combined: element (r, c) is the sum over s < S of
    ``slabs.view(-1)[offset + s * slab_stride + r * ld + c]`` (the split-K slabs of its GEMM)."""
    __slots__ = ("slabs", "S", "offset", "ld", "slab_stride", "shape")

    def __init__(self, slabs, S, offset, ld, slab_stride, shape):
        self.slabs, self.S, self.offset, self.ld, self.slab_stride = slabs, S, offset, ld, slab_stride
        self.shape = tuple(shape)


class ConstGrad:
    """A gradient whose every element is ``value`` (f32)."""
    __slots__ = ("value", "shape")

    def __init__(self, value, shape):
        self.value, self.shape = float(value), tuple(shape)


# Count increments deferred inside a HIP-graph capture (a G-step graph): each Adam launch reads the
# count as it was at the last flush plus the increments still pending, and the pending increments
# become ONE launch when the capture segment ends (spmd/graphs.BEFORE_CUT) -- one count launch per
# graph instead of one per step.  Eager calls and single-controller multi-device captures
# increment at once.  LJS_ADAM_DEFER_INC=0: off.
_DEFER_INC = os.environ.get("LJS_ADAM_DEFER_INC", "1") == "1"
_PENDING_INC: Dict[int, list] = {}     # step data_ptr -> [step tensor, pending increments]


def _flush_step_incs() -> None:
    while _PENDING_INC:
        _, (st, n) = _PENDING_INC.popitem()
        if n:
            _ck(lib().ljs_step_add(_p(st), n, _stream(st)), "ljs_step_add")


def flush_step_inc(step: torch.Tensor) -> None:
    """Launch ``step``'s pending deferred increments now (in stream order), so a kernel that reads
    the count after this point -- anything but the next Adam launch, which adds the pending
    offset itself -- sees the incremented value (optim/adam.CountLocal calls this on reads)."""
    ent = _PENDING_INC.get(step.data_ptr())
    if ent is not None and ent[1]:
        _ck(lib().ljs_step_add(_p(ent[0]), ent[1], _stream(ent[0])), "ljs_step_add")
        ent[1] = 0


def _defer_step_inc(step: torch.Tensor):
    """Pending increments of ``step`` before this one (and one more recorded), or None when the
    increment must be launched now."""
    if not _DEFER_INC:
        return None
    from ..spmd import graphs as _graphs
    g = _graphs.current()
    if g is None or isinstance(g, _graphs.MultiDeviceGraph):
        return None
    if _flush_step_incs not in _graphs.BEFORE_CUT:
        _graphs.BEFORE_CUT.append(_flush_step_incs)
    ent = _PENDING_INC.setdefault(step.data_ptr(), [step, 0])
    pend = ent[1]
    ent[1] += 1
    return pend




_ADAM_ROWS = [0]


def set_adam_rows(rows: int) -> None:
    """Force the fused Adam's tile height (16 / 32 / 64; 0 = automatic: 32, or 64 when a tensor
    carries MX-fp8 shadows).  For tests of the kernel's tile paths; bit-identical results."""
    lib().ljs_adam_set_rows(int(rows))
    _ADAM_ROWS[0] = int(rows)


def adam_rows() -> int:
    return _ADAM_ROWS[0]


def _grad_source(g, shape):
    """One row's gradient fields of the fused Adam's table, ``(R, C, (pointer, is_bf16, gS, g_ld,
    g_ss), g)`` (csrc/kernels/adam_common.h AdamTensor), for a gradient of ``shape`` in any of its
    source forms; the returned ``g`` has to outlive the launch."""
    import numpy as np
    shape = tuple(shape)
    R, C = (shape[0], shape[1]) if len(shape) == 2 else (1, int(math.prod(shape)))
    if isinstance(g, SlabGrad):
        # the weight gradient is still its split-K slabs: the kernel sums them (no combine)
        assert g.shape == shape and g.slabs.dtype in (torch.float32, torch.bfloat16) \
            and g.slabs.is_contiguous()
        es = g.slabs.element_size()
        gsrc = (g.slabs.data_ptr() + es * g.offset, int(es == 2), g.S, g.ld, g.slab_stride)
    elif isinstance(g, ConstGrad):
        assert g.shape == shape
        bits = int(np.asarray(g.value, dtype=np.float32).view(np.int32))
        gsrc = (0, 0, -1, bits, 0)
    else:
        if g.dtype not in (torch.float32, torch.bfloat16) or not g.is_contiguous():
            g = g.float().contiguous() if g.dtype not in (torch.float32, torch.bfloat16) else g.contiguous()
        gsrc = (g.data_ptr(), int(g.dtype == torch.bfloat16), 0, C, 0)
    return R, C, gsrc, g


def take_step_offset(step: torch.Tensor, increment_step: bool):
    """``(step_offset, pending)`` of the optimizer launches of one step: the kernels use
    ``t = *step + step_offset``.  Read once per step and given to every launch of it
    (:func:`step_hyper`, :func:`adam_multi` with ``taken=``): inside a capture this records one
    more deferred increment (``_defer_step_inc``)."""
    if increment_step:
        assert step.dtype == torch.int32 and step.is_contiguous()
    pend = _defer_step_inc(step) if increment_step else None
    return int(increment_step) + (pend or 0), pend


def _sumsq_ws(dev: torch.device) -> torch.Tensor:
    return _workspace(dev, "grad_sumsq", 4 * lib().ljs_grad_sumsq_ws_words())


def grad_sumsq(sources, device: torch.device) -> torch.Tensor:
    """Sum of squares of many gradients read where they lie, one launch per 32: ``sources`` =
    ``[(shape, g)]`` with ``g`` a plain f32 / bf16 tensor, a :class:`SlabGrad` (the slabs are summed
    in ``slab_reduce``'s order, then squared) or a :class:`ConstGrad`.  Returns the float64
    ``[launches]`` view of the launches' slots in the device's persistent workspace (valid until the
    next call on this device); their sum is the result."""
    import numpy as np
    ws = _sumsq_ws(device)
    rows = []
    for shape, g in sources:
        R, C, gsrc, g = _grad_source(g, shape)
        rows.append(([0, gsrc[0], 0, 0, 0, 0, R, C, gsrc[1], gsrc[2], 0, 0, 0, 0, gsrc[3], gsrc[4]], g))
    n_launch = (len(rows) + 31) // 32
    if n_launch > lib().ljs_grad_sumsq_slots():
        raise ValueError(f"grad_sumsq: {len(rows)} tensors need {n_launch} launches; the workspace holds "
                         f"{lib().ljs_grad_sumsq_slots()} slots")
    stream = torch.cuda.current_stream(device).cuda_stream
    for k in range(n_launch):
        chunk = rows[32 * k:32 * k + 32]
        tab = np.asarray([r[0] for r in chunk], dtype=np.int64).reshape(-1)
        arr = (ctypes.c_long * tab.size)(*tab.tolist())
        _ck(lib().ljs_grad_sumsq(arr, len(chunk), _p(ws), k, stream), "ljs_grad_sumsq")
    w0 = lib().ljs_grad_sumsq_slot_word()
    return ws[w0:w0 + 2 * n_launch].view(torch.float64)


def step_hyper(step: torch.Tensor, step_offset: int, schedule=None, lr: float = 0.0, max_norm=None,
               slots: Optional[torch.Tensor] = None, gathered: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One one-wave launch writing the step's f32 record ``[grad_scale, lr, norm, 0]`` for the dynamic
    Adam instance.  The sum of squares is ``slots`` (float64, added in index order) or, when given,
    ``gathered`` (the devices' float64 sums, in device-id order); ``max_norm`` None: no clipping.
    ``schedule``: an ``optim.schedule.Schedule`` evaluated on the device at ``*step + step_offset - 1``
    (else the constant ``lr``)."""
    rec = torch.empty(4, dtype=torch.float32, device=step.device)
    kind, ps = (schedule.kind, schedule.params) if schedule is not None else (0, (float(lr), 0.0, 0.0, 0.0, 0.0))
    for t in (slots, gathered):
        assert t is None or (t.dtype == torch.float64 and t.is_contiguous() and t.device == step.device)
    rc = lib().ljs_step_hyper(_p(slots), 0 if slots is None else slots.numel(), _p(gathered),
                              0 if gathered is None else gathered.numel(), None, _p(step), int(step_offset),
                              int(max_norm is not None), float(max_norm or 0.0), int(kind), *[float(x) for x in ps],
                              _p(rec), _stream(step))
    _ck(rc, "ljs_step_hyper")
    return rec


def sumsq_partial(slots: torch.Tensor) -> torch.Tensor:
    """The float64 ``[1]`` sum of a device's launch slots, in index order (its contribution to the
    all-gather of a sharded tree's norm)."""
    out = torch.empty(1, dtype=torch.float64, device=slots.device)
    rc = lib().ljs_step_hyper(_p(slots), slots.numel(), None, 0, _p(out), None, 0, 0, 0.0, 0, 0.0, 0.0, 0.0, 0.0, 0.0,
                              None, _stream(slots))
    _ck(rc, "ljs_step_hyper")
    return out


def adam_multi(entries, step: torch.Tensor, lr, b1, b2, eps, wd, increment_step: bool = False,
               hyper: Optional[torch.Tensor] = None, taken=None) -> None:
    """In-place fused Adam over many params (one launch per 32): entries = [(p, g, m, v)].

    Also rewrites each param's registered bf16 and MX-fp8 shadows (see :mod:`.shadow`).  With
    ``increment_step`` the bias corrections use ``step + 1`` and int32 ``step`` is incremented in
    place by a one-lane launch -- inside a graph capture one launch per segment for all its
    steps (``_defer_step_inc``).

    ``hyper``: the record of :func:`step_hyper` -- the dynamic kernel instance takes the learning
    rate from it (``lr`` is ignored) and multiplies every gradient by its ``grad_scale``;
    ``taken``: the step's :func:`take_step_offset`, when a launch before this one already read it."""
    from . import shadow
    import numpy as np
    rows = []
    for p, g, m, v in entries:
        assert p.is_contiguous() and m.is_contiguous() and v.is_contiguous() and p.dtype == torch.float32
        R, C, gsrc, g = _grad_source(g, p.shape)
        bufs = shadow.kinds_of(p) if p.dim() == 2 else {}
        st, sn = bufs.get("T"), bufs.get("N")
        ptr = lambda k: bufs[k].data_ptr() if k in bufs else 0  # noqa: E731
        rows.append(([p.data_ptr(), gsrc[0], m.data_ptr(), v.data_ptr(),
                      st.data_ptr() if st is not None else 0, sn.data_ptr() if sn is not None else 0,
                      R, C, gsrc[1], gsrc[2],
                      ptr("QN"), ptr("QNs"), ptr("QT"), ptr("QTs"), gsrc[3], gsrc[4]], g))
    if increment_step:
        assert step.dtype == torch.int32 and step.is_contiguous()
    step_i = step if step.dtype == torch.int32 else step.to(torch.int32)
    # inside a capture the increments are deferred (one launch per capture segment, see
    # _defer_step_inc): this launch reads the not-yet-incremented count, offset by what is pending
    offset, pend = taken if taken is not None else take_step_offset(step_i, increment_step)
    # the next step's input cast, run by the last launch's extra blocks (ops/linear.py early cast)
    cast = None
    if rows and step_i.is_cuda:
        from . import linear as _lin
        cast = _lin.take_optimizer_precast(step_i.device)
    for i in range(0, len(rows), 32):
        chunk = rows[i:i + 32]
        tab = np.asarray([r[0] for r in chunk], dtype=np.int64).reshape(-1)
        arr = (ctypes.c_long * tab.size)(*tab.tolist())
        last = i + 32 >= len(rows)
        cj = cast if last else None
        cargs = (_p(cj[0]) if cj else None, _p(cj[1]) if cj else None, cj[0].numel() if cj else 0, _stream(step_i))
        if hyper is not None:
            rc = lib().ljs_adam_multi_dyn(arr, len(chunk), _p(step_i), offset, _p(hyper), b1, b2, eps, wd, *cargs)
        else:
            rc = lib().ljs_adam_multi(arr, len(chunk), _p(step_i), offset, None, lr, b1, b2, eps, wd, *cargs)
        _ck(rc, "ljs_adam_multi")
        if cj is not None:
            _lin.commit_optimizer_precast(cj)
    if increment_step and pend is None:
        _ck(lib().ljs_step_add(_p(step_i), 1, _stream(step_i)), "ljs_step_add")
    for p, _, _, _ in entries:
        shadow.mark_fresh(p)


# ============================================================================ clock probe
_CLOCK: Dict[int, tuple] = {}   # device index -> (records [cap, 4] int64, counter int32)


def clock_probe(dev: torch.device, ticks: int = 300, cap: int = 8192) -> None:
    """Record the shader clock here in the stream (csrc/kernels/diag.hip): one lane spins for
    ``ticks`` of the 100 MHz counter (3 us) and stores delta s_memtime / delta s_memrealtime; a
    diagnostic, launched by bench.py after every step under LJS_CLOCK_PROBE (graph-capturable)."""
    dev = torch.device(dev)
    ent = _CLOCK.get(dev.index)
    if ent is None:
        ent = _CLOCK[dev.index] = (torch.zeros((cap, 4), dtype=torch.int64, device=dev),
                                   torch.zeros(1, dtype=torch.int32, device=dev))
    rec, ctr = ent
    _ck(lib().ljs_clock_probe(_p(rec), _p(ctr), rec.shape[0], int(ticks), torch.cuda.current_stream(dev).cuda_stream),
        "ljs_clock_probe")


def clock_probe_records(dev: torch.device) -> List[dict]:
    """Every record so far, in launch order: shader clock (MHz), start (us of the 100 MHz counter)."""
    ent = _CLOCK.get(torch.device(dev).index)
    if ent is None:
        return []
    torch.cuda.synchronize(dev)
    rec, ctr = ent
    n = min(int(ctr.item()), rec.shape[0])
    out = []
    for d_sclk, d_ref, ref0, xcc in rec[:n].cpu().tolist():
        out.append({"sclk_mhz": round(d_sclk / max(1, d_ref) * 100.0, 1), "t_us": ref0 / 100.0, "xcc": int(xcc)})
    return out


# ============================================================================ RNG
_DIST = {"normal": 0, "uniform": 1, "truncated_normal": 2}


def rng_fill(shape, region, k0, k1, dist, lo, hi, dtype, device) -> torch.Tensor:
    if dist not in _DIST:
        raise NotImplementedError(dist)
    local = tuple(r1 - r0 for r0, r1 in region)
    od = dtype if dtype in (torch.float32, torch.bfloat16) else torch.float32
    out = torch.empty(local, dtype=od, device=device)
    nd = len(shape)
    strides = [1] * nd
    for i in range(nd - 2, -1, -1):
        strides[i] = strides[i + 1] * shape[i + 1]
    ea = eb = 0.0
    if dist == "truncated_normal":
        ea, eb = math.erf(lo / math.sqrt(2)), math.erf(hi / math.sqrt(2))
    if out.numel():
        rc = lib().ljs_rng_fill(_p(out), int(od == torch.bfloat16), nd, _longs([r[0] for r in region] or [0]),
                                _longs(list(local) or [1]), _longs(strides or [1]), k0, k1, _DIST[dist], lo, hi, ea,
                                eb, torch.cuda.current_stream(device).cuda_stream)
        _ck(rc, "ljs_rng_fill")
    return out if od == dtype else out.to(dtype)


# ============================================================================ dropout
def _dropout_raw(x: torch.Tensor, shape, region, k0: int, k1: int, keep: float) -> torch.Tensor:
    x = x.contiguous()
    y = torch.empty_like(x)
    nd = len(shape)
    strides = [1] * nd
    for i in range(nd - 2, -1, -1):
        strides[i] = strides[i + 1] * shape[i + 1]
    rc = lib().ljs_dropout(_p(x), _p(y), int(x.dtype == torch.bfloat16), nd, _longs([r[0] for r in region]),
                           _longs([r1 - r0 for r0, r1 in region]), _longs(strides), k0, k1, keep, _stream(x))
    _ck(rc, "ljs_dropout")
    return y


class _Dropout(torch.autograd.Function):
    """Counter-based dropout of one shard (csrc/kernels/elementwise.hip dropout_kernel): the
    backward recomputes the mask from the key, nothing is stored."""

    @staticmethod
    def forward(ctx, x, meta):
        shape, region, k0, k1, keep = meta
        ctx.meta = meta
        return _dropout_raw(x, shape, region, k0, k1, keep)

    @staticmethod
    def backward(ctx, dy):
        shape, region, k0, k1, keep = ctx.meta
        return _dropout_raw(dy, shape, region, k0, k1, keep), None


def dropout(x: torch.Tensor, shape, region, k0: int, k1: int, keep: float) -> torch.Tensor:
    """Dropout of the shard ``x`` (region ``region`` of a global array of ``shape``), f32 / bf16."""
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise NotImplementedError(f"dropout kernel: f32 / bf16 only, got {x.dtype}")
    return _Dropout.apply(x, (tuple(shape), tuple(region), int(k0), int(k1), float(keep)))
