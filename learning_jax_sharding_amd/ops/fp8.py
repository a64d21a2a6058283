"""MX-fp8 (OCP e4m3 + e8m0 block scales) dense layers on CDNA4 block-scaled MFMA.

North-star config "attention+FF transformer layer, 2D mesh, fp8 MFMA (CDNA4)" (BASELINE.json;
the FF formula of ``case6_attention.py:36-40``).  Recipe:

* forward GEMM in MX-fp8: activations quantized per row in 32-element blocks along K
  (shared exponent = OCP's floor(log2 amax) - 8, plus one when the block max would
  saturate, i.e. its mantissa exceeds 1.75),
  weights quantized per output column (also along K) and cached per weight version;
  ``v_mfma_scale_f32_16x16x128_f8f6f4`` applies the block scales inside the MFMA and
  accumulates in f32 (twice the bf16 MFMA rate per clock); bias/ReLU fused in the epilogue;
* backward in bf16 with the same kernels as :mod:`.linear` (gradients keep bf16 range,
  the common fp8-training split).

On host devices (CPU) the same math runs as an exact emulation (quantize -> dequantize ->
f32 matmul), so sharded CPU runs and the GPU kernels agree up to f32 summation order.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import os

import torch

from . import hip
from .linear import _Linear, _bf16, _inv_perm

__all__ = ["quantize_mx_ref", "dequantize_mx_ref", "mx_linear_ref", "quant_rows", "quant_cols", "gemm_mx",
           "gemm_mx_plan", "mx_flags", "linear_fp8", "fp8_dense", "E4M3_MAX", "BLOCK"]

E4M3_MAX = 448.0
BLOCK = 32

# the epilogue flags of ljs_gemm_mx_fp8 (enum MxFlag, csrc/kernels/fp8.hip)
MX_RELU, MX_BIAS, MX_BIAS_F32, MX_OUT_F32 = 1, 2, 4, 32
MX_RES_ADD, MX_RES_MASK = 64, 128            # residual add of ``res`` / ReLU mask (keep where res > 0)
MX_QC, MX_QT = 256, 512                      # MX copy of the output / its transposed MX copy
MX_RES_E4M3 = 1024                           # ``res`` is e4m3 bytes (mask mode)
MX_COLSUM = 2048                             # per-row-tile column sums of the bf16 output (8-wave tiles)

_SIGS = {
    "ljs_quant_mx_rows": [ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p],
    "ljs_quant_mx_cols": [ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                          ctypes.c_void_p, ctypes.c_void_p],
    "ljs_quant_mx_both": [ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p],
    "ljs_bcast_scalar_mx2": [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                             ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p],
    "ljs_bcast_scalar_mx": [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                            ctypes.c_void_p, ctypes.c_void_p],
    "ljs_gemm_mx_fp8": [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                        ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_long, ctypes.c_int,
                        ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                        ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_int,
                        ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p],
}
# the same call without the stream, plus (int* out, char* name, int name_cap)
_PLAN_SIG = _SIGS["ljs_gemm_mx_fp8"][:-1] + [ctypes.POINTER(ctypes.c_int), ctypes.c_char_p, ctypes.c_int]
_PLAN_FIELDS = ("err", "resolved_tile", "family", "BM", "BN", "WM", "NST", "fix", "out_f32", "nsplit", "kps", "grid",
                "block")
_PLAN_FAMILIES = ("4-wave", "8-wave")
_bound = False


def _lib():
    global _bound
    L = hip.lib()
    if not _bound:
        for name, argt in _SIGS.items():
            fn = getattr(L, name)
            fn.argtypes = argt
            fn.restype = ctypes.c_int
        _bound = True
    return L


# ----------------------------------------------------------------------------- host reference
def _block_exponent(amax: torch.Tensor) -> torch.Tensor:
    """Shared exponent: OCP MX's floor(log2(amax)) - emax(e4m3 = 8), raised by one when the
    block max would still exceed 448 (mantissa > 1.75), so no element saturates; clamped to
    e8m0's range."""
    m, e = torch.frexp(amax)
    x = e - 1 - 8 + (m > 0.875).to(e.dtype)
    x = torch.where(amax > 0, x, torch.full_like(x, -127))
    return x.clamp(-127, 127)


def quantize_mx_ref(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """x[..., K] -> (e4m3 values as float8_e4m3fn [..., K], int exponents [..., K/32]).

    The exponent clamps at -127 and a non-zero block that clamps is still scaled by 2^127 (scale byte 0 is
    2^-127, never "zeros"); zeros keep their sign.  Non-finite inputs are outside the contract.  Held to the
    integer oracle of tests/mx_oracle.py on every finite bf16 pattern (tests/test_mx_oracle.py)."""
    K = x.shape[-1]
    assert K % BLOCK == 0, K
    xb = x.float().reshape(*x.shape[:-1], K // BLOCK, BLOCK)
    ex = _block_exponent(xb.abs().amax(-1))
    scaled = xb * torch.ldexp(torch.ones_like(ex, dtype=torch.float32), -ex)[..., None]
    q = scaled.clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn)
    return q.reshape(x.shape), ex


def dequantize_mx_ref(q: torch.Tensor, ex: torch.Tensor) -> torch.Tensor:
    K = q.shape[-1]
    qb = q.float().reshape(*q.shape[:-1], K // BLOCK, BLOCK)
    return (qb * torch.ldexp(torch.ones_like(ex, dtype=torch.float32), ex)[..., None]).reshape(q.shape)


def mx_linear_ref(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], relu: bool,
                  out_dtype: torch.dtype) -> torch.Tensor:
    """Emulation of the GPU path: y = deq(q(x)) @ deq(q(w^T))^T (+b)(relu), f32 accumulate."""
    lead = x.shape[:-1]
    x2 = x.reshape(-1, x.shape[-1])
    xd = dequantize_mx_ref(*quantize_mx_ref(x2))
    wd = dequantize_mx_ref(*quantize_mx_ref(w.t().contiguous()))  # [N][K], blocks along K
    y = xd @ wd.t()
    if b is not None:
        y = y + b.to(out_dtype).float()
    if relu:
        y = torch.relu(y)
    return y.to(out_dtype).reshape(tuple(lead) + (w.shape[1],))


# ----------------------------------------------------------------------------- HIP path
def quant_rows(x2: torch.Tensor, out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
               xb: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """x[R][K] (f32/bf16, unit column stride) -> (q uint8 [R][K], s uint8 [R][K/32]) (``out``:
    existing contiguous buffers to write).  ``xb``: a contiguous bf16 [R][K] buffer the same pass
    fills with x rounded to bf16 (f32 x only)."""
    R, K = x2.shape
    if x2.stride(1) != 1 or x2.stride(0) % 8 or x2.data_ptr() % 16:
        x2 = x2.contiguous()
    if xb is not None:
        assert (x2.dtype == torch.float32 and xb.dtype == torch.bfloat16 and xb.is_contiguous()
                and xb.shape == (R, K) and xb.data_ptr() % 16 == 0)
    q, s = out if out is not None else (torch.empty((R, K), dtype=torch.uint8, device=x2.device),
                                        torch.empty((R, K // BLOCK), dtype=torch.uint8, device=x2.device))
    rc = _lib().ljs_quant_mx_rows(hip._p(x2), int(x2.dtype == torch.bfloat16), x2.stride(0), R, K, hip._p(q),
                                  hip._p(s), hip._p(xb) if xb is not None else None, hip._stream(x2))
    hip._ck(rc, "quant_mx_rows")
    return q, s


def quant_cols(w: torch.Tensor, out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None
               ) -> Tuple[torch.Tensor, torch.Tensor]:
    """w[K][N] -> (q uint8 [N][K], s uint8 [N][K/32]) (blocks along K, i.e. quantized W^T)."""
    K, N = w.shape
    if w.stride(1) != 1:
        w = w.contiguous()
    q, s = out if out is not None else (torch.empty((N, K), dtype=torch.uint8, device=w.device),
                                        torch.empty((N, K // BLOCK), dtype=torch.uint8, device=w.device))
    rc = _lib().ljs_quant_mx_cols(hip._p(w), int(w.dtype == torch.bfloat16), w.stride(0), K, N, hip._p(q), hip._p(s),
                                  hip._stream(w))
    hip._ck(rc, "quant_mx_cols")
    return q, s


_WCACHE = {}


def _weight_q(w: torch.Tensor):
    """MX quantization of a weight along K (the forward GEMM's B operand): the optimizer-maintained
    shadow when the weight qualifies (:func:`.shadow.get_mx`, rewritten by the fused Adam in the
    pass that updates the weight: no per-step quantization kernel), else cached per version."""
    from . import shadow
    if shadow.mx_eligible(w):
        return shadow.get_mx(w, "QT")
    key = (w.data_ptr(), tuple(w.shape), w.dtype, w.device)
    ent = _WCACHE.get(key)
    if ent is not None and ent[0] == w._version:
        return ent[1], ent[2]
    q, s = quant_cols(w.detach())
    _WCACHE[key] = (w._version, q, s)
    return q, s


def mx_flags(out_dtype=None, bias_dtype=None, relu: bool = False, res_dtype=None, res_mode: str = "add",
             qout: bool = False, qtout: bool = False, colsum: bool = False) -> int:
    """The flags word of one :func:`gemm_mx` call, from the dtypes of its tensors (None: absent)."""
    flags = (MX_RELU if relu else 0) | (MX_OUT_F32 if out_dtype == torch.float32 else 0)
    if bias_dtype is not None:
        flags |= MX_BIAS | (MX_BIAS_F32 if bias_dtype == torch.float32 else 0)
    if res_dtype is not None:
        assert res_dtype in (torch.bfloat16, torch.uint8)
        assert res_dtype == torch.bfloat16 or res_mode == "mask"
        flags |= (MX_RES_ADD if res_mode == "add" else MX_RES_MASK) | (MX_RES_E4M3 if res_dtype == torch.uint8 else 0)
    return flags | (MX_QC if qout else 0) | (MX_QT if qtout else 0) | (MX_COLSUM if colsum else 0)


def gemm_mx_plan(M: int, N: int, K: int, flags: int = 0, tile: int = 0, nsplit: int = 1, ldc: Optional[int] = None,
                 ldr: Optional[int] = None, ldqt: Optional[int] = None, **addr) -> dict:
    """What ``ljs_gemm_mx_fp8`` would launch for these numbers (``ljs_gemm_mx_plan``: the launcher's
    own plan step; needs the library, not a GPU).  ``flags``: the ``MX_*`` bits (:func:`mx_flags`);
    ``tile`` as the launcher receives it (:func:`gemm_mx` passes :func:`_auto_tile`'s answer for 0).
    Tensors are given by what the plan reads of them, their addresses: by default the output C and
    every tensor ``flags`` asks for are present and aligned; ``addr`` (keys ``C``, ``bias``, ``R``,
    ``QC``, ``SC``, ``QT``, ``ST``, ``csum``) overrides one, 0 meaning absent.  Returns the fields of
    a launch record (``name``, ``grid``, ``blocks``, ``block``, ``resolved_tile``, ``splitk``,
    ``variant``) plus ``family``, ``BM``, ``BN``, ``WM``, ``NST``, ``fix`` (the 4-wave kernel's
    compile-time epilogue, None for an 8-wave tile), ``out_f32``, ``nsplit`` and ``kps``; ``err`` is
    the launcher's error code (0: it would launch)."""
    res = flags & (MX_RES_ADD | MX_RES_MASK)
    a = dict(C=4096, bias=4096 if flags & MX_BIAS else 0, R=4096 if res else 0, QC=4096 if flags & MX_QC else 0,
             SC=4096 if flags & MX_QC else 0, QT=4096 if flags & MX_QT else 0, ST=4096 if flags & MX_QT else 0,
             csum=4096 if flags & MX_COLSUM else 0)
    assert set(addr) <= set(a), addr
    a.update(addr)
    p = {k: ctypes.c_void_p(v) if v else None for k, v in a.items()}
    fn = hip.lib().ljs_gemm_mx_plan     # (bound here: gemm_mx also serves a library without the plan export)
    fn.argtypes, fn.restype = _PLAN_SIG, ctypes.c_int
    out, name, fake = (ctypes.c_int * len(_PLAN_FIELDS))(), ctypes.create_string_buffer(64), ctypes.c_void_p(4096)
    fn(fake, fake, fake, fake, p["C"], p["bias"], M, N, K, N if ldc is None else ldc, flags, p["R"],
       (N if res else 0) if ldr is None else ldr, p["QC"], p["SC"], tile, 0, 0, p["QT"], p["ST"],
       M if ldqt is None else ldqt, nsplit, M * N if nsplit > 1 else 0, p["csum"], out, name, len(name))
    plan = dict(zip(_PLAN_FIELDS, out))
    fix = None if plan["fix"] < 0 else plan["fix"]
    plan.update(name=name.value.decode(), family=_PLAN_FAMILIES[plan["family"]], grid=(plan["grid"], 1, 1),
                blocks=plan["grid"], out_f32=bool(plan["out_f32"]), fix=fix, variant=fix, splitk=plan["nsplit"])
    return plan


def gemm_mx(qa, sa, qb, sb, M: int, N: int, K: int, out: Optional[torch.Tensor], bias: Optional[torch.Tensor] = None,
            relu: bool = False, res: Optional[torch.Tensor] = None, res_mode: str = "add",
            qout: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, tile: int = 0,
            a_bcast: bool = False, b_bcast: bool = False,
            qtout: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, nsplit: int = 1,
            colsum: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """out[M][N] = qa . qb^T (MX-fp8 operands, f32 accumulation) (+bias)(relu); epilogue options:
    ``res`` (bf16 [M][N]) added as a residual (``res_mode="add"``, bit-exact with the unfused bf16
    add) or used as a ReLU mask (``"mask"``: keep where res > 0); ``qout = (q, s)`` also receives
    the MX-fp8 quantization of the (bf16-rounded) output, blocks of 32 along N - the next GEMM's
    operand without a quantization pass.  ``out`` may be None when only ``qout`` is wanted.
    ``tile``: a code of ``LJS_MX_TILES`` (csrc/kernels/fp8.hip), 0 = automatic.  ``a_bcast`` /
    ``b_bcast``: ``qa`` / ``qb`` (and scales) hold ONE row, used for all rows (a broadcast
    gradient, never materialised).  ``qtout = (qT, sT)``: the TRANSPOSED MX copy of the output,
    qT [N][M] with blocks of 32 along M (the output as the K-major operand of a GEMM that
    contracts over M, e.g. a weight gradient over tokens).  ``res`` of dtype uint8 in "mask"
    mode: an e4m3 activation (keep where its value > 0).  ``nsplit`` > 1: split-K into f32
    slabs ``out[s]`` (``out`` [nsplit][M][N]; the caller sums them)."""
    flags = mx_flags(None if out is None else out.dtype, None if bias is None else bias.dtype, relu,
                     None if res is None else res.dtype, res_mode, qout is not None, qtout is not None)
    ldr = 0
    if res is not None:
        assert res.stride(-1) == 1
        ldr = res.stride(0) if res.dim() == 2 else N
    q_o, s_o = qout if qout is not None else (None, None)
    qt_o, st_o = qtout if qtout is not None else (None, None)
    ldc = out.stride(-2) if out is not None else N
    sC = out.stride(0) if (out is not None and nsplit > 1) else 0
    if tile == 0:
        tile = _auto_tile(M, N, K, flags, nsplit)
    if colsum is not None:
        # ``colsum`` f32 [ceil(M / BM)][N]: per-row-tile column sums of the bf16 output (8-wave
        # tiles only; the caller sums the rows)
        assert tile >= 10000 and colsum.dtype == torch.float32 and colsum.shape == (-(-M // (tile % 1000000 // 1000)), N)
        flags |= MX_COLSUM
    rc = _lib().ljs_gemm_mx_fp8(hip._p(qa), hip._p(sa), hip._p(qb), hip._p(sb), hip._p(out), hip._p(bias), M, N, K,
                                ldc, flags, hip._p(res), ldr, hip._p(q_o), hip._p(s_o), tile, int(a_bcast),
                                int(b_bcast), hip._p(qt_o), hip._p(st_o), M, nsplit, sC, hip._p(colsum), hip._stream(qa))
    hip._ck(rc, "gemm_mx_fp8")
    return out


# tile choice (scripts/fp8_tiles.py, gpurun_out/r3d/fp8_tiles.log, T=16384): the 8-wave 256x160
# tile for the N=640 GEMMs of the FF block (down projection + residual 42.9 vs 53.2 us, dX 36.0
# vs 49.0 us: one round of 256 tiles, a third fewer bytes per FLOP); the epilogue-heavy K=640
# GEMMs (up projection / dA with both MX copies) stay on the 4-wave 128x128 kernel, whose two
# blocks per CU overlap one block's epilogue with the other's K-loop.
_F8_AUTO = True


def _auto_tile(M: int, N: int, K: int, flags: int, nsplit: int) -> int:
    if not _F8_AUTO:
        return 0
    quant_out = flags & (MX_QC | MX_QT)
    if not quant_out and nsplit == 1 and N % 160 == 0 and N <= 1280 and M >= 4096 and K >= 1024:
        return _F8_N640_TILE
    return 0


_F8_N640_TILE = 256160


class _Fp8Linear(torch.autograd.Function):
    """Forward on MX-fp8 MFMA; backward = :class:`.linear._Linear`'s bf16 backward (same ctx and
    input layout: ``res`` is always None here)."""

    @staticmethod
    def forward(ctx, x, b, res, relu, out_dtype, w):
        lead = x.shape[:-1]
        K = x.shape[-1]
        x2 = x.reshape(-1, K)
        M, N = x2.shape[0], w.shape[1]
        # an f32 input's bf16 copy (the backward's dW operand) comes out of the quantization pass,
        # which reads x anyway: no separate cast pass over x (verdict r5 item 5)
        xb = None
        if x2.dtype == torch.float32:
            if not x2.is_contiguous() or x2.data_ptr() % 16:
                x2 = x2.contiguous()
            xb = torch.empty((M, K), dtype=torch.bfloat16, device=x.device)
        qa, sa = quant_rows(x2, xb=xb)
        qb, sb = _weight_q(w)
        od = out_dtype if out_dtype in (torch.bfloat16, torch.float32) else torch.float32
        out = torch.empty((M, N), dtype=od, device=x.device)
        bias = None if b is None else (b if b.dtype in (torch.float32, torch.bfloat16) else b.float()).contiguous()
        gemm_mx(qa, sa, qb, sb, M, N, K, out, bias, relu)
        y = out.view(tuple(lead) + (N,))
        if od != out_dtype:
            y = y.to(out_dtype)
        if xb is None:
            xb = _bf16(x2 if x2.is_contiguous() else x2.contiguous())
        ctx.save_for_backward(xb, b, w, *([y] if relu else []))
        ctx.meta = (lead, K, M, N, 1, relu, x.dtype, b is not None)
        ctx.has_res = False
        ctx.premask = False
        return y

    @staticmethod
    def backward(ctx, dy):
        return _Linear.backward(ctx, dy)


class _Fp8LinearRef(torch.autograd.Function):
    """Host emulation with the GPU path's autograd: MX-fp8 forward, bf16 straight-through
    backward (dX = dY W^T, dW = X^T dY on bf16-rounded operands, f32 accumulation)."""

    @staticmethod
    def forward(ctx, x, b, relu, out_dtype, w):
        y = mx_linear_ref(x, w, b, relu, out_dtype)
        ctx.save_for_backward(x, b, w, y if relu else None)
        ctx.relu = relu
        return y

    @staticmethod
    def backward(ctx, dy):
        x, b, w, y = ctx.saved_tensors
        K, N = w.shape
        g = dy.reshape(-1, N).float()
        if ctx.relu:
            g = g * (y.reshape(-1, N) > 0).float()
        g = g.to(torch.bfloat16).float()
        xb = x.reshape(-1, K).to(torch.bfloat16).float()
        dx = (g @ w.to(torch.bfloat16).float().t()).to(x.dtype).reshape(x.shape) if ctx.needs_input_grad[0] else None
        dw = (xb.t() @ g).to(w.dtype) if ctx.needs_input_grad[4] else None
        db = g.sum(0).to(b.dtype) if (b is not None and ctx.needs_input_grad[1]) else None
        return dx, db, None, None, dw


def supported(x: torch.Tensor, w: torch.Tensor) -> bool:
    K, N = w.shape
    return x.is_cuda and K % 128 == 0 and N % 8 == 0 and x.shape[-1] == K


def linear_fp8(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], relu: bool,
               out_dtype: torch.dtype) -> torch.Tensor:
    """Local (per-shard) fp8 dense: HIP block-scaled MFMA on GPU, exact emulation on CPU."""
    if x.is_cuda:
        if not supported(x, w):
            raise ValueError(f"fp8 dense needs K % 128 == 0 and N % 8 == 0, got x {tuple(x.shape)} w {tuple(w.shape)}")
        return _Fp8Linear.apply(x, b, None, relu, out_dtype, w)
    return _Fp8LinearRef.apply(x, b, relu, out_dtype, w)


def fp8_dense(x, w, bias=None, relu: bool = False, out_dtype=torch.bfloat16):
    """Global-view ``relu?(x @ w + b)`` on sharded arrays with MX-fp8 forward GEMMs; the
    partitioning (weight gathers, partial sums over a sharded contraction) is :func:`core.dense`'s."""
    from . import core
    return core.dense(x, [w], bias, compute_dtype=out_dtype, relu=relu, fp8=True)[0]


# ----------------------------------------------------------------------------- fused FF block
def _weight_q_rows(w: torch.Tensor):
    """Cached MX quantization of ``w`` along its LAST dim (``quant_rows``), per weight version:
    the B operand of a dX GEMM (``dX = dY W^T`` reads W's rows as [n][k]); an optimizer-maintained
    shadow when the weight qualifies (see :func:`_weight_q`)."""
    from . import shadow
    if shadow.mx_eligible(w):
        return shadow.get_mx(w, "QN")
    key = ("rows", w.data_ptr(), tuple(w.shape), w.dtype, w.device)
    ent = _WCACHE.get(key)
    if ent is not None and ent[0] == w._version:
        return ent[1], ent[2]
    q, s = quant_rows(w.detach())
    _WCACHE[key] = (w._version, q, s)
    return q, s


def _quant_grad_rows(dy2: torch.Tensor):
    """(q, s, broadcast): MX-fp8 rows of a gradient.  A broadcast row (stride 0 over rows, the
    cotangent of y.sum()) is quantized once and read by the GEMM for every row (``a_bcast``)."""
    if dy2.stride(0) == 0:
        row = dy2[:1]
        q1, s1 = quant_rows(row if row.is_contiguous() else row.contiguous())
        return q1, s1, True
    q, s = quant_rows(dy2)
    return q, s, False


def _bcast_grad_mx(dy2: torch.Tensor):
    """(bf16 row view [T][M] with stride 0, q [1][M], s [1][M/32]) of a broadcast SCALAR gradient
    (the cotangent of y.sum()) from one launch, or None for any other gradient."""
    T, M = dy2.shape
    if not (dy2.is_cuda and dy2.numel() > 0 and dy2.stride(0) == 0 and dy2.stride(1) == 0 and M % 32 == 0
            and dy2.dtype in (torch.float32, torch.bfloat16)):
        return None
    row = torch.empty((1, M), dtype=torch.bfloat16, device=dy2.device)
    q = torch.empty((1, M), dtype=torch.uint8, device=dy2.device)
    s = torch.empty((1, M // BLOCK), dtype=torch.uint8, device=dy2.device)
    rc = _lib().ljs_bcast_scalar_mx(hip._p(dy2.as_strided((1,), (1,))), int(dy2.dtype == torch.bfloat16), M,
                                    hip._p(row), hip._p(q), hip._p(s), hip._stream(row))
    hip._ck(rc, "bcast_scalar_mx")
    return row.expand(T, M), q, s


def _t_quant(t2: torch.Tensor):
    """(q [C][R], s [C][R/32]): the MX quantization of ``t2`` [R][C] along its ROWS, stored
    transposed -- the K-major operand of a GEMM contracting over R (tokens)."""
    return quant_cols(t2)


def _both_tiles(x2: torch.Tensor) -> bool:
    T, M = x2.shape
    return (x2.is_cuda and x2.dtype in (torch.bfloat16, torch.float32) and T % 128 == 0 and M % 64 == 0
            and x2.stride(1) == 1 and x2.stride(0) % 8 == 0 and x2.data_ptr() % 16 == 0)


def _quant_both(x2: torch.Tensor, xb: Optional[torch.Tensor] = None):
    """((q [T][M], s): row-blocked, (qT [M][T], sT): token-blocked transposed) MX quantizations of
    a bf16 [T][M] in one pass over it (or two passes when the shape does not tile).  An f32 x2
    (tiling shapes only) is rounded to bf16 on load, written to ``xb`` (contiguous bf16 [T][M])
    and quantized from those values."""
    T, M = x2.shape
    if _both_tiles(x2):
        f32 = x2.dtype == torch.float32
        assert (xb is not None) == f32, "an f32 input needs its bf16 destination (and only it)"
        if f32:
            assert xb.dtype == torch.bfloat16 and xb.is_contiguous() and xb.shape == (T, M) and xb.data_ptr() % 16 == 0
        dev = x2.device
        q = torch.empty((T, M), dtype=torch.uint8, device=dev)
        s = torch.empty((T, M // BLOCK), dtype=torch.uint8, device=dev)
        qT = torch.empty((M, T), dtype=torch.uint8, device=dev)
        sT = torch.empty((M, T // BLOCK), dtype=torch.uint8, device=dev)
        rc = _lib().ljs_quant_mx_both(hip._p(x2), x2.stride(0), T, M, hip._p(qT), hip._p(sT), hip._p(q), hip._p(s),
                                      hip._p(xb) if f32 else None, hip._stream(x2))
        hip._ck(rc, "quant_mx_both")
        return (q, s), (qT, sT)
    assert x2.dtype == torch.bfloat16 or not x2.is_cuda
    return quant_rows(x2), _t_quant(x2)


# upper bound on the split count (tuning / A/B: each split is one more f32 slab that the fused Adam
# or the slab reduction reads back)
_MX_SPLIT_MAX = 64


def _pick_split(tiles: int, nkt: int) -> int:
    """Split-K count for an MX weight-gradient GEMM: the most splits keeping the work items within
    two 128x128 blocks per CU (2 x 256), each split at least 8 K-tiles, ceil-consistent."""
    best = 1
    for S in range(1, 65):
        if tiles * S > 512 or nkt < 8 * S or S > _MX_SPLIT_MAX:
            break
        if hip.slab_count(nkt, S) == S:
            best = S
    return best


def _mx_wgrad(qa, sa, qb, sb, M: int, N: int, K: int, b_bcast: bool = False, w=None) -> torch.Tensor:
    """f32 [M][N] = A B^T over K (both operands MX-fp8, K-major, blocks along K), split-K into f32
    slabs summed by one streaming reduction -- or, for the gradient of weight ``w`` inside a
    deferring value_and_grad, left to the fused Adam (ops/linear.defer_slabs)."""
    from .linear import defer_slabs
    S = _pick_split(-(-M // 128) * -(-N // 128), K // 128)
    out = torch.empty((M, N), dtype=torch.float32, device=qa.device)
    if S == 1:
        gemm_mx(qa, sa, qb, sb, M, N, K, out, b_bcast=b_bcast)
        return out
    slabs = torch.empty((S, M, N), dtype=torch.float32, device=qa.device)
    gemm_mx(qa, sa, qb, sb, M, N, K, slabs, b_bcast=b_bcast, nsplit=S)
    defer = defer_slabs(w, out, N) if w is not None else None
    if defer is not None:
        defer(slabs, S, lambda done=[]: done or (hip.slab_reduce(slabs, out, N, 0), done.append(1)))
    else:
        hip.slab_reduce(slabs, out, N, 0)
    return out


class _FFBlockFp8(torch.autograd.Function):
    """``y = relu(x Win) Wout (+ res)`` with ALL FF GEMMs on MX-fp8 block-scaled MFMA and the
    hidden activation kept only in fp8:

    * forward: x quantized per row (the up projection's operand) and per 32-token column block
      (the weight gradient's); the up projection's epilogue writes the ReLU output ONLY as MX-fp8,
      twice -- blocked along features (the down projection's A operand, and the ReLU mask) and
      transposed, blocked along tokens (dW_out's operand) -- the bf16 activation is never stored;
      the down projection's epilogue adds the residual;
    * backward: dY quantized per row (a broadcast dY once, read as one row); dA = dY Wout^T with
      the ReLU mask taken from the e4m3 activation (value > 0), its epilogue writing dA as MX-fp8
      blocked along features (dX's operand) and along tokens (dW_in's operand); dX = dA Win^T
      with the skip path's dY added in its epilogue when the residual is x itself;
      dW_out = A^T dY and dW_in = X^T dA on the MX MFMA too (operands blocked along tokens,
      split-K into f32 slabs + one reduction).

    Per step that moves ~40 % fewer bytes than keeping the bf16 activation and its fp8 copy
    (the up projection's and dA's outputs are half the size), and every FF FLOP runs at the
    fp8 rate.  The host emulation :class:`_FFBlockFp8Ref` is the numerical oracle."""

    @staticmethod
    def forward(ctx, x, w_in, w_out, res):
        M = x.shape[-1]
        F = w_in.shape[1]
        # rows (tokens) in x's STORAGE order (every op of the block is per token except the weight
        # gradients, which sum over all of them): a seq-major activation - the 2-D mesh's out
        # projection output, stored [seq][batch][M] - is read without a transposing copy, and y
        # (and dX) keep that order.  The residual, when it is x, is the same bf16 rows.
        nd = x.dim()
        o = hip.storage_order(x) if x.is_cuda else None
        order = tuple(o) if o is not None and o[-1] == nd - 1 else tuple(range(nd))
        xs = x.permute(order)
        pshape = tuple(xs.shape[:-1])
        xf = xs.reshape(-1, M).contiguous()
        T = xf.shape[0]
        dev = x.device
        # [T][M] blocked along M (the up projection's operand) and [M][T] blocked along T
        # (dW_in's), from one pass over x; an f32 x is rounded to bf16 inside that pass, which
        # also writes the bf16 rows (the residual): no separate cast pass (verdict r5 item 5)
        if xf.dtype == torch.float32 and _both_tiles(xf):
            x2 = torch.empty((T, M), dtype=torch.bfloat16, device=dev)
            (qx, sx), (qxT, sxT) = _quant_both(xf, x2)
        else:
            x2 = _bf16(xf)
            (qx, sx), (qxT, sxT) = _quant_both(x2)
        qwi, swi = _weight_q(w_in)                  # [F][M], blocks along M
        qa = torch.empty((T, F), dtype=torch.uint8, device=dev)
        sa = torch.empty((T, F // BLOCK), dtype=torch.uint8, device=dev)
        qaT = torch.empty((F, T), dtype=torch.uint8, device=dev)
        saT = torch.empty((F, T // BLOCK), dtype=torch.uint8, device=dev)
        gemm_mx(qx, sx, qwi, swi, T, F, M, None, relu=True, qout=(qa, sa), qtout=(qaT, saT))
        qwo, swo = _weight_q(w_out)                 # [M][F], blocks along F
        y = torch.empty((T, M), dtype=torch.bfloat16, device=dev)
        r2 = None
        if res is not None:
            r2 = x2 if res is x else _bf16(res.permute(order).reshape(T, M).contiguous())
        gemm_mx(qa, sa, qwo, swo, T, M, F, y, res=r2)
        ctx.save_for_backward(qa, qaT, saT, qxT, sxT, w_in, w_out)
        ctx.meta = (order, pshape, M, F, T, res is not None, res is x)
        return y.view(pshape + (M,)).permute(_inv_perm(order))

    @staticmethod
    def backward(ctx, dy):
        from .linear import _row_view
        qa, qaT, saT, qxT, sxT, w_in, w_out = ctx.saved_tensors
        order, pshape, M, F, T, has_res, res_is_x = ctx.meta
        dev = qa.device
        dy2 = dy.permute(order).reshape(T, M)       # the forward's row order (a view when dy shares it)
        bm = _bcast_grad_mx2(dy2, T) if ctx.needs_input_grad[2] else _bcast_grad_mx(dy2)
        if bm is not None:                          # scalar broadcast: its rows + MX rows, one launch
            t, qdy, sdy = bm[:3]
            ld, bc = 0, True
        else:
            t, ld = _row_view(dy2, T, M)            # bf16 dY (one row, ld 0, when broadcast)
            qdy, sdy, bc = _quant_grad_rows(t)
        qwo_r, swo_r = _weight_q_rows(w_out)        # Wout [F][M] rows: blocks along M
        qdA = torch.empty((T, F), dtype=torch.uint8, device=dev)
        sdA = torch.empty((T, F // BLOCK), dtype=torch.uint8, device=dev)
        qdAT = torch.empty((F, T), dtype=torch.uint8, device=dev)
        sdAT = torch.empty((F, T // BLOCK), dtype=torch.uint8, device=dev)
        gemm_mx(qdy, sdy, qwo_r, swo_r, T, F, M, None, res=qa, res_mode="mask", qout=(qdA, sdA),
                qtout=(qdAT, sdAT), a_bcast=bc)
        out = {}
        fold = has_res and res_is_x and ctx.needs_input_grad[0]
        if ctx.needs_input_grad[0]:
            qwi_r, swi_r = _weight_q_rows(w_in)     # Win [M][F] rows: blocks along F
            dx = torch.empty((T, M), dtype=torch.bfloat16, device=dev)
            # the skip path's dY summed in the epilogue (bf16(bf16(dx) + dY), the unfused add);
            # on the 8-wave tiles the epilogue also writes dx's column sums per row tile: the bias
            # gradient of the dense that produced x (a transformer layer's out projection) is then
            # one small reduction, computed only if that backward asks (hip.colsum_for)
            tile = _auto_tile(T, M, F, MX_RES_ADD if fold else 0, 1)
            cs = None
            if tile >= 10000 and _FUSED_COLSUM:
                rows = tile % 1000000 // 1000
                cs = torch.empty((-(-T // rows), M), dtype=torch.float32, device=dev)
            gemm_mx(qdA, sdA, qwi_r, swi_r, T, M, F, dx, res=t if fold else None, res_mode="add", tile=tile,
                    colsum=cs)
            if cs is not None:
                hip.register_colsum(dx, _lazy_rows_sum(cs))
            out["dx"] = dx.view(pshape + (M,)).permute(_inv_perm(order))
        if ctx.needs_input_grad[2]:
            # dY blocked along tokens: one constant row for a broadcast scalar, else a column pass
            if bm is not None:
                qdyT, sdyT = bm[3], bm[4]
                dwo = _mx_wgrad(qaT, saT, qdyT, sdyT, F, M, T, b_bcast=True, w=w_out)
            else:
                qdyT, sdyT = _t_quant(t)
                dwo = _mx_wgrad(qaT, saT, qdyT, sdyT, F, M, T, w=w_out)
            out["wo"] = dwo
        if ctx.needs_input_grad[1]:
            out["wi"] = _mx_wgrad(qxT, sxT, qdAT, sdAT, M, F, T, w=w_in)
        dres = dy if (has_res and ctx.needs_input_grad[3] and not fold) else None
        return out.get("dx"), out.get("wi"), out.get("wo"), dres


_FUSED_COLSUM = True


def _lazy_rows_sum(cs: torch.Tensor):
    """f32 [N] = sum over the rows of ``cs`` [R][N], computed on first use (one short-matrix row sum)."""
    done = []

    def get():
        if not done:
            # (one short-matrix pass over the row-tile partials: the long-R column-sum kernel ran
            # 3 workgroups for 21 us here, slab_reduce one workgroup for 10 us)
            done.append(hip.rows_sum(cs))
        return done[0]
    return get


def _bcast_grad_mx2(dy2: torch.Tensor, n: int):
    """:func:`_bcast_grad_mx` plus the MX row of length ``n`` (the token-blocked dY^T row), one
    launch; None unless ``dy2`` is a broadcast scalar."""
    T, M = dy2.shape
    if not (dy2.is_cuda and dy2.numel() > 0 and dy2.stride(0) == 0 and dy2.stride(1) == 0 and M % 32 == 0
            and n % 32 == 0 and dy2.dtype in (torch.float32, torch.bfloat16)):
        return None
    dev = dy2.device
    row = torch.empty((1, M), dtype=torch.bfloat16, device=dev)
    q1 = torch.empty((1, M), dtype=torch.uint8, device=dev)
    s1 = torch.empty((1, M // BLOCK), dtype=torch.uint8, device=dev)
    q2 = torch.empty((1, n), dtype=torch.uint8, device=dev)
    s2 = torch.empty((1, n // BLOCK), dtype=torch.uint8, device=dev)
    rc = _lib().ljs_bcast_scalar_mx2(hip._p(dy2.as_strided((1,), (1,))), int(dy2.dtype == torch.bfloat16), M,
                                     hip._p(row), hip._p(q1), hip._p(s1), n, hip._p(q2), hip._p(s2), hip._stream(row))
    hip._ck(rc, "bcast_scalar_mx2")
    return row.expand(T, M), q1, s1, q2, s2


def _bcast_row_mx(dy2: torch.Tensor, n: int):
    """(q [1][n], s [1][n/32]): the MX row of a broadcast scalar gradient repeated n times (the
    tokens-blocked dY^T of y.sum(), read as one row for every output column)."""
    row = torch.empty((1, n), dtype=torch.bfloat16, device=dy2.device)
    q = torch.empty((1, n), dtype=torch.uint8, device=dy2.device)
    s = torch.empty((1, n // BLOCK), dtype=torch.uint8, device=dy2.device)
    rc = _lib().ljs_bcast_scalar_mx(hip._p(dy2.as_strided((1,), (1,))), int(dy2.dtype == torch.bfloat16), n,
                                    hip._p(row), hip._p(q), hip._p(s), hip._stream(row))
    hip._ck(rc, "bcast_scalar_mx")
    return q, s


def _deq_rows(t: torch.Tensor) -> torch.Tensor:
    """MX quantize -> dequantize along the last dim (f32)."""
    return dequantize_mx_ref(*quantize_mx_ref(t.float()))


class _FFBlockFp8Ref(torch.autograd.Function):
    """Host emulation of :class:`_FFBlockFp8` (quantize -> dequantize -> f32 matmul, the same
    roundings in the same places, including the token-blocked weight-gradient operands and the
    ReLU mask read from the e4m3 activation)."""

    @staticmethod
    def forward(ctx, x, w_in, w_out, res):
        lead, M = x.shape[:-1], x.shape[-1]
        x2 = x.reshape(-1, M).to(torch.bfloat16).float()
        xd = _deq_rows(x2)
        wid = _deq_rows(w_in.t().contiguous())                              # [F][M]
        a = torch.relu(xd @ wid.t()).to(torch.bfloat16).float()            # bf16-rounded ReLU output
        ad = _deq_rows(a)                                                   # the stored e4m3 activation
        wod = _deq_rows(w_out.t().contiguous())                             # [M][F]
        y = (ad @ wod.t()).to(torch.bfloat16)
        if res is not None:
            y = y + res.reshape(y.shape).to(torch.bfloat16)
        ctx.save_for_backward(x2, a, ad, w_in, w_out)
        ctx.meta = (lead, M, res is not None)
        return y.reshape(tuple(lead) + (M,))

    @staticmethod
    def backward(ctx, dy):
        x2, a, ad, w_in, w_out = ctx.saved_tensors
        lead, M, has_res = ctx.meta
        dy2 = dy.reshape(-1, M).to(torch.bfloat16).float()
        dyd = _deq_rows(dy2)
        wod_r = _deq_rows(w_out)                                            # [F][M], blocks along M
        dA = (dyd @ wod_r.t()).to(torch.bfloat16).float()
        dA = torch.where(ad > 0, dA, torch.zeros_like(dA))
        dAd = _deq_rows(dA)
        wid_r = _deq_rows(w_in)                                             # [M][F], blocks along F
        dx = (dAd @ wid_r.t()).to(torch.bfloat16).reshape(tuple(lead) + (M,)) if ctx.needs_input_grad[0] else None
        # weight gradients on token-blocked operands (A^T dY, X^T dA)
        dwo = (_deq_rows(a.t().contiguous()) @ _deq_rows(dy2.t().contiguous()).t()).to(w_out.dtype) \
            if ctx.needs_input_grad[2] else None
        dwi = (_deq_rows(x2.t().contiguous()) @ _deq_rows(dA.t().contiguous()).t()).to(w_in.dtype) \
            if ctx.needs_input_grad[1] else None
        dres = dy if (has_res and ctx.needs_input_grad[3]) else None
        return dx, dwi, dwo, dres


def ff_block_supported(x: torch.Tensor, w_in: torch.Tensor, w_out: torch.Tensor) -> bool:
    """M, F multiples of 128 (MX GEMM K-tiles); the token count a multiple of 128 too (the weight
    gradients contract over tokens)."""
    M, F = w_in.shape
    T = x.numel() // max(1, x.shape[-1])
    return (x.shape[-1] == M and tuple(w_out.shape) == (F, M) and M % 128 == 0 and F % 128 == 0
            and T % 128 == 0)


def ff_block_local(x: torch.Tensor, w_in: torch.Tensor, w_out: torch.Tensor,
                   res: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per-shard fused MX-fp8 FF block (GPU kernels; exact emulation on host devices)."""
    if not ff_block_supported(x, w_in, w_out):
        raise ValueError(f"fp8 FF block needs M, F % 128 == 0: x {tuple(x.shape)} w_in {tuple(w_in.shape)}")
    if x.is_cuda:
        return _FFBlockFp8.apply(x, w_in, w_out, res)
    return _FFBlockFp8Ref.apply(x, w_in, w_out, res)


def ff_block(x, w_in, w_out, residual=None, fp8: bool = True):
    """Global-view fused FF block ``relu(x Win) Wout (+ residual)`` on sharded arrays: x keeps its
    tiling (its feature dim gathered if split), the weights are used replicated (data / FSDP
    meshes; a hidden dim split over a mesh axis takes the two-dense path in ``FeedForward``).
    ``fp8``: the MX-fp8 block (:class:`_FFBlockFp8`); else bf16 (:class:`.linear._FFBlock`, where
    a residual that is x itself is summed into the dX GEMM's epilogue)."""
    from ..sharding.tile import TileAssignment
    from ..spmd.reshard import reshard_tile
    from ..sharding.shardings import sharding_from_tile
    from ..array import ShardedArray
    from . import core
    from . import linear as L
    xt = x.tile
    if xt.tile_shape[-1] > 1:
        x = reshard_tile(x, xt.unshard([x.ndim - 1]), note="ff.x")
        xt = x.tile
    devs = xt.device_ids
    rep = TileAssignment.replicated(devs, 2)
    if fp8 and all(t.is_cuda for t in x.local.values()):
        # sharded weights gathered as their shards' MX-fp8 shadows (a quarter of the f32 bytes,
        # no per-step quantization of the gathered copy; parallel/weight_gather.gather_mx)
        from ..parallel import weight_gather as _wg
        gi, go = _wg.mx_eligible(w_in, rep), _wg.mx_eligible(w_out, rep)
        wi = _wg.gather_mx(w_in, rep, gi, note="ff.w_in") if gi is not None else \
            reshard_tile(w_in, rep, note="ff.w_in")
        wo = _wg.gather_mx(w_out, rep, go, note="ff.w_out") if go is not None else \
            reshard_tile(w_out, rep, note="ff.w_out")
    else:
        wi = reshard_tile(w_in, rep, note="ff.w_in")
        wo = reshard_tile(w_out, rep, note="ff.w_out")
    self_res = residual is x
    r_loc = None
    if residual is not None and not self_res:
        r_loc = reshard_tile(residual, xt, note="ff.residual").local
    core._plan.record("ff_block", fp8=fp8, tiles=xt.tile_shape)
    loc = {}
    for d in x.local:
        xl, wil, wol = x.local[d], wi.local[d], wo.local[d]
        rl = xl if self_res else (r_loc[d] if r_loc is not None else None)
        if fp8:
            loc[d] = ff_block_local(xl, wil, wol, rl)
        elif xl.is_cuda and L.ff_block_supported(xl, wil, wol) and (rl is None or self_res):
            loc[d] = L.ff_block(xl, wil, wol, self_res)
        else:  # host devices / other shapes: the unfused dense pair (same roundings)
            from . import kernels as K
            h = K.linear(xl, [wil], None, torch.bfloat16, relu=True)[0]
            loc[d] = K.linear(h, [wol], None, torch.bfloat16, residual=rl)[0]
    return ShardedArray(tuple(x.shape), torch.bfloat16, sharding_from_tile(xt, like=[x.sharding]), loc)


# ----------------------------------------------------------------------------- tensor-parallel FF block
def ff_block_tp_plan(x, w_in, w_out):
    """``(groups, token_dim)`` when the FF hidden dim is split over a device group: ``w_out``
    ``[F][M]`` tiled ``(tp, *)`` (rule ``('hidden', 'model')``, ``case6_attention.py:186``; a split of
    M as well, e.g. the GSPMD-paper 2-D rules, is gathered) and x
    sharded along one token dim ``token_dim`` tp ways by groups whose members hold all tp hidden
    blocks (the reference's sequence-over-``model`` layout, ``case6_attention.py:161``); else None."""
    wt = w_out.tile
    if wt.ndim != 2 or wt.tile_shape[0] < 2:
        return None
    tp = wt.tile_shape[0]
    xt = x.tile
    if xt.tile_shape[-1] != 1 or set(xt.device_ids) != set(wt.device_ids) or set(w_in.tile.device_ids) != set(
            wt.device_ids):
        return None
    fblk = {d: wt.coords[d][0] for d in wt.device_ids}
    for k in range(x.ndim - 1):
        if xt.tile_shape[k] != tp:
            continue
        gs = xt.groups_along([k])
        if all(sorted(fblk[d] for d in g) == list(range(tp)) for g in gs):
            return gs, k
    return None


def ff_block_tp(x, w_in, w_out, residual=None, fp8: bool = True, plan=None):
    """Global-view FF block with the hidden dim split over a group of tp devices (Megatron-style
    tensor parallelism with a sequence-parallel activation, SURVEY §2.4 "FF-layer TP"):

    * x's token blocks all-gathered over the group (``[.., S/tp, M] -> [.., S, M]``);
    * ``W_in`` column-parallel (``[M][F/tp]``, resharded to the hidden block each device's
      ``W_out`` row block holds), ``W_out`` row-parallel (``[F/tp][M]``, its own layout);
    * every device runs the fused FF block on its hidden slice - with ``fp8`` every GEMM
      (forward, dX and both weight gradients) on the MX-fp8 MFMA, the hidden activation kept only
      in fp8 (:class:`_FFBlockFp8`) - producing a bf16 partial of y;
    * the partials are reduce-scattered over the group back to x's token blocks; the residual is
      added after.

    The backward is the transpose: dY all-gathered over the group, the local block's backward,
    dX reduce-scattered; the weight gradients stay on their hidden slices (``W_in``'s flows back
    through its reshard)."""
    from ..array import ShardedArray
    from ..comm import collectives as C
    from ..sharding.tile import TileAssignment
    from ..spmd.reshard import reshard_tile
    from . import core
    from . import linear as L
    if plan is None:
        plan = ff_block_tp_plan(x, w_in, w_out)
    if plan is None:
        raise ValueError("ff_block_tp: no tensor-parallel layout for these shardings")
    groups, k = plan
    wt = w_out.tile
    tp = wt.tile_shape[0]
    devs = wt.device_ids
    fblk = {d: wt.coords[d][0] for d in devs}
    col = TileAssignment.from_coords({d: (0, fblk[d]) for d in devs}, (1, tp))
    row = TileAssignment.from_coords({d: (fblk[d], 0) for d in devs}, (tp, 1))
    core._plan.record("ff_block_tp", fp8=fp8, tp=tp, token_dim=k, groups=tuple(tuple(g) for g in groups))
    xg = reshard_tile(x, x.tile.unshard([k]), note="ff_tp.x")
    wi = reshard_tile(w_in, col, note="ff_tp.w_in")
    wo = reshard_tile(w_out, row, note="ff_tp.w_out")
    part = {}
    for d in xg.local:
        xl, wil, wol = xg.local[d], wi.local[d], wo.local[d]
        if fp8:
            part[d] = ff_block_local(xl, wil, wol, None)
        elif xl.is_cuda and L.ff_block_supported(xl, wil, wol):
            part[d] = L.ff_block(xl, wil, wol, False)
        else:
            from . import kernels as K
            h = K.linear(xl, [wil], None, torch.bfloat16, relu=True)[0]
            part[d] = K.linear(h, [wol], None, torch.bfloat16)[0]
    loc = C.reduce_scatter(part, groups, dim=k, note="ff_tp.partial_sum")
    y = ShardedArray(tuple(x.shape), torch.bfloat16, x.sharding, loc)
    if residual is not None:
        y = core.binary("add", core.convert(residual, torch.bfloat16), y)
    return y
