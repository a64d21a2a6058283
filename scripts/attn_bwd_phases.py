"""Phase timing of the fused attention backward (attn_bwd_fused_kernel) from shader-clock stamps
(LJS_ATTN_BWD_TRACE build):

    LJS_KERNELS_LIB=learning_jax_sharding_amd/_lib/variants/bwdtrace/libljs_kernels.so \\
        python scripts/attn_bwd_phases.py [B] [kvdma | proj | proj0]

``proj`` / ``proj0``: the instance that forms dO = dY . Wo^T in the block (attn_bwd_proj_kernel; M =
640, a full dY / one broadcast row), whose prologue splits into the GEMM phase (start -> dO image
written, with the K / V / Q / O pieces streaming under it) and the rest (delta of the first block).
Its K-tile steps are stamped too (top of each step, after the barrier): the mean step time over steps
1-11 and over steps 12-19 (of the 20 at M = 640), and the phase's tail (last step's top -> everything
landed).  ``proj0`` runs the broadcast-row phase unless LJS_ATTN_BWD_PROJ_BCAST=0: in that one waves
0-3 stamp each group of four K-tiles after its counted wait, and each group's time is printed.

Per block (averaged over blocks and waves, shader-clock cycles): prologue (start -> first query
block's Q / dO / O and delta ready), each query block of the sweep, and the dK / dV epilogue;
plus how the blocks' start times spread (the second round of blocks starts when the first ends)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from learning_jax_sharding_amd.ops import hip  # noqa: E402


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    if len(sys.argv) > 2 and sys.argv[2] == "kvdma":   # K / V by LDS-DMA beside the first block's
        hip.set_attention_bwd_kv_dma(True)
    H, S, D = 8, 256, 64
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(5)
    qkv = torch.randn(B, S, 3, H, D, generator=g).bfloat16().to(dev)
    q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
    do = torch.randn(B, S, H, D, generator=g).bfloat16().to(dev)
    o, lse = hip.attn_fwd_lse(q, k, v, 0.125)
    mode = sys.argv[2] if len(sys.argv) > 2 else ""
    run = lambda: hip.attn_bwd_block(q, k, v, o, do, lse, 0.125)
    if mode in ("proj", "proj0"):
        M = 640
        hip.set_attention_bwd_proj(True)
        w = (torch.randn(H * D, M, generator=g) * M ** -0.5).bfloat16().to(dev)
        dy = torch.randn(1 if mode == "proj0" else B * S, M, generator=g).bfloat16().to(dev)
        run = lambda: hip.attn_bwd_proj_block(q, k, v, o, dy, 0 if mode == "proj0" else M, w, lse, 0.125)
    for _ in range(5):
        run()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        run()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) / 20 * 1e3
    waves = 8
    trace = torch.zeros((B, H, waves, 8), dtype=torch.int64, device=dev)
    steps = torch.zeros((B, H, waves, 32), dtype=torch.int64, device=dev)
    hip.lib().ljs_attn_set_trace(hip._p(trace))
    hip.lib().ljs_attn_set_trace_steps(hip._p(steps))
    run()
    torch.cuda.synchronize()
    hip.lib().ljs_attn_set_trace(None)
    hip.lib().ljs_attn_set_trace_steps(None)
    t = trace.cpu().double()
    ok = (t[..., 0] > 0) & (t[..., 7] > 0)
    print(f"B={B} {mode}: {B * H} blocks, backward {us:.1f} us; {int(ok.sum())} of {ok.numel()} (block, wave) records")
    if mode in ("proj", "proj0"):
        print(f"  {'GEMM phase':14s} {(t[..., 6] - t[..., 0])[ok].mean().item():8.0f} cycles (of the prologue)")
        # step k = stamp k -> stamp k + 1; stamp nk is the phase's last barrier (everything landed)
        nk = M // 32
        st = steps.cpu().double()
        if hip.attn_bwd_proj_last_path() == 1:
            # the broadcast-row phase: waves 0-3 stamp each group of 4 K-tiles after its counted wait
            ng = -(-nk // 4)
            st, t4, ok4 = st[:, :, :4], t[:, :, :4], ok[:, :, :4]
            d = (st[..., 1:ng + 1] - st[..., :ng])[ok4]      # [records][group]
            print(f"  {'tile groups':14s} (broadcast-row phase, waves 0-3, {ng} groups of 4 K-tiles) first stamp "
                  f"{(st[..., 0] - t4[..., 0])[ok4].mean().item():6.0f} cycles after the start; "
                  + "; ".join(f"group {i} {d[:, i].mean().item():6.0f}" for i in range(ng - 1))
                  + f"; group {ng - 1} and the tail {d[:, ng - 1].mean().item():6.0f}")
        else:
            d = (st[..., 1:nk + 1] - st[..., :nk])[ok]       # [records][step]
            print(f"  {'K-tile steps':14s} first stamp {(st[..., 0] - t[..., 0])[ok].mean().item():6.0f} cycles after the start; "
                  f"step 0 {d[:, 0].mean().item():6.0f}; steps 1-11 {d[:, 1:12].mean().item():6.0f} / step; "
                  f"steps 12-{nk - 2} {d[:, 12:nk - 1].mean().item():6.0f} / step; "
                  f"step {nk - 1} and the tail {d[:, nk - 1].mean().item():6.0f}")
    names = ["prologue"] + [f"query block {i}" for i in range(4)]
    for i, n in enumerate(names):
        d = (t[..., i + 1] - t[..., i])[ok]
        print(f"  {n:14s} {d.mean().item():8.0f} cycles")
    d = (t[..., 7] - t[..., 5])[ok]
    print(f"  {'epilogue':14s} {d.mean().item():8.0f} cycles")
    span = (t[..., 7] - t[..., 0])[ok]
    print(f"  block span {span.mean().item():8.0f} cycles")
    st = t[..., 0][ok]
    en = t[..., 7][ok]
    print(f"  kernel span {(en.max() - st.min()).item():.0f} cycles; block starts: "
          f"first {0:.0f}, median {(st.median() - st.min()).item():.0f}, last {(st.max() - st.min()).item():.0f}")


if __name__ == "__main__":
    main()
