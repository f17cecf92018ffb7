#!/usr/bin/env python3
"""A/B timing of the packed skinny GEMM (skinny_gemm_qi through mia_op_skinny_gemm) at 4, 6 and 8 bits in ONE process: interleaved
rounds, device events, random codes.  Default shape: a Llama-1B gate|up matrix (N 16384, K 2048, SK_SWIGLU), rows 1 and 8.

The matrix at any width fits the Infinity Cache, so every launch of a round reads another of --copies copies (together larger than the
cache): the time is that of a weight stream from HBM, as in a decode step that walks a whole model.  Reported per width: median us per
launch over the rounds (the first round is dropped), and the effective TB/s over the bytes the kernel streams -- N K bits / 8 of codes
plus the fp32 (scale, offset) pairs, 8 bytes per 64 weights.

--packed-prompt measures the many-row packed GEMM instead (gemm_quant.hip through mia_op_gemm_quant): --prompt-rows rows (default 512) of
the same gate|up matrix at each width against mia_op_linear (fp32 output) on the de-quantised matrix rounded to bf16, interleaved rounds
in one process, device events around --passes back-to-back launches, median of --rounds (>= 7) rounds after one dropped round.  The
operands stay resident in the caches here, as in a prompt pass that multiplies hundreds of rows per weight read: the figure is
compute time.  Reported: us per launch, TFLOP/s over 2 M N K, and the ratio to the 16-bit GEMM."""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mlx_swift_audio_amd as m  # noqa: E402
from mlx_swift_audio_amd import checkpoint, ops  # noqa: E402


def packed_prompt(a):
    from mlx_swift_audio_amd._abi import GemmQuantDesc
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx = m.Context(0, stream=stream.cuda_stream)
    rng = np.random.default_rng(0)
    M, N, K, rounds = a.prompt_rows, a.N, a.K, max(a.rounds, 7)
    A = torch.randn(M, K, device="cuda").to(torch.bfloat16).view(torch.int16)
    Cq = torch.zeros(M, N, dtype=torch.float32, device="cuda")
    Cd = torch.zeros(M, N, dtype=torch.float32, device="cuda")
    legs = {}
    for bits in a.bits:
        w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
        codes, s, b = checkpoint.quantize_affine(w, 64, bits, np.float16)
        wf, st = ops.quant_repack(codes, s, b, bits, m._lib.F16, m.BF16)
        wf, st = torch.from_numpy(wf.view(np.int32).reshape(-1)).cuda(), torch.from_numpy(st.reshape(-1)).cuda()
        legs[bits] = (wf, st, GemmQuantDesc(A.data_ptr(), K, wf.data_ptr(), st.data_ptr(), bits, Cq.data_ptr(), N, None, 0, M, N, K, m.BF16))
        ops.gemm_quant(ctx, A, wf, st, bits, Cq, M, N, K, m.BF16, lda=K, ldc=N)              # warm-up, through the checked path
    # the 16-bit yardstick: the last width's matrix de-quantised (any values take the same time)
    W16 = torch.from_numpy(checkpoint.dequantize_affine(ctx, codes, s, b, 64, a.bits[-1]).astype(np.float32)).cuda().to(torch.bfloat16).view(torch.int16)

    def dense():
        ctx.check(ctx.lib.mia_op_linear(ctx.h, A.data_ptr(), K, W16.data_ptr(), None, None, 0, Cd.data_ptr(), N, M, N, K, 0, m.BF16, 1, 3, m._lib.MEM_DEVICE))

    dense()
    torch.cuda.synchronize()
    err = float((Cq - Cd).abs().max() / Cd.std())
    calls = {"16-bit": dense}
    for bits in a.bits:
        calls[f"{bits} bit"] = (lambda d: lambda: ctx.check(ctx.lib.mia_op_gemm_quant(ctx.h, C.byref(d))))(legs[bits][2])
    res = {k: [] for k in calls}
    for rnd in range(rounds + 1):
        for k, f in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.passes):
                f()
            e1.record()
            torch.cuda.synchronize()
            if rnd:
                res[k].append(e0.elapsed_time(e1) * 1e3 / a.passes)
    base = float(np.median(res["16-bit"]))
    print(f"M={M} N={N} K={K}, {rounds} rounds x {a.passes} launches; last packed width against the 16-bit GEMM: max |delta| / std = {err:.5f}", flush=True)
    for k, v in res.items():
        us = float(np.median(v))
        print(f"{k}: {us:.1f} us per launch (min {min(v):.1f}, max {max(v):.1f}), {2.0 * M * N * K / us / 1e6:.1f} TFLOP/s, {us / base:.2f} x the 16-bit GEMM", flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=16384)
    ap.add_argument("--K", type=int, default=2048)
    ap.add_argument("--rows", type=int, nargs="*", default=[1, 8])
    ap.add_argument("--bits", type=int, nargs="*", default=[4, 6, 8])
    ap.add_argument("--copies", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--passes", type=int, default=8, help="walks over the copies per timed window")
    ap.add_argument("--packed-prompt", action="store_true", help="the many-row packed GEMM against mia_op_linear")
    ap.add_argument("--prompt-rows", type=int, default=512)
    a = ap.parse_args()
    if a.packed_prompt:
        return packed_prompt(a)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx = m.Context(0, stream=stream.cuda_stream)
    rng = np.random.default_rng(0)
    N, K = a.N, a.K
    W = {}
    for bits in a.bits:
        q = rng.integers(0, 1 << bits, (N, K))
        s = np.full((N, K // 64), 0.01, np.float16)
        b = np.full((N, K // 64), -0.01 * (1 << (bits - 1)), np.float16)
        wf, st = ops.quant_repack(checkpoint.pack_codes(q, bits), s, b, bits, m._lib.F16, m.BF16)
        wf, st = torch.from_numpy(wf.view(np.int32).reshape(-1)).cuda(), torch.from_numpy(st.reshape(-1)).cuda()
        W[bits] = [(wf.clone(), st.clone()) for _ in range(a.copies)]
        print(f"{bits} bit: {wf.numel() * 4 / 1e6:.1f} MB of codes + {st.numel() * 4 / 1e6:.1f} MB of pairs per copy, {a.copies} copies", flush=True)
    for M in a.rows:
        A = torch.randn(M, K, device="cuda").to(torch.bfloat16).view(torch.int16)
        out = torch.zeros(M, N // 2, dtype=torch.int16, device="cuda")
        # one descriptor per (width, copy), launched back to back without a synchronise in between (ops.skinny_gemm drains the stream per call)
        desc = {bits: [ops.SkinnyDesc(A=A.data_ptr(), lda=K, wfrag=wf.data_ptr(), stfrag=st.data_ptr(), out=out.data_ptr(), ldo=N // 2, M=M, N=N, K=K, S=1,
                                      mode=ops.SK_SWIGLU, dtype=m.BF16, bits=bits, rs_scale=1.0) for wf, st in W[bits]] for bits in a.bits}
        for bits in a.bits:      # warm-up, through the checked path
            ops.skinny_gemm(ctx, A=A, M=M, N=N, K=K, mode=ops.SK_SWIGLU, dtype=m.BF16, wfrag=W[bits][0][0], stfrag=W[bits][0][1], bits=bits, out=out)
        res = {bits: [] for bits in a.bits}
        for rnd in range(a.rounds + 1):
            for bits in a.bits:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.passes):
                    for d in desc[bits]:
                        ctx.check(ctx.lib.mia_op_skinny_gemm(ctx.h, C.byref(d)))
                e1.record()
                torch.cuda.synchronize()
                if rnd:
                    res[bits].append(e0.elapsed_time(e1) * 1e3 / (a.copies * a.passes))
        for bits in a.bits:
            us = float(np.median(res[bits]))
            nbytes = N * K * bits / 8 + N * (K // 64) * 8
            print(f"M={M} N={N} K={K} {bits} bit: {us:.2f} us per launch (min {min(res[bits]):.2f}, max {max(res[bits]):.2f}), {nbytes / 1e6:.1f} MB streamed, "
                  f"{nbytes / us / 1e6:.2f} TB/s effective", flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
