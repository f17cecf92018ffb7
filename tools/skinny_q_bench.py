#!/usr/bin/env python3
"""A/B timing of the packed skinny GEMM (skinny_gemm_qi through mia_op_skinny_gemm) at 4, 6 and 8 bits in ONE process: interleaved
rounds, device events, random codes.  Default shape: a Llama-1B gate|up matrix (N 16384, K 2048, SK_SWIGLU), rows 1 and 8.

The matrix at any width fits the Infinity Cache, so every launch of a round reads another of --copies copies (together larger than the
cache): the time is that of a weight stream from HBM, as in a decode step that walks a whole model.  Reported per width: median us per
launch over the rounds (the first round is dropped), and the effective TB/s over the bytes the kernel streams -- N K bits / 8 of codes
plus the fp32 (scale, offset) pairs, 8 bytes per 64 weights."""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mlx_swift_audio_amd as m  # noqa: E402
from mlx_swift_audio_amd import checkpoint, ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=16384)
    ap.add_argument("--K", type=int, default=2048)
    ap.add_argument("--rows", type=int, nargs="*", default=[1, 8])
    ap.add_argument("--bits", type=int, nargs="*", default=[4, 6, 8])
    ap.add_argument("--copies", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--passes", type=int, default=8, help="walks over the copies per timed window")
    a = ap.parse_args()
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
