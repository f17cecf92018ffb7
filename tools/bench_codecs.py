"""Codec-only timing (SNAC / DAC / HiFT decode) -- the `codec` object of bench.py without the Whisper pass; used under rocprofv3.

--stacked: time per utterance of the stacked decode (mia_snac_decode_batch / mia_dac_decode_batch) next to the loop of single calls,
same process, same device-resident inputs: the Orpheus chunk (171 frames, snac_24khz) 1, 8 and 32 at a time and 10 s of DAC speech
(750 steps) 1 and 8 at a time.  Each figure is a window of WINDOW utterances between two device events; the two forms alternate,
--repeats windows each (min / median / max reported), after a warm-up of both at that size; the stacked waveforms are compared with
the single calls' bit for bit before anything is timed.  --sweep-budget adds the stacked form at two other stack budgets."""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import mlx_swift_audio_amd as M  # noqa: E402

WINDOW = 64          # utterances per timed window (a window of one call would time the clock as much as the kernels)


def _spread(ms):
    ms = sorted(ms)
    return {"min": round(ms[0], 3), "median": round(ms[len(ms) // 2], 3), "max": round(ms[-1], 3)}


def _compare(ctx, name, sizes, single, batch, outputs, repeats, set_budget=None, budgets=(-1,)):
    """single(u) decodes utterance u alone, batch(n) the first n in one call; outputs(n) -> (single pcm, stacked pcm) device tensors."""
    res = {}
    for n in sizes:
        for u in range(n):
            single(u)
        batch(n)
        torch.cuda.synchronize()
        a, b = outputs(n)
        identical = bool(torch.equal(a, b))
        calls = max(1, WINDOW // n)
        forms = ["serial"] + [f"stacked_budget_{b >> 20}MiB" if b >= 0 else "stacked" for b in budgets]
        t = {f: [] for f in forms}
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(repeats):
            for fi, form in enumerate(forms):
                if fi and set_budget:
                    set_budget(budgets[fi - 1])
                e0.record()
                for _ in range(calls):
                    if form == "serial":
                        for u in range(n):
                            single(u)
                    else:
                        batch(n)
                e1.record()
                torch.cuda.synchronize()
                t[form].append(e0.elapsed_time(e1) / (calls * n))
        res[f"{name}_x{n}"] = {**{"ms_per_utterance_" + f: _spread(t[f]) for f in forms},
                               "stacked_over_serial_median": round(_spread(t["stacked"])["median"] / _spread(t["serial"])["median"], 3),
                               "bit_identical": identical, "repeats": repeats, "utterances_per_window": calls * n}
        if set_budget:
            set_budget(-1)
    return res


def stacked_bench(ctx, repeats, budgets):
    from mlx_swift_audio_amd import codec as HC
    from mlx_swift_audio_amd import synthetic as S
    lib = ctx.lib
    rng = np.random.default_rng(7)
    res = {}
    # ---- SNAC: NMAX different utterances of 171 frames each
    cfg = S.SNAC_CONFIGS["snac_24khz"]
    dec = HC.SNACDecoder.load(ctx, cfg, S.snac_weights(cfg, 0))
    NMAX, N, T0 = 32, 171, 171 * 4
    n_noise, n_out = dec.noise_len(T0), dec.output_len(T0)
    per = [N * (4 // s) for s in cfg.vq_strides]
    codes = torch.from_numpy(rng.integers(0, cfg.codebook_size, (NMAX, sum(per))).astype(np.int32)).cuda()
    noise = torch.randn(NMAX, n_noise, device="cuda")
    pcm1, pcmb = torch.zeros(NMAX, n_out, device="cuda"), torch.zeros(NMAX, n_out, device="cuda")
    n_codes = np.tile(np.asarray(per, np.int32), (NMAX, 1))
    lvl = np.concatenate([[0], np.cumsum(per)[:-1]])
    ptrs = [(C.c_void_p * 3)(*[codes[u].data_ptr() + 4 * int(o) for o in lvl]) for u in range(NMAX)]
    off = np.arange(NMAX + 1, dtype=np.int64) * n_out
    ns, nsb = C.c_int64(0), np.zeros(NMAX, np.int64)

    def snac_single(u):
        ctx.check(lib.mia_snac_decode(dec.h, ptrs[u], n_codes[u].ctypes.data, 3, noise[u].data_ptr(), n_noise, pcm1[u].data_ptr(), n_out, C.byref(ns), 1))

    def snac_batch(n):
        ctx.check(lib.mia_snac_decode_batch(dec.h, n, codes.data_ptr(), n_codes.ctypes.data, 3, noise.data_ptr(), n * n_noise, pcmb.data_ptr(),
                                            off.ctypes.data, nsb.ctypes.data, 1))

    res.update(_compare(ctx, "snac_24khz_171_frames", (1, 8, 32), snac_single, snac_batch, lambda n: (pcm1[:n], pcmb[:n]), repeats, dec.set_stack_budget, budgets))
    dec.close()
    del pcm1, pcmb, noise
    # ---- DAC: 750 steps
    dcfg = S.DAC_CONFIGS["dac_speech"]
    dd = HC.DACCodec.load(ctx, dcfg, S.dac_weights(dcfg, 0))
    DMAX, T = 8, 750
    d_out = dd.output_len(T)
    dcodes = torch.from_numpy(rng.integers(0, dcfg.codebook_size, (DMAX, dcfg.n_codebooks, T)).astype(np.int32)).cuda()
    d1, db = torch.zeros(DMAX, d_out, device="cuda"), torch.zeros(DMAX, d_out, device="cuda")
    Ts, doff = np.full(DMAX, T, np.int64), np.arange(DMAX + 1, dtype=np.int64) * d_out

    def dac_single(u):
        ctx.check(lib.mia_dac_decode(dd.h, dcodes[u].data_ptr(), dcfg.n_codebooks, T, d1[u].data_ptr(), d_out, C.byref(ns), 1))

    def dac_batch(n):
        ctx.check(lib.mia_dac_decode_batch(dd.h, n, dcodes.data_ptr(), dcfg.n_codebooks, Ts.ctypes.data, db.data_ptr(), doff.ctypes.data, nsb.ctypes.data, 1))

    res.update(_compare(ctx, "dac_speech_750_steps", (1, 8), dac_single, dac_batch, lambda n: (d1[:n], db[:n]), repeats, dd.set_stack_budget, budgets))
    dd.close()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--stacked", action="store_true", help="stacked decode (N utterances in one call) against the loop of single calls")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sweep-budget", action="store_true", help="also time the stacked form with the stack budget at 0 (only stage 0 stacked) and "
                    "at 64 GiB (every stage stacked), next to the handle's default (mia_codec_set_stack_budget)")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)
    ctx = M.Context(stream=st.cuda_stream)
    budgets = (-1, 0, 64 << 30) if args.sweep_budget else (-1,)
    print(json.dumps(stacked_bench(ctx, max(3, args.repeats), budgets) if args.stacked else bench.codec_bench(ctx, torch)))
