#!/usr/bin/env python3
"""OuteTTS on one MI355X: a Llama-3.2-1B-shaped LM (random-init bf16, synthetic.LM_CONFIGS["llama-3.2-1b"]) behind a speaker-profile
prompt, plus the synthetic 24 kHz DAC of tools/bench_codecs.py.  The profile is drawn from a seed with the bundled default speaker's
counts (26 words, 759 code pairs; --words / --pairs change them) and tokenised by a character-level stand-in tokenizer, so the prompt is
somewhat longer than the ~1 900 ids a BPE tokenizer gives.

Prints one JSON line:
  * the prompt length;
  * the prompt pass (CausalLM.forward of the whole prompt: batched pass + the last position's step + the logits copy) with
    set_prompt_attention(0) and (1), alternated in one process, at that length and at 512 and 4 096 rows: synchronised host clock,
    one warm-up of each mode first, then --repeats (>= 3) timed runs each -- min / median / max in ms;
  * max |delta| / sigma of the last-position logits between the two modes at each length;
  * ms per generated token (one sentence) and per step with 8 sentences side by side, with mode 1;
  * the DAC decode of --frames code frames, host inclusive.

--speaker SECONDS WORDS measures speaker-profile creation instead (and nothing else): a synthetic clip of SECONDS at 24 kHz cut into
WORDS equal words, on the dac_speech shape with random-init weights.  Per stage -- preprocess (SpeakerAudio), DAC encode of the resident
clip, features of the clip and all words in one call -- the median of 5 host-inclusive runs after 2 warm-ups, the feature stage's kernel
launch count, and the float64 numpy restatement of the feature stage (tests/_outetts_speaker_ref.py) timed once on this host for scale.

--packed-prompt BITS measures the packed prompt pass instead (and nothing else): the layer Linears quantised (group 64, BITS = 4 | 6 | 8;
the vocabulary head stays 16-bit) and attached to a handle loaded from the de-quantised tensors, then CausalLM.forward of 512, 2 087 and
4 096 random ids (--lengths changes them) with set_prompt_weights(False) -- the 16-bit prompt pass, what every earlier build ran -- and
(True) alternated in one process, tiled prompt attention in both: one warm-up of each, then --repeats (>= 7) timed runs each, min /
median / max in ms; max |delta| / sigma of the last-position logits between the two; weight_bytes() before and after release_dense(),
and the packed prompt pass once more after the release.

--vocab: the reference reads the vocabulary size from the checkpoint's config.json; the default (128 256, Llama-3.2's) is an assumption."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dataclasses  # noqa: E402

import _outetts_ref as R  # noqa: E402  (the stand-in tokenizer and the seeded profile)
import mlx_swift_audio_amd as m  # noqa: E402
from mlx_swift_audio_amd import codec as HC, lm as HL, outetts as OT, synthetic as S  # noqa: E402


def spread(ms):
    ms = sorted(ms)
    return {"min": round(ms[0], 3), "median": round(ms[len(ms) // 2], 3), "max": round(ms[-1], 3)}


def speaker(seconds: float, n_words: int, seed: int):
    import _outetts_speaker_ref as SR
    sr = 24000
    n = int(seconds * sr)
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    env = 0.5 * (1 + np.sin(2 * np.pi * 1.3 * t))
    x = (0.3 * env * np.sin(2 * np.pi * (140 + 6 * np.sin(t)) * t) + 0.1 * env * np.sin(2 * np.pi * 1900 * t) + 0.02 * rng.standard_normal(n)).astype(np.float32)
    edges = np.linspace(0.0, seconds, n_words + 1)
    words = [("w%d" % i, float(edges[i]), float(edges[i + 1])) for i in range(n_words)]
    ctx = m.Context(0)
    dcfg = S.DAC_CONFIGS["dac_speech"]
    dac = HC.DACCodec.load(ctx, dcfg, S.dac_weights(dcfg, 0))

    def median_ms(f, keep=None):
        ts = []
        for i in range(7):                               # 2 warm-ups, then 5
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = f()
            ctx.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
            if keep is not None:
                keep(out)
        return spread(ts[2:])

    made = []
    pre = median_ms(lambda: OT.SpeakerAudio(ctx, x, sr), made.append)
    for sa in made[:-1]:
        sa.close()
    sa = made[-1]
    enc = median_ms(lambda: dac.encode(sa))
    codes = dac.encode(sa)
    sl = OT.slice_words(words, codes.shape[1], n, sr)
    segs = [(0, n)] + [(w.a_start, w.a_end - w.a_start) for w in sl]
    feat = median_ms(lambda: sa.features(segs))
    launches = sa.launches
    whole = median_ms(lambda: OT.OuteTTSAudioProcessor(ctx, dac, sr).create_speaker_from_transcription(x, "bench", words))
    p = sa.read()
    t0 = time.perf_counter()
    for s0, ln in segs:
        SR.raw_features(p[s0:s0 + ln], sr)
    ref_ms = (time.perf_counter() - t0) * 1e3
    print(json.dumps({"speaker": {"seconds": seconds, "samples": n, "words": n_words, "codes": int(codes.shape[1]), "preprocess_ms": pre,
                                  "dac_encode_ms": enc, "features_ms": feat, "feature_launches": launches,
                                  "create_speaker_from_transcription_ms": whole, "features_numpy_float64_ms": round(ref_ms, 1)}}))
    sa.close()
    dac.close()
    ctx.close()


def packed_prompt(args):
    from mlx_swift_audio_amd import checkpoint as CK
    bits, reps = args.packed_prompt, max(7, args.repeats)
    lengths = [int(x) for x in args.lengths] if args.lengths != [512, 4096] else [512, 2087, 4096]
    cfg = dataclasses.replace(S.LM_CONFIGS["llama-3.2-1b"], vocab=args.vocab)
    ctx = m.Context(0)
    t0 = time.time()
    dense = S.lm_weights(cfg, seed=args.seed, dtype=np.float16)
    packed = {}
    for k in [k for k in dense if k.endswith("_proj.weight")]:
        q, s, b = CK.quantize_affine(np.asarray(dense[k], np.float32), 64, bits, np.float16)
        packed[k], packed[k[:-7] + ".scales"], packed[k[:-7] + ".biases"] = q, s, b
        dense[k] = CK.dequantize_affine(ctx, q, s, b, 64, bits).astype(np.float16)
    model = HL.CausalLM.load(ctx, cfg, dense, m.BF16)
    model.attach_q4(packed, bits=bits)
    model.set_prompt_attention(1)
    print(f"[outetts] weights generated, quantised, loaded and attached in {time.time() - t0:.1f}s", file=sys.stderr, flush=True)
    rng = np.random.default_rng(args.seed)
    res = {"model": "llama-3.2-1b", "vocab": cfg.vocab, "bits": bits, "repeats": reps, "prompt_attention": 1}

    def forward_ms(ids, on):
        model.set_prompt_weights(on)
        model.reset()
        torch.cuda.synchronize()
        t = time.perf_counter()
        lg = model.forward(ids)                      # synchronises before it returns
        return (time.perf_counter() - t) * 1e3, lg

    ids_of = {n: rng.integers(0, cfg.vocab, n).tolist() for n in lengths}
    passes = {}
    for n in lengths:
        lg = {on: forward_ms(ids_of[n], on)[1] for on in (False, True)}
        t = {False: [], True: []}
        for _ in range(reps):
            for on in (False, True):
                t[on].append(forward_ms(ids_of[n], on)[0])
        passes[str(n)] = {"rows": n, "dense16_ms": spread(t[False]), "packed_ms": spread(t[True]),
                          "packed_over_dense16_median": round(spread(t[True])["median"] / spread(t[False])["median"], 2),
                          "logits_max_delta_over_sigma": round(float(np.abs(lg[True] - lg[False]).max() / lg[False].std()), 5)}
        print(f"[outetts] packed prompt pass {n}: {passes[str(n)]}", file=sys.stderr, flush=True)
    res["prompt_pass"] = passes
    res["weight_bytes_before_release"] = dict(zip(("dense", "packed"), model.weight_bytes()))
    model.release_dense()
    res["weight_bytes_after_release"] = dict(zip(("dense", "packed"), model.weight_bytes()))
    res["packed_ms_after_release"] = {str(n): spread([forward_ms(ids_of[n], True)[0] for _ in range(reps)]) for n in lengths}
    model.close()
    ctx.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--vocab", type=int, default=128256, help="vocabulary size (an assumption: the checkpoint's config.json is not at hand)")
    ap.add_argument("--words", type=int, default=26)
    ap.add_argument("--pairs", type=int, default=759)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--new-tokens", type=int, default=128)
    ap.add_argument("--frames", type=int, default=300, help="DAC code frames to decode (75 per second)")
    ap.add_argument("--lengths", type=int, nargs="*", default=[512, 4096])
    ap.add_argument("--speaker", nargs=2, metavar=("SECONDS", "WORDS"), help="measure speaker-profile creation only")
    ap.add_argument("--packed-prompt", type=int, metavar="BITS", help="measure the prompt pass on packed weights only")
    args = ap.parse_args()
    if args.speaker:
        return speaker(float(args.speaker[0]), int(args.speaker[1]), args.seed)
    if args.packed_prompt:
        return packed_prompt(args)
    reps = max(3, args.repeats)
    cfg = dataclasses.replace(S.LM_CONFIGS["llama-3.2-1b"], vocab=args.vocab)
    ctx = m.Context(0)
    t0 = time.time()
    model = HL.CausalLM.load(ctx, cfg, S.lm_weights(cfg, seed=args.seed, dtype=np.float16), m.BF16)
    print(f"[outetts] weights generated and loaded in {time.time() - t0:.1f}s", file=sys.stderr, flush=True)
    proc = R.processor()
    spk = R.seeded_speaker(args.seed, args.words, args.pairs)
    prompt = proc.get_completion_prompt_tokens("The first snow of the year fell quietly over the harbour.", spk)
    rng = np.random.default_rng(args.seed)
    res = {"model": "llama-3.2-1b", "vocab": cfg.vocab, "speaker_words": args.words, "speaker_pairs": args.pairs, "prompt_tokens": len(prompt), "repeats": reps}

    def forward_ms(ids, mode):
        model.set_prompt_attention(mode)
        model.reset()
        torch.cuda.synchronize()
        t = time.perf_counter()
        lg = model.forward(ids)                      # synchronises before it returns
        return (time.perf_counter() - t) * 1e3, lg

    passes = {}
    for n in [len(prompt)] + [int(x) for x in args.lengths]:
        ids = prompt if n == len(prompt) else rng.integers(0, R.VOCAB, n).tolist()
        lg = {mode: forward_ms(ids, mode)[1] for mode in (0, 1)}                 # warm-up of both modes at this length
        t = {0: [], 1: []}
        for _ in range(reps):
            for mode in (0, 1):
                t[mode].append(forward_ms(ids, mode)[0])
        passes[str(n)] = {"rows": n, "mode0_ms": spread(t[0]), "mode1_ms": spread(t[1]),
                          "mode0_over_mode1_median": round(spread(t[0])["median"] / spread(t[1])["median"], 2),
                          "logits_max_delta_over_sigma": round(float(np.abs(lg[1] - lg[0]).max() / lg[0].std()), 5)}
        print(f"[outetts] prompt pass {n}: {passes[str(n)]}", file=sys.stderr, flush=True)
    res["prompt_pass"] = passes

    # ---- generation with mode 1: one sentence, then 8 side by side
    model.set_prompt_attention(1)
    n_new, stop = args.new_tokens, (cfg.vocab - 1,)
    kw = dict(temperature=0.4, top_p=0.9, rep_penalty=OT.REPETITION_PENALTY, rep_window=OT.REPETITION_CONTEXT_SIZE, stop_ids=stop)
    u = rng.random(n_new).astype(np.float32)
    model.generate(prompt, u, max_new_tokens=16, **kw)                           # warm-up + graph capture

    def timed(f):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = f()
        return (time.perf_counter() - t) * 1e3, out

    one = [timed(lambda: model.generate(prompt, u, max_new_tokens=1, **kw))[0] for _ in range(3)]
    full = [timed(lambda: model.generate(prompt, u, max_new_tokens=n_new, **kw)) for _ in range(3)]
    steps = len(full[0][1]) - 1
    res["generate"] = {"new_tokens": len(full[0][1]), "prompt_plus_first_token_ms": spread(one), "total_ms": spread([f[0] for f in full]),
                       "ms_per_token": round((spread([f[0] for f in full])["median"] - spread(one)["median"]) / max(steps, 1), 4)}
    B = 8
    model.set_batch(B)
    model.set_prompt_attention(1)
    prompts = [proc.get_completion_prompt_tokens(f"Sentence number {b} of the batch.", spk) for b in range(B)]
    ub = rng.random((B, n_new)).astype(np.float32)
    model.generate_batch(prompts, ub, max_new_tokens=16, **kw)
    one_b = [timed(lambda: model.generate_batch(prompts, ub, max_new_tokens=1, **kw))[0] for _ in range(3)]
    full_b = [timed(lambda: model.generate_batch(prompts, ub, max_new_tokens=n_new, **kw)) for _ in range(3)]
    ntok = sum(len(o) for o in full_b[0][1])
    med_b = spread([f[0] for f in full_b])["median"]
    res["generate_x8"] = {"sequences": B, "prompt_rows": sum(len(p) - 1 for p in prompts), "prompts_plus_first_token_ms": spread(one_b), "total_ms": spread([f[0] for f in full_b]),
                          "ms_per_step": round((med_b - spread(one_b)["median"]) / max(n_new - 1, 1), 4), "tokens_per_s": round(ntok / med_b * 1e3, 1)}
    model.set_prompt_attention(0)
    one_b0 = [timed(lambda: model.generate_batch(prompts, ub, max_new_tokens=1, **kw))[0] for _ in range(4)][1:]
    res["generate_x8"]["prompts_plus_first_token_ms_mode0"] = spread(one_b0)
    model.close()

    # ---- DAC decode
    dcfg = S.DAC_CONFIGS["dac_speech"]
    dac = HC.DACCodec.load(ctx, dcfg, S.dac_weights(dcfg, 0))
    codes = rng.integers(0, dcfg.codebook_size, (1, dcfg.n_codebooks, args.frames)).astype(np.int32)
    dac.decode_from_codes(codes)
    d = [timed(lambda: dac.decode_from_codes(codes)) for _ in range(5)]
    res["dac_decode"] = {"frames": args.frames, "samples": int(d[0][1].size), "host_inclusive_ms": spread([x[0] for x in d])}
    dac.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
