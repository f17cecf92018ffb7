"""GPU: the staging rule of the C ABI (csrc/host_io.h).  Every entry point that takes `int mem` gives the same bytes through host memory
(numpy arrays, the library stages and copies) and through device memory (torch tensors' data_ptr(), nothing copied), in every output,
integer and length outputs included; and a host-memory call that fails after it has queued copies returns with the stream drained and
leaves the handle as it was.  Micro models, the smallest shapes that cross a staging boundary.

Entry points per case (the union is every `int mem` function of include/mia.h; tests/test_host_io_rule.py checks the list):
  front ends      mia_logmel_whisper mia_logmel_s3 mia_mel_s3gen mia_resample_linear mia_resample_sinc mia_dequant_affine
                  mia_sensevoice_features mia_op_funasr_logmel                     (two clips of unequal length where batched)
  operators       mia_op_linear; in-out, T no multiple of 32, padded ld, sentinels: mia_op_linear_epi mia_op_attention_h64
                  mia_op_attention_h64_variant mia_op_attention_h128 mia_op_fsmn_add
  whisper         mia_whisper_encode mia_whisper_get_audio_features mia_whisper_decode_greedy mia_whisper_encode_windows
                  mia_whisper_transcribe_windows mia_whisper_audio_create
  codecs          mia_snac_decode mia_dac_decode mia_dac_decode_batch mia_dac_encode; mia_snac_decode_batch is pinned by
                  tests/test_codec_batch_gpu.py::test_snac_batch_device_memory_equals_host_memory and not repeated here
  sensevoice      mia_sensevoice_encode mia_sensevoice_encode_audio
  s3              mia_s3tok_encode
  hift            mia_hift_f0 mia_hift_source mia_hift_decode mia_hift_vocode mia_hift_vocode_batch   (batch: n = 2, unequal T)
  flow            mia_flow_encode mia_flow_inference mia_flow_inference_streaming mia_flow_inference_batch   (batch: n = 2, unequal T)
  campplus        mia_campplus_fbank mia_campplus_forward mia_campplus_embed
"""
import ctypes as C

import numpy as np
import pytest
import torch          # before the library is loaded: the device-memory half shares the device with torch

from mlx_swift_audio_amd import synthetic as S

pytestmark = pytest.mark.gpu
SENTINEL = 0x7B


class In:
    """An input operand: a numpy array (None = a null pointer)."""
    def __init__(self, a):
        self.a = None if a is None else np.ascontiguousarray(a)


class Out(In):
    """An output operand: the array holds its initial bytes; each run works on a copy."""


class Ptrs:
    """A host array of pointers to operands (const T* const*)."""
    def __init__(self, items):
        self.items = items


def sentinel(shape, dtype):
    return np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, SENTINEL, np.uint8).view(dtype).reshape(shape)


def run(ctx, fn, args, mem, ok=True):
    """fn(*args, mem) with every In / Out placed in host (mem 0) or device (mem 1) memory -> (status, the Out arrays afterwards)."""
    keep, outs = [], []

    def place(o):
        if o.a is None:
            return None
        a = o.a.copy()
        if mem == 0:
            keep.append(a)
            ptr = a.ctypes.data
        else:
            a = torch.from_numpy(a.reshape(-1).view(np.uint8)).cuda()
            keep.append(a)
            ptr = a.data_ptr()
        if isinstance(o, Out):
            outs.append((o, a))
        return ptr

    real = []
    for x in args:
        if isinstance(x, Ptrs):
            arr = (C.c_void_p * len(x.items))(*[place(i) for i in x.items])
            keep.append(arr)
            real.append(arr)
        else:
            real.append(place(x) if isinstance(x, In) else x)
    torch.cuda.synchronize()
    rc = fn(*real, mem)
    if ok:
        ctx.check(rc)
    ctx.synchronize()
    res = [a if mem == 0 else a.cpu().numpy().view(o.a.dtype).reshape(o.a.shape) for o, a in outs]
    return rc, res


def same(ctx, fn, args, extra=lambda: ()):
    """Host and device runs of one call give the same bytes in every Out and the same `extra()` (host-side results such as lengths)."""
    _, host = run(ctx, fn, args, 0)
    eh = tuple(extra())
    _, dev = run(ctx, fn, args, 1)
    ed = tuple(extra())
    assert eh == ed, (fn.__name__, eh, ed)
    assert len(host) == len(dev) and len(host) > 0 or eh
    for i, (h, d) in enumerate(zip(host, dev)):
        assert h.tobytes() == d.tobytes(), f"{fn.__name__}: output {i} differs between host and device memory"
    return host


def clips2(n0=4000, n1=2500):
    c = [S.synth_clip(0, n0).astype(np.float32), S.synth_clip(1, n1).astype(np.float32)]
    return np.concatenate(c), np.asarray([0, n0, n0 + n1], np.int64)


def bf16(a):
    from mlx_swift_audio_amd import audio as A
    return A.f32_to_bf16(np.asarray(a, np.float32))


# ---- front ends ---------------------------------------------------------------------------------------------------------------------

def test_front_ends(ctx):
    import mlx_swift_audio_amd as m
    lib, rng = ctx.lib, np.random.default_rng(1)
    pcm, offs = clips2()
    F = 25
    same(ctx, lib.mia_logmel_whisper, [ctx.h, In(pcm), offs.ctypes.data, 2, 80, 0, F, Out(sentinel((2, F, 80), np.uint16)), m.F16])
    same(ctx, lib.mia_logmel_s3, [ctx.h, In(pcm), offs.ctypes.data, 2, 128, 0, F, Out(sentinel((2, 128, F), np.float32)), m.F32])
    x = pcm[:5001]
    same(ctx, lib.mia_mel_s3gen, [ctx.h, In(x), x.size, Out(sentinel((int(lib.mia_mel_s3gen_frames(x.size)), 80), np.float32))])
    same(ctx, lib.mia_resample_linear, [ctx.h, In(x), x.size, 1.5, Out(sentinel(int(lib.mia_resample_linear_len(x.size, 1.5)), np.float32))])
    N, got = int(lib.mia_resample_sinc_len(x.size, 16000, 24000)), C.c_int64(0)
    same(ctx, lib.mia_resample_sinc, [ctx.h, In(x), x.size, 16000, 24000, Out(sentinel(N, np.float32)), N, C.byref(got)], lambda: (got.value,))
    assert got.value == N
    rows, cols = 3, 128
    wq = rng.integers(0, 2 ** 32, rows * cols * 4 // 32, dtype=np.uint32)
    sc, bi = rng.standard_normal(rows * 2).astype(np.float32), rng.standard_normal(rows * 2).astype(np.float32)
    same(ctx, lib.mia_dequant_affine, [ctx.h, In(wq), In(sc), In(bi), rows, cols, 64, 4, m.F32, Out(sentinel((rows, cols), np.float32)), m.F32])
    n_rows, t = int(lib.mia_sensevoice_feature_rows(offs.ctypes.data, 2)), np.zeros(2, np.int32)
    same(ctx, lib.mia_sensevoice_features, [ctx.h, In(pcm), offs.ctypes.data, 2, Out(sentinel((n_rows, 560), np.float32)), t.ctypes.data, 560],
         lambda: tuple(t))
    frames = sum(1 + int(offs[i + 1] - offs[i]) // 160 for i in range(2))
    same(ctx, lib.mia_op_funasr_logmel, [ctx.h, In(pcm), offs.ctypes.data, 2, Out(sentinel((frames, 80), np.float32))])


# ---- operators ----------------------------------------------------------------------------------------------------------------------

def test_operators(ctx):
    """The four in-out operators keep the bytes they do not write in both modes: sentinel columns past the row, V^T columns past T."""
    import mlx_swift_audio_amd as m
    lib, rng = ctx.lib, np.random.default_rng(2)
    B, T, H, K, Tpad = 2, 36, 1, 64, 64
    D, M = H * 64, B * T
    x, w = bf16(rng.standard_normal((M, K))), bf16(rng.standard_normal((3 * D, K)) / 8)
    bias = rng.standard_normal(3 * D).astype(np.float32)
    same(ctx, lib.mia_op_linear, [ctx.h, In(x), K, In(w), In(bias), In(None), 0, Out(sentinel((M, 3 * D), np.uint16)), 3 * D, M, 3 * D, K, 0, m.BF16, 0, 1])
    ldy = 2 * D + 4
    y, vt = same(ctx, lib.mia_op_linear_epi, [ctx.h, In(x), K, In(w), In(bias), Out(sentinel((M, ldy), np.uint16)), ldy,
                                              Out(sentinel((B, H, 64, Tpad), np.uint16)), M, 3 * D, K, 1, T, H, Tpad, 1, m.BF16, 0, 3])
    s16 = sentinel(1, np.uint16)[0]
    assert (y[:, 2 * D:] == s16).all() and (vt[..., T:] == s16).all() and (y[:, :2 * D] != s16).any() and (vt[..., :T] != s16).any()
    ld_qk, ld_out = 2 * D + 8, D + 4
    qk = sentinel((M, ld_qk), np.uint16)
    qk[:, :2 * D] = bf16(rng.standard_normal((M, 2 * D)))
    v = np.zeros((B, H, 64, Tpad), np.uint16)
    v[..., :T] = bf16(rng.standard_normal((B, H, 64, T)))
    for fn, tail in ((lib.mia_op_attention_h64, []), (lib.mia_op_attention_h64_variant, [1])):
        out, = same(ctx, fn, [ctx.h, In(qk), ld_qk, In(v), Out(sentinel((M, ld_out), np.uint16)), ld_out, B, T, H, Tpad, m.BF16] + tail)
        assert (out[:, D:] == s16).all() and (out[:, :D] != s16).any()
    D8, ld = 128, 128 + 8
    q8, k8, v8 = (np.ascontiguousarray(np.pad(bf16(rng.standard_normal((M, D8))), ((0, 0), (0, 8)))) for _ in range(3))
    seq = np.asarray([T, T - 5], np.int32)
    out, = same(ctx, lib.mia_op_attention_h128, [ctx.h, In(q8), ld, In(k8), ld, In(v8), ld, Out(sentinel((M, D8 + 4), np.uint16)), D8 + 4, B, T, 1,
                                                 float(128 ** -0.5), In(seq), m.BF16])
    assert (out[:, D8:] == s16).all() and (out[T + T - 5:, :] == s16).all() and (out[:T, :D8] != s16).any()       # rows past seq_len too
    Df, Kf, ldx = 64, 11, 64 + 4
    xf = sentinel((M, ldx), np.float32)
    xf[:, :Df] = rng.standard_normal((M, Df)).astype(np.float32)
    vf = np.ascontiguousarray(np.pad(bf16(rng.standard_normal((M, Df))), ((0, 0), (0, 4))))
    wf = (0.3 * rng.standard_normal((Kf, Df))).astype(np.float32)
    out, = same(ctx, lib.mia_op_fsmn_add, [ctx.h, Out(xf), ldx, In(vf), ldx, In(wf), B, T, Df, Kf, 5, In(seq), m.BF16])
    assert out[:, Df:].tobytes() == xf[:, Df:].tobytes() and not np.array_equal(out[:T, :Df], xf[:T, :Df])


# ---- whisper ------------------------------------------------------------------------------------------------------------------------

def test_whisper(ctx):
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import whisper as HW
    from oracle import whisper as OW
    lib = ctx.lib
    dims = OW.DIMS["micro.en"]
    model = HW.WhisperModel.load(ctx, dims, OW.synthetic_weights(dims, seed=5, round_to="f16"), m.F16)
    st = OW.SpecialTokens.for_vocab(dims.n_vocab)
    o = HW.DecodingOptions(suppress_ids=OW.synthetic_suppress_list(st), blank_ids=[220], max_new_tokens=8, max_tokens=32)
    co, keep = model._opts(o)
    B, rows = 2, 2 * dims.n_audio_ctx
    n = rows * 160
    pcm, offs = clips2(n, n // 2 + 77)
    mel = (0.5 * np.random.default_rng(3).standard_normal((B, rows, dims.n_mels))).astype(np.float16)
    results = lambda: [Out(np.zeros((B, o.max_tokens), np.int32)), Out(np.zeros(B, np.int32)), Out(sentinel(B, np.float32)), Out(sentinel(B, np.float32))]
    feats = {}
    for mem in (0, 1):                       # the handle carries state from call to call: each mode runs the chain of calls
        run(ctx, lib.mia_whisper_encode, [model.h, In(mel), B], mem)
        feats[mem] = [run(ctx, lib.mia_whisper_get_audio_features, [model.h, Out(sentinel((B, dims.n_audio_ctx, dims.n_audio_state), dt)), k], mem)[1][0]
                      for dt, k in ((np.float32, m.F32), (np.uint16, m.F16))]
        feats[mem] += run(ctx, lib.mia_whisper_decode_greedy, [model.h, C.byref(co)] + results(), mem)[1]
        run(ctx, lib.mia_whisper_encode_windows, [model.h, In(pcm), offs.ctypes.data, B, n], mem)
        feats[mem] += run(ctx, lib.mia_whisper_get_audio_features, [model.h, Out(sentinel((B, dims.n_audio_ctx, dims.n_audio_state), np.uint16)), m.F16], mem)[1]
        feats[mem] += run(ctx, lib.mia_whisper_transcribe_windows, [model.h, In(pcm), offs.ctypes.data, B, n, C.byref(co)] + results(), mem)[1]
        keep_alive = []
        run(ctx, lambda *a: keep_alive.append(lib.mia_whisper_audio_create(*a)) or 0, [model.h, In(pcm), offs.ctypes.data, B, n], mem)
        assert keep_alive[0], lib.mia_last_error(ctx.h)
        F = int(lib.mia_whisper_audio_frames(keep_alive[0]))
        got = np.empty((B, F, dims.n_mels), np.float32)
        for b in range(B):
            ctx.check(lib.mia_whisper_audio_read(keep_alive[0], b, 0, F, got[b].ctypes.data))
        lib.mia_whisper_audio_free(keep_alive[0])
        feats[mem].append(got)
    assert len(feats[0]) == len(feats[1]) == 12
    for i, (a, b) in enumerate(zip(feats[0], feats[1])):
        assert a.tobytes() == b.tobytes(), f"whisper chain: result {i} differs between host and device memory"
    assert feats[0][3].max() > 0 and feats[0][8].max() > 0                   # token counts: something was decoded
    model.close()


# ---- codecs -------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def snac(ctx):
    from mlx_swift_audio_amd import codec as HC
    cfg = S.SNAC_CONFIGS["snac_micro_cn"]
    dec = HC.SNACDecoder.load(ctx, cfg, S.snac_weights(cfg, seed=3))
    yield cfg, dec
    dec.close()


def _snac_args(cfg, dec, frames, rng, n_noise_delta=0):
    codes = [rng.integers(0, cfg.codebook_size, frames * (cfg.vq_strides[0] // s)).astype(np.int32) for s in cfg.vq_strides]
    T0 = frames * cfg.vq_strides[0]
    noise = rng.standard_normal(dec.noise_len(T0)).astype(np.float32)
    n = np.asarray([c.size for c in codes], np.int32)
    ns = C.c_int64(0)
    cap = dec.output_len(T0) + 3
    args = [dec.h, Ptrs([In(c) for c in codes]), n.ctypes.data, len(codes), In(noise), noise.size + n_noise_delta, Out(sentinel(cap, np.float32)), cap, C.byref(ns)]
    return args, ns, (n, codes)


def test_codecs(ctx, snac):
    from mlx_swift_audio_amd import codec as HC
    lib, rng = ctx.lib, np.random.default_rng(4)
    cfg, dec = snac
    args, ns, keep = _snac_args(cfg, dec, 7, rng)
    pcm, = same(ctx, lib.mia_snac_decode, args, lambda: (ns.value,))
    assert ns.value == pcm.size - 3 and (pcm[ns.value:].view(np.uint8) == SENTINEL).all()
    dcfg = S.DAC_CONFIGS["dac_micro"]
    dac = HC.DACCodec.load(ctx, dcfg, S.dac_weights(dcfg, seed=4))
    T = 7
    codes = rng.integers(0, dcfg.codebook_size, (dcfg.n_codebooks, T)).astype(np.int32)
    cap = dac.output_len(T)
    same(ctx, lib.mia_dac_decode, [dac.h, In(codes), dcfg.n_codebooks, T, Out(sentinel(cap, np.float32)), cap, C.byref(ns)], lambda: (ns.value,))
    Ts = np.asarray([7, 3], np.int64)
    flat = rng.integers(0, dcfg.codebook_size, dcfg.n_codebooks * int(Ts.sum())).astype(np.int32)
    off = np.asarray([0, dac.output_len(7), dac.output_len(7) + dac.output_len(3)], np.int64)
    nsb = np.zeros(2, np.int64)
    same(ctx, lib.mia_dac_decode_batch, [dac.h, 2, In(flat), dcfg.n_codebooks, Ts.ctypes.data, Out(sentinel(int(off[-1]), np.float32)), off.ctypes.data,
                                         nsb.ctypes.data], lambda: tuple(nsb))
    audio = S.synth_clip(2, 1003).astype(np.float32)
    steps = int(lib.mia_dac_code_len(dac.h, audio.size))
    cc, = same(ctx, lib.mia_dac_encode, [dac.h, In(audio), audio.size, 0, Out(sentinel((dcfg.n_codebooks, steps + 2), np.int32)), steps + 2, C.byref(ns)],
               lambda: (ns.value,))
    assert ns.value == steps and (cc[:, steps:].view(np.uint8) == SENTINEL).all() and (cc[:, :steps] < dcfg.codebook_size).all()
    dac.close()


# ---- SenseVoice, S3, HiFT, flow, CAM++ ----------------------------------------------------------------------------------------------

def test_sensevoice(ctx):
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import funasr
    lib = ctx.lib
    cfg = funasr.SENSEVOICE_CONFIGS["sensevoice-micro"]
    sv = funasr.SenseVoiceEncoder.load(ctx, cfg, S.sensevoice_weights(cfg, seed=1, round_to="bf16"), m.BF16)
    t = np.asarray([9, 4], np.int32)
    feats = np.random.default_rng(5).standard_normal((int(t.sum()), cfg.input_dim)).astype(np.float32)
    n_emb = int(((t - 1) // cfg.adaptor_k + 1).sum())
    n = np.zeros(2, np.int32)
    same(ctx, lib.mia_sensevoice_encode, [sv.h, In(feats), t.ctypes.data, 2, Out(sentinel((int(t.sum()), cfg.encoder_dim), np.float32)),
                                          Out(sentinel((n_emb, cfg.llm_dim), np.float32)), n.ctypes.data], lambda: tuple(n))
    pcm, offs = clips2(9000, 5000)
    rows = [int(lib.mia_sensevoice_feature_rows(offs[i:].ctypes.data, 1)) for i in range(2)]
    n_emb = sum((r - 1) // cfg.adaptor_k + 1 for r in rows)
    same(ctx, lib.mia_sensevoice_encode_audio, [sv.h, In(pcm), offs.ctypes.data, 2, Out(sentinel((n_emb, cfg.llm_dim), np.float32)), n.ctypes.data],
         lambda: tuple(n))
    sv.close()


@pytest.fixture(scope="module")
def s3(ctx):
    from mlx_swift_audio_amd import s3tok as HS
    cfg = S.S3_CONFIGS["s3_micro"]
    tok = HS.S3Tokenizer.load(ctx, cfg, S.s3_weights(cfg, 2))
    yield cfg, tok
    tok.close()


def _s3_args(cfg, tok, mel_len):
    B, T = 2, 50
    mel = (0.5 * np.random.default_rng(6).standard_normal((B, cfg.n_mels, T))).astype(np.float32)
    ml, n = np.asarray(mel_len, np.int32), np.zeros(B, np.int32)
    stride = ((T - 1) // 2 + 1 - 1) // 2 + 1
    return [tok.h, In(mel), ml.ctypes.data, B, T, Out(sentinel((B, stride), np.int32)), stride, n.ctypes.data], n, ml


def test_s3tok(ctx, s3):
    cfg, tok = s3
    args, n, keep = _s3_args(cfg, tok, [50, 31])
    same(ctx, ctx.lib.mia_s3tok_encode, args, lambda: tuple(n))
    assert n[0] > n[1] > 0


def test_hift(ctx):
    from mlx_swift_audio_amd import hift as HH
    lib, rng = ctx.lib, np.random.default_rng(7)
    cfg = S.HIFT_CONFIGS["hift_micro"]
    gen = HH.HiFTGenerator.load(ctx, cfg, S.hift_weights(cfg))
    T, up, Hn = 5, gen.up, cfg.nb_harmonics + 1
    mel = (rng.standard_normal((80, T)) * 1.5 - 2).astype(np.float32)
    noise = rng.standard_normal((T * up, Hn)).astype(np.float32)
    f0, = same(ctx, lib.mia_hift_f0, [gen.h, In(mel), T, Out(sentinel(T, np.float32))])
    src, = same(ctx, lib.mia_hift_source, [gen.h, In(f0), T, In(noise), Out(sentinel(T * up, np.float32))])
    same(ctx, lib.mia_hift_decode, [gen.h, In(mel), T, In(src), Out(sentinel(T * up, np.float32))])
    cache = rng.standard_normal(37).astype(np.float32)
    same(ctx, lib.mia_hift_vocode, [gen.h, In(mel), T, In(noise), In(cache), cache.size, Out(sentinel(T * up, np.float32)), Out(sentinel(T * up, np.float32))])
    same(ctx, lib.mia_hift_vocode, [gen.h, In(mel), T, In(None), In(None), 0, Out(sentinel(T * up, np.float32)), Out(None)])
    Ts = np.asarray([5, 3], np.int32)
    mels = np.concatenate([mel.reshape(-1), mel[:, :3].reshape(-1)])
    nz = rng.standard_normal((int(Ts.sum()) * up, Hn)).astype(np.float32)
    same(ctx, lib.mia_hift_vocode_batch, [gen.h, In(mels), Ts.ctypes.data, 2, In(nz), Out(sentinel(int(Ts.sum()) * up, np.float32))])
    gen.close()


def test_flow(ctx):
    from mlx_swift_audio_amd import flow as HF
    lib, rng = ctx.lib, np.random.default_rng(8)
    cfg = S.FLOW_CONFIGS["flow_micro"]
    mod = HF.FlowModule.load(ctx, cfg, S.flow_weights(cfg))
    M, st = cfg.output_size, cfg.upsample_stride

    def utt(n, p, pf_len):
        tok, ptok = rng.integers(0, cfg.vocab_size, n).astype(np.int32), rng.integers(0, cfg.vocab_size, p).astype(np.int32)
        pf = rng.standard_normal((pf_len, M)).astype(np.float32)
        return tok, ptok, pf, rng.standard_normal(cfg.spk_embed_dim).astype(np.float32), rng.standard_normal((M, st * (n + p))).astype(np.float32)

    tok, ptok, pf, emb, z = utt(7, 3, 4)
    T = st * 10
    same(ctx, lib.mia_flow_encode, [mod.h, In(tok), tok.size, Out(sentinel((tok.size * st, M), np.float32))])
    same(ctx, lib.mia_flow_inference, [mod.h, In(tok), 7, In(ptok), 3, In(pf), 4, In(emb), In(z), 2, Out(sentinel((M, T - 4), np.float32))])
    trim = cfg.pre_lookahead_len * st
    nf = C.c_int(0)
    same(ctx, lib.mia_flow_inference_streaming, [mod.h, In(tok), 7, In(ptok), 3, In(pf), 4, In(emb), In(z[:, :T - trim].copy()), 2, 0, 2, 2,
                                                 Out(sentinel((M, T - trim - 4), np.float32)), C.byref(nf)], lambda: (nf.value,))
    assert nf.value == T - trim - 4
    us = [(tok, ptok, pf, emb, z), utt(4, 0, 0)]
    col = lambda i, cls=In: Ptrs([cls(u[i] if u[i].size else None) for u in us])
    cnt = lambda f: np.asarray([f(u) for u in us], np.int32)
    n_tok, n_pt, n_pf = cnt(lambda u: u[0].size), cnt(lambda u: u[1].size), cnt(lambda u: u[2].shape[0])
    mels = Ptrs([Out(sentinel((M, st * int(a + b) - int(c)), np.float32)) for a, b, c in zip(n_tok, n_pt, n_pf)])
    same(ctx, lib.mia_flow_inference_batch, [mod.h, 2, col(0), n_tok.ctypes.data, col(1), n_pt.ctypes.data, col(2), n_pf.ctypes.data, col(3), col(4), 2, mels])
    mod.close()


def test_campplus(ctx):
    from mlx_swift_audio_amd import speaker as SP
    lib = ctx.lib
    enc = SP.CAMPlusSpeakerEncoder.load(ctx, S.campplus_weights(7))
    x = S.synth_clip(3, 3300).astype(np.float32)
    F = int(lib.mia_kaldi_fbank_frames(x.size))
    fb, = same(ctx, lib.mia_campplus_fbank, [enc.h, In(x), x.size, 1, Out(sentinel((F, 80), np.float32))])
    same(ctx, lib.mia_campplus_forward, [enc.h, In(fb), F, Out(sentinel(192, np.float32))])
    same(ctx, lib.mia_campplus_embed, [enc.h, In(x), x.size, Out(sentinel(192, np.float32))])
    enc.close()


# ---- a failing host-memory call leaves nothing pending and nothing broken -----------------------------------------------------------

def test_failed_host_calls_return_drained():
    """Argument errors that are found only after copies have been queued.  Each returns MIA_ERR_INVALID_ARGUMENT; right after the return
    the stream has nothing pending; the correct call that follows gives the bits it gave before.  (stream.query() can be true on a build
    without the guarantee as well, when the copies happen to have finished: the assertion pins the guarantee, it does not tell builds
    apart.)  mia_op_lm_prompt_attention and mia_op_kvq_attention have no such error that their own argument checks let through, so the
    third such site is mia_op_linear, whose mia_gemm_check (lda a multiple of 8) runs after the operands are staged."""
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import codec as HC, s3tok as HS
    stream = torch.cuda.Stream()
    ctx = m.Context(0, stream=stream.cuda_stream)
    lib, rng = ctx.lib, np.random.default_rng(9)
    bad = m._lib.ERR_INVALID_ARGUMENT
    cfg = S.SNAC_CONFIGS["snac_micro_cn"]
    dec = HC.SNACDecoder.load(ctx, cfg, S.snac_weights(cfg, seed=3))
    state = rng.bit_generator.state
    good, ns, keep = _snac_args(cfg, dec, 7, rng)
    rng.bit_generator.state = state
    short, ns2, keep2 = _snac_args(cfg, dec, 7, rng, n_noise_delta=-1)
    want = run(ctx, lib.mia_snac_decode, good, 0)[1][0]
    rc, _ = run_and_query(ctx, stream, lib.mia_snac_decode, short)
    assert rc == bad and "noise must hold" in lib.mia_last_error(ctx.h).decode()
    assert run(ctx, lib.mia_snac_decode, good, 0)[1][0].tobytes() == want.tobytes()
    dec.close()

    scfg = S.S3_CONFIGS["s3_micro"]
    tok = HS.S3Tokenizer.load(ctx, scfg, S.s3_weights(scfg, 2))
    good, n, keep = _s3_args(scfg, tok, [50, 31])
    long1, n1, keep1 = _s3_args(scfg, tok, [50, 51])
    want = run(ctx, lib.mia_s3tok_encode, good, 0)[1][0]
    rc, _ = run_and_query(ctx, stream, lib.mia_s3tok_encode, long1)
    assert rc == bad and "mel_len[1] = 51" in lib.mia_last_error(ctx.h).decode()
    assert run(ctx, lib.mia_s3tok_encode, good, 0)[1][0].tobytes() == want.tobytes()
    tok.close()

    M, N, K = 8, 64, 64
    x, w = bf16(rng.standard_normal((M, K + 4))), bf16(rng.standard_normal((N, K)) / 8)
    lin = lambda lda: [ctx.h, In(x), lda, In(w), In(None), In(None), 0, Out(sentinel((M, N), np.uint16)), N, M, N, K, 0, m.BF16, 0, 1]
    x8 = np.ascontiguousarray(np.pad(x[:, :K], ((0, 0), (0, 8))))
    lin8 = [ctx.h, In(x8), K + 8, In(w), In(None), In(None), 0, Out(sentinel((M, N), np.uint16)), N, M, N, K, 0, m.BF16, 0, 1]
    want = run(ctx, lib.mia_op_linear, lin8, 0)[1][0]
    rc, _ = run_and_query(ctx, stream, lib.mia_op_linear, lin(K + 4))
    assert rc == bad and "lda must be a multiple of 8" in lib.mia_last_error(ctx.h).decode()
    assert run(ctx, lib.mia_op_linear, lin8, 0)[1][0].tobytes() == want.tobytes()
    ctx.close()


def run_and_query(ctx, stream, fn, args):
    """The failing host-memory call; the stream is asked at once, before anything else can wait for it."""
    done = []

    def call(*a):
        rc = fn(*a)
        done.append(stream.query())
        return rc
    rc, outs = run(ctx, call, args, 0, ok=False)
    assert done == [True], "a copy was still pending when the failing call returned"
    return rc, outs
