"""GPU: stacked SNAC / DAC decode (mia_snac_decode_batch / mia_dac_decode_batch and their Python mirrors).  The contract is "utterance u
of a batch = its own single call, bit for bit" (np.array_equal): within a sequence every output element keeps the single call's
accumulation order, a tap never reads another sequence's rows, and rows past a sequence's end read as zero.  The shapes are the smallest
that can go wrong: a 1-frame utterance (2 latent rows) between long ones, so that every dilated tap (reach 27 rows) of its depthwise
convolutions would land in a neighbour; lengths that are no multiple of the 64- or 128-row GEMM tile; the shortest and the longest first."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from mlx_swift_audio_amd import synthetic as S
from oracle import codec as OC

pytestmark = pytest.mark.gpu
TOL = 2e-4                                                          # tests/test_codec_gpu.py's bound against the fp32 oracle


def _snac_codes(cfg, rng, n):
    return [rng.integers(0, cfg.codebook_size, n * (cfg.vq_strides[0] // s)).tolist() for s in cfg.vq_strides]


def _snac_case(dec, cfg, rng, frames, with_noise):
    codes = [_snac_codes(cfg, rng, n) for n in frames]
    noises = [rng.standard_normal(dec.noise_len(n * cfg.vq_strides[0])).astype(np.float32) for n in frames] if with_noise else None
    return codes, noises


def _assert_batch_equals_single(dec, cfg, codes, noises):
    got = dec.decode_batch(codes, noises)
    assert len(got) == len(codes)
    hop = int(np.prod(cfg.decoder_rates))
    for u, c in enumerate(codes):
        one = dec.decode(c, None if noises is None else noises[u])
        T0 = max(len(lv) * s for lv, s in zip(c, cfg.vq_strides))
        assert got[u].shape == one.shape == (T0 * hop,), (u, got[u].shape, one.shape)
        assert np.array_equal(got[u], one), (u, float(np.abs(got[u] - one).max()))
    return got


@pytest.fixture(scope="module")
def snac_micro(ctx):
    from mlx_swift_audio_amd import codec as HC
    decs = {}
    for name in ("snac_micro", "snac_micro_cn"):
        cfg = S.SNAC_CONFIGS[name]
        decs[name] = (cfg, HC.SNACDecoder.load(ctx, cfg, S.snac_weights(cfg, seed=3)))
    yield decs
    for _, d in decs.values():
        d.close()


@pytest.mark.parametrize("name", ["snac_micro", "snac_micro_cn"])
@pytest.mark.parametrize("with_noise", [False, True])
@pytest.mark.parametrize("frames", [[37, 5, 37, 1, 64], [1, 90], [33]])
def test_snac_batch_equals_single_calls(snac_micro, name, with_noise, frames):
    cfg, dec = snac_micro[name]
    rng = np.random.default_rng(sum(frames))
    codes, noises = _snac_case(dec, cfg, rng, frames, with_noise)
    _assert_batch_equals_single(dec, cfg, codes, noises)


@pytest.mark.parametrize("name", ["snac_micro", "snac_micro_cn"])
def test_snac_batch_with_per_utterance_tail(snac_micro, name):
    """Stages whose activations exceed the stack budget run per utterance on the stacked buffers (set_stack_budget; 0 = everything
    after stage 0): the hand-over from the stacked stages to the single-call launches keeps every bit."""
    cfg, dec = snac_micro[name]
    rng = np.random.default_rng(144)
    codes, noises = _snac_case(dec, cfg, rng, [37, 5, 37, 1, 64], True)
    try:
        dec.set_stack_budget(0)
        _assert_batch_equals_single(dec, cfg, codes, noises)
        _assert_batch_equals_single(dec, cfg, codes, None)
    finally:
        dec.set_stack_budget(-1)


@pytest.mark.parametrize("name", ["snac_micro", "snac_micro_cn"])
def test_snac_batch_after_longer_batch_reads_padding_as_zero(ctx, name):
    """Scratch is grow-only and never cleared: a batch of short utterances after a batch of long ones finds the long ones' activations in
    its padding rows.  They must read as zero."""
    from mlx_swift_audio_amd import codec as HC
    cfg = S.SNAC_CONFIGS[name]
    dec = HC.SNACDecoder.load(ctx, cfg, S.snac_weights(cfg, seed=3))
    rng = np.random.default_rng(21)
    codes, noises = _snac_case(dec, cfg, rng, [70, 64, 70], True)
    _assert_batch_equals_single(dec, cfg, codes, noises)
    codes, noises = _snac_case(dec, cfg, rng, [3, 9, 1], True)       # same handle, same count, every utterance shorter
    got = dec.decode_batch(codes, noises)                            # (before any single call touches the scratch again)
    for u, c in enumerate(codes):
        assert np.array_equal(got[u], dec.decode(c, noises[u])), u
    dec.close()


def test_snac_batch_skips_wrong_length_level_for_that_utterance_only(snac_micro):
    cfg, dec = snac_micro["snac_micro"]
    rng = np.random.default_rng(4)
    odd = [[1, 2], [4, 5, 6, 7, 8, 9]]                               # level 0 expands to 4 rows, level 1 to 6: level 0 is skipped
    codes = [_snac_codes(cfg, rng, 6), odd, _snac_codes(cfg, rng, 3)]
    got = dec.decode_batch(codes)
    for u, c in enumerate(codes):
        assert np.array_equal(got[u], dec.decode(c)), u
    assert got[1].shape == (6 * int(np.prod(cfg.decoder_rates)),)


def test_batches_match_oracle(ctx, snac_micro):
    from mlx_swift_audio_amd import codec as HC
    cfg, dec = snac_micro["snac_micro"]
    ora = OC.SNACOracle(cfg, S.snac_weights(cfg, seed=3))
    rng = np.random.default_rng(12)
    codes, noises = _snac_case(dec, cfg, rng, [37, 1, 20], True)
    for u, got in enumerate(dec.decode_batch(codes, noises)):
        ref = ora.decode(codes[u], noises[u])
        assert got.shape == ref.shape
        assert np.abs(got - ref).max() <= TOL, (u, np.abs(got - ref).max())
    dcfg = S.DAC_CONFIGS["dac_micro"]
    w = S.dac_weights(dcfg, seed=4)
    dac = HC.DACCodec.load(ctx, dcfg, w)
    dora = OC.DACOracle(dcfg, w)
    dcodes = [rng.integers(0, dcfg.codebook_size, (dcfg.n_codebooks, T)) for T in (45, 2, 70)]
    for u, got in enumerate(dac.decode_batch(dcodes)):
        ref = dora.decode_from_codes(dcodes[u])
        assert got.shape == ref.shape
        assert np.abs(got - ref).max() <= TOL, (u, np.abs(got - ref).max())
    dac.close()


def _unsaturate(w, final_g_key, oracle_decode):
    """As in tests/test_codec_gpu.py: rescale the last conv's weight-norm gain so that the oracle's pre-tanh peak is 0.5 (a random-init
    stack this deep otherwise saturates the output tanh, which would hide every error but the zero crossings')."""
    g0 = w[final_g_key].copy()
    w[final_g_key[:-len("weight_g")] + "bias"][:] = 0.0
    w[final_g_key] = g0 * np.float32(1e-7)
    peak = np.abs(oracle_decode(w)).max() / 1e-7
    w[final_g_key] = g0 * np.float32(0.5 / max(peak, 1e-30))
    return w


def test_snac_24khz_real_geometry_batch(ctx):
    from mlx_swift_audio_amd import codec as HC
    cfg = S.SNAC_CONFIGS["snac_24khz"]
    rng = np.random.default_rng(8)
    frames = [12, 3, 7]
    codes = [_snac_codes(cfg, rng, n) for n in frames]
    w = S.snac_weights(cfg, seed=6)
    n0 = rng.standard_normal(OC.SNACOracle(cfg, w).noise_len(frames[0] * cfg.vq_strides[0])).astype(np.float32)
    w = _unsaturate(w, f"decoder.model.layers.{3 + len(cfg.decoder_rates)}.weight_g", lambda ww: OC.SNACOracle(cfg, ww).decode(codes[0], n0))
    dec = HC.SNACDecoder.load(ctx, cfg, w)
    noises = [n0] + [rng.standard_normal(dec.noise_len(n * cfg.vq_strides[0])).astype(np.float32) for n in frames[1:]]
    got = _assert_batch_equals_single(dec, cfg, codes, noises)
    assert 0.05 < np.abs(got[0]).max() < 0.9 and got[0].std() > 0.01     # inside tanh's open range: the equality is not one of +-1 against +-1
    # three utterances x three buffers hold 7, 28, 57 and 57 MB at the four upsampled stages: 16 MiB hands over to the per-utterance
    # launches after the first of them, 0 right after stage 0 (the default budget above keeps every stage stacked)
    for budget in (16 << 20, 0, 1 << 40):
        dec.set_stack_budget(budget)
        for a, b in zip(dec.decode_batch(codes, noises), got):
            assert np.array_equal(a, b), budget
    dec.close()


def test_dac_speech_real_geometry_batch(ctx):
    from mlx_swift_audio_amd import codec as HC
    cfg = S.DAC_CONFIGS["dac_speech"]
    rng = np.random.default_rng(2)
    codes = [rng.integers(0, cfg.codebook_size, (cfg.n_codebooks, T)) for T in (60, 2, 25)]
    w = S.dac_weights(cfg, seed=7)
    w = _unsaturate(w, f"decoder.model.layers.{2 + len(cfg.decoder_rates)}.weight_g", lambda ww: OC.DACOracle(cfg, ww).decode_from_codes(codes[0]))
    dec = HC.DACCodec.load(ctx, cfg, w)
    got = dec.decode_batch(codes)
    for u, c in enumerate(codes):
        one = dec.decode_from_codes(c)
        assert got[u].shape == one.shape == (dec.output_len(c.shape[1]),)
        assert np.array_equal(got[u], one), (u, float(np.abs(got[u] - one).max()))
    assert 0.05 < np.abs(got[0]).max() < 0.9 and got[0].std() > 0.01
    dec.set_stack_budget(0)                                          # per-utterance launches from the first transposed convolution on
    for a, b in zip(dec.decode_batch(codes), got):
        assert np.array_equal(a, b)
    dec.close()


def _dac_single(dec, codes):
    """One sequence through mia_dac_decode itself (decode_from_codes sends B > 1 through the batch entry)."""
    c = np.ascontiguousarray(codes, np.int32)
    out = np.empty(dec.output_len(c.shape[1]), np.float32)
    ns = C.c_int64(0)
    dec.ctx.check(dec.ctx.lib.mia_dac_decode(dec.h, c.ctypes.data, c.shape[0], c.shape[1], out.ctypes.data, out.size, C.byref(ns), 0))
    return out[:ns.value]


def test_dac_micro_batch_equals_single_calls(ctx):
    from mlx_swift_audio_amd import codec as HC
    cfg = S.DAC_CONFIGS["dac_micro"]
    dec = HC.DACCodec.load(ctx, cfg, S.dac_weights(cfg, seed=4))
    rng = np.random.default_rng(1)
    ragged = [rng.integers(0, cfg.codebook_size, (cfg.n_codebooks, T)) for T in (45, 2, 130)]
    got = dec.decode_batch(ragged)
    for u, c in enumerate(ragged):
        one = _dac_single(dec, c)
        assert got[u].shape == one.shape == (dec.output_len(c.shape[1]),)
        assert np.array_equal(got[u], one), u
    cube = rng.integers(0, cfg.codebook_size, (3, cfg.n_codebooks, 45))
    out = dec.decode_from_codes(cube)
    assert out.shape == (3, dec.output_len(45))
    for b in range(3):
        assert np.array_equal(out[b], _dac_single(dec, cube[b])), b
    assert np.array_equal(dec.decode_from_codes(cube[1]), out[1])
    dec.close()


def _flat_snac_args(cfg, dec, codes, noises):
    n = np.asarray([[len(lv) for lv in c] for c in codes], np.int32)
    flat = np.concatenate([np.asarray(lv, np.int32) for c in codes for lv in c])
    nz = np.concatenate(noises).astype(np.float32)
    outs = [dec.output_len(max(len(lv) * s for lv, s in zip(c, cfg.vq_strides))) for c in codes]
    off = np.zeros(len(codes) + 1, np.int64)
    off[1:] = np.cumsum(outs)
    return n, flat, nz, off


def test_snac_batch_device_memory_equals_host_memory(ctx, snac_micro):
    import torch
    cfg, dec = snac_micro["snac_micro_cn"]
    rng = np.random.default_rng(31)
    codes, noises = _snac_case(dec, cfg, rng, [20, 1, 37], True)
    host = dec.decode_batch(codes, noises)
    n, flat, nz, off = _flat_snac_args(cfg, dec, codes, noises)
    d_codes, d_noise = torch.from_numpy(flat).cuda(), torch.from_numpy(nz).cuda()
    d_pcm = torch.zeros(int(off[-1]), dtype=torch.float32, device="cuda")
    ns = np.zeros(len(codes), np.int64)
    torch.cuda.synchronize()
    ctx.check(ctx.lib.mia_snac_decode_batch(dec.h, len(codes), d_codes.data_ptr(), n.ctypes.data, n.shape[1], d_noise.data_ptr(), nz.size,
                                            d_pcm.data_ptr(), off.ctypes.data, ns.ctypes.data, 1))
    torch.cuda.synchronize()
    pcm = d_pcm.cpu().numpy()
    for u in range(len(codes)):
        assert ns[u] == host[u].size
        assert np.array_equal(pcm[off[u]:off[u] + ns[u]], host[u]), u


def test_batch_error_paths_leave_the_handle_usable(ctx, snac_micro):
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import codec as HC
    cfg, dec = snac_micro["snac_micro"]
    rng = np.random.default_rng(17)
    codes, noises = _snac_case(dec, cfg, rng, [5, 2], True)
    want = [dec.decode(c, z) for c, z in zip(codes, noises)]
    n, flat, nz, off = _flat_snac_args(cfg, dec, codes, noises)
    pcm = np.empty(int(off[-1]), np.float32)
    ns = np.zeros(2, np.int64)
    lib = ctx.lib
    dcfg = S.DAC_CONFIGS["dac_micro"]
    dac = HC.DACCodec.load(ctx, dcfg, S.dac_weights(dcfg, seed=4))
    dcodes = rng.integers(0, dcfg.codebook_size, (2, dcfg.n_codebooks, 6)).astype(np.int32)
    dT = np.asarray([6, 6], np.int64)
    doff = np.arange(3, dtype=np.int64) * dac.output_len(6)
    dpcm = np.empty(int(doff[-1]), np.float32)

    def snac(h=None, U=2, flat=flat, n=n, nz=nz, off=off):
        return lib.mia_snac_decode_batch(dec.h if h is None else h, U, flat.ctypes.data, n.ctypes.data, n.shape[1], nz.ctypes.data, nz.size,
                                         pcm.ctypes.data, off.ctypes.data, ns.ctypes.data, 0)

    def dacb(h=None, U=2, codes=dcodes, T=dT, off=doff):
        return lib.mia_dac_decode_batch(dac.h if h is None else h, U, codes.ctypes.data, dcfg.n_codebooks, T.ctypes.data, dpcm.ctypes.data,
                                        off.ctypes.data, ns.ctypes.data, 0)

    bad_code = flat.copy(); bad_code[0] = cfg.codebook_size + 3
    empty = n.copy(); empty[1, :] = 0
    tight = off.copy(); tight[1] -= 1                                # utterance 0 gets one sample too few
    dbad = dcodes.copy(); dbad[1, 0, 0] = -1
    dtight = doff.copy(); dtight[2] -= 1
    calls = [lambda: snac(h=dac.h), lambda: dacb(h=dec.h),          # wrong handle kind
             lambda: snac(U=0), lambda: snac(U=65), lambda: dacb(U=0), lambda: dacb(U=65),
             lambda: snac(n=empty), lambda: dacb(T=np.asarray([6, 0], np.int64)),     # an utterance with no codes
             lambda: snac(flat=bad_code), lambda: dacb(codes=dbad),                   # code out of range
             lambda: snac(nz=nz[:-1].copy()),                                         # noise total != sum of the utterances' lengths
             lambda: snac(off=tight), lambda: dacb(off=dtight)]                       # pcm gap too small
    for i, call in enumerate(calls):
        with pytest.raises(m.MiaError) as e:
            ctx.check(call())
        assert e.value.code == m._lib.ERR_INVALID_ARGUMENT, (i, e.value)
    got = dec.decode_batch(codes, noises)                            # both handles still give the right bits
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    ctx.check(dacb())
    for b in range(2):
        assert np.array_equal(dpcm[doff[b]:doff[b + 1]], _dac_single(dac, dcodes[b])), b
    dac.close()


def test_orpheus_generate_chunks_decodes_in_one_batch(ctx, snac_micro):
    """generate_chunks = generate_chunk per sentence, the sentence without codes included.  parse_output reads the ids after the last
    audio-start marker of prompt + generation, so prompts that carry whole 7-id frames decode to audio whatever the random-init LM
    emits; max_new_tokens = 5 is less than one frame, so the marker-only prompt parses to no codes."""
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import lm as HL
    cfg = dataclasses.replace(S.LM_CONFIGS["llama-micro"], vocab=HL.CODE_OFFSET + 7 * 4096 + 2)
    model = HL.CausalLM.load(ctx, cfg, S.lm_weights(cfg, seed=9, round_to="bf16"), m.BF16)
    scfg, snac = snac_micro["snac_micro"]
    tts = HL.OrpheusTTS(model, snac)
    rng = np.random.default_rng(6)

    def prompt(n_text, n_frames):
        ids = rng.integers(0, 3000, n_text).tolist() + [HL.AUDIO_CODE_DATA_START_MARKER]
        for _ in range(n_frames):
            ids += [HL.CODE_OFFSET + k * 4096 + int(rng.integers(0, scfg.codebook_size)) for k in range(7)]
        return ids

    sents = [prompt(6, 3), prompt(9, 0), prompt(4, 1), prompt(3, 11)]
    u = rng.random((len(sents), 5)).astype(np.float32)
    seq = [tts.generate_chunk(s, u[b], max_new_tokens=5) for b, s in enumerate(sents)]
    model.set_batch(len(sents))
    par = tts.generate_chunks(sents, u, max_new_tokens=5)
    assert [g for g, _ in par] == [g for g, _ in seq]
    assert [a.size > 0 for _, a in seq] == [True, False, True, True]
    for b, ((_, a), (_, c)) in enumerate(zip(par, seq)):
        assert a.dtype == c.dtype and a.shape == c.shape and np.array_equal(a, c), b
    model.close()
