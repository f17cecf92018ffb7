"""Mimi encode on the GPU against the NumPy restatement of the reference (tests/_mimi_encode_ref.py, float64).

Latent (mia_mimi_encode_latent): max|got - ref64| <= tol * max|ref64|.  tol is NOT taken from the GPU: it is 8x the largest gap between
the oracle run in float32 and in float64 over the config's cases, measured on the CPU (test_mimi_encode_ref.py prints the table):

  float32-vs-float64 gap of the oracle's latent (weights seed 1, clips of _mimi_encode_cases.pcm):
    mimi_micro    n = 1: 3.07e-07   11: 3.72e-07   12: 3.83e-07   13: 3.96e-07   108: 8.04e-07   485: 7.40e-07   -> tol = 8 * 8.04e-07 = 6.43e-06
    mimi_202407   n = 5760 (P = 6): 1.17e-06      n = 6537 (P = 7, ODD: the edge copy behind): 1.32e-06        -> tol = 8 * 1.32e-06 = 1.06e-05

Codes (mia_mimi_quantize, mia_mimi_encode): exact equality with the oracle's codes.  That claim is safe only where the oracle's own
decision is not within arithmetic noise, so each test first asserts ON THE ORACLE that every (stage, frame) gap between the best and the
second-best distance exceeds GAP_TOL = 8 x max|d32 - d64| over its cases, d32 being the float32 chain teacher-forced on the float64
picks.  Measured on the CPU (seeds 0 / 1 / 2 of the latent draw; the chosen one is in _mimi_encode_cases.QUANT_CASES):
    mimi_micro T = 37          noise 3.9e-06 .. 4.2e-06   smallest gap 1.8e-03 / 2.7e-02 / 5.1e-03
    mimi_micro bins = 100      noise 6.3e-06 .. 7.8e-06   smallest gap 2.3e-03 / 1.8e-03 / 8.1e-03
    mimi_202407 T = 1 / 5 / 33 noise 2.5e-05 .. 5.5e-05   smallest gap 2.1e-02 / 3.0e-02 / 1.1e-02, 3.1e-04 / 2.9e-03 / 1.5e-03, 3.9e-04 / 3.0e-04 / 2.6e-03
    -> GAP_TOL = 8 * 5.5e-05 = 4.4e-04 for the quantiser cases; the end-to-end cases: noise 7.6e-06 and 9.4e-05, gaps 1.8e-03 and 6.4e-03
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import _mimi_cases as mc
import _mimi_encode_cases as ec

pytestmark = pytest.mark.gpu

TOL = {"mimi_micro": 6.43e-06, "mimi_202407": 1.06e-05}


@pytest.fixture(scope="module")
def codecs(ctx):
    from mlx_swift_audio_amd.mimi import MimiCodec
    made = {}

    def get(name):
        if name not in made:
            made[name] = MimiCodec.load(ctx, ec.config(name), ec.weights(name))
        return made[name]

    yield get
    for c in made.values():
        c.close()


def _gap_tol(triples):
    return 8.0 * max(noise for _, _, noise in triples)


@pytest.mark.parametrize("name,n", ec.LATENT_CASES)
def test_latent_matches_oracle(codecs, name, n):
    codec, ref = codecs(name), ec.latent_ref(name, n)
    assert codec.has_encoder and codec.encode_frames(n) == ref.shape[0]
    got = codec.encode_latent(ec.pcm(name, n))
    assert got.shape == ref.shape
    gap = ec.rel_gap(got, ref)
    print(f"latent {name} n={n} T={ref.shape[0]}: rel gap {gap:.3e} (tol {TOL[name]:.3e}, peak {np.abs(ref).max():.3f})")
    assert np.isfinite(got).all() and gap <= TOL[name], (name, n, gap)


@pytest.mark.parametrize("name,frames,seed", ec.QUANT_CASES)
def test_quantize_matches_oracle(codecs, name, frames, seed):
    gap_tol = _gap_tol([ec.quant_ref(*c) for c in ec.QUANT_CASES])
    codes, gap, noise = ec.quant_ref(name, frames, seed)
    print(f"quantize {name} T={frames}: oracle noise {noise:.2e}, smallest gap {gap.min():.2e}, GAP_TOL {gap_tol:.2e}")
    assert gap.min() > gap_tol, "the oracle's own decision is within noise: pick another seed"
    got = codecs(name).quantize(ec.latent_draw(name, frames, seed))
    assert got.dtype == np.int32 and got.shape == codes.shape
    assert np.array_equal(got, codes), np.argwhere(got != codes)[:8]


def test_tie_goes_to_the_lowest_index(ctx):
    """The winning entry duplicated at j and j + bins / 2 (identical embedding_sum and cluster_usage rows: bitwise equal distances, in
    different entry slices): the lower of the two must come out, in rvq_first's stage and in a later stage of rvq_rest."""
    from mlx_swift_audio_amd.mimi import MimiCodec
    from _mimi_encode_ref import MimiEncodeRef
    name, T = "mimi_micro_bins512", 3
    cfg, w = ec.config(name), dict(ec.weights(name))
    z = ec.latent_draw(name, T, 0)
    half = cfg.quantizer_bins // 2
    for stage in (0, 2):                     # stage 2's winner does not depend on the copy made in stage 0's book (separate chains)
        p = "quantizer.rvq_first.vq.layers.0.codebook." if stage == 0 else f"quantizer.rvq_rest.vq.layers.{stage - 1}.codebook."
        win = int(MimiEncodeRef(cfg, w).quantize(z)[0][stage, 0])
        twin = (win + half) % cfg.quantizer_bins
        for t in ("embedding_sum", "cluster_usage"):
            a = w[p + t].copy()
            a[twin] = a[win]
            w[p + t] = a
    codes, gap, _ = MimiEncodeRef(cfg, w).quantize(z)
    assert gap[0, 0] == 0.0 and gap[2, 0] == 0.0                      # exact ties in the oracle, resolved to the lower index
    codec = MimiCodec.load(ctx, cfg, w)
    try:
        got = codec.quantize(z)
    finally:
        codec.close()
    for stage in (0, 2):
        assert got[stage, 0] == codes[stage, 0] and got[stage, 0] < half, (stage, got[stage, 0], codes[stage, 0])
    assert np.array_equal(got[:, 0], codes[:, 0])                     # and the chain behind the tie went on from the same entry


@pytest.mark.parametrize("name,n", ec.ENCODE_CASES)
def test_encode_end_to_end(codecs, ctx, name, n):
    from mlx_swift_audio_amd import _lib
    codec, pcm, nq = codecs(name), ec.pcm(name, n), ec.config(name).quantizer_nq
    full = codec.encode(pcm)
    assert full.shape == (nq, codec.encode_frames(n)) and full.min() >= 0 and full.max() < ec.config(name).quantizer_bins
    assert np.array_equal(full, codec.quantize(codec.encode_latent(pcm)))                      # bit for bit
    codes, gap, _ = ec.encode_ref(name, n)
    gap_tol = _gap_tol([ec.encode_ref(*c) for c in ec.ENCODE_CASES])
    print(f"encode {name} n={n}: smallest oracle gap {gap.min():.2e}, GAP_TOL {gap_tol:.2e}")
    assert gap.min() > gap_tol
    assert np.array_equal(full, codes), np.argwhere(full != codes)[:8]
    for k in (1, 2, nq):
        assert np.array_equal(codec.encode(pcm, n_q=k), full[:k])
    # device pcm == host pcm
    lib, d = ctx.lib, C.c_void_p()
    assert lib.hipMalloc(C.byref(d), C.c_size_t(n * 4)) == 0
    try:
        assert lib.hipMemcpy(d, C.c_void_p(pcm.ctypes.data), C.c_size_t(n * 4), 1) == 0          # 1 = hipMemcpyHostToDevice
        out, nf = np.zeros_like(full), C.c_int64(0)
        ctx.check(lib.mia_mimi_encode(codec.h, d, n, nq, out.ctypes.data, out.shape[1], C.byref(nf), _lib.MEM_DEVICE))
        assert nf.value == full.shape[1] and np.array_equal(out, full)
    finally:
        lib.hipFree(d)


def test_refused_calls_launch_nothing_and_leave_decode_and_a_stream_usable(codecs, ctx):
    from mlx_swift_audio_amd import MiaError, _lib
    name, frames, n_q = mc.STREAM_CASES[0]
    codec, codes, cfg = codecs(name), mc.codes(name, frames, n_q), ec.config(name)
    lib, pcm = ctx.lib, ec.pcm(name, 12 * 9)
    whole_before = codec.decode(codes).copy()
    fresh = codec.new_stream()
    try:
        stream_before = np.concatenate([fresh.decode_frames(codes[:, :8]).copy(), fresh.decode_frames(codes[:, 8:]).copy()])
    finally:
        fresh.close()
    s = codec.new_stream()
    try:
        first = s.decode_frames(codes[:, :8]).copy()

        def refused(fn):
            with pytest.raises(MiaError) as e:
                fn()
            assert e.value.code == _lib.ERR_INVALID_ARGUMENT, e.value

        for bad_q in (0, cfg.quantizer_nq + 1):
            refused(lambda: codec.encode(pcm, n_q=bad_q))
            refused(lambda: codec.quantize(np.zeros((3, cfg.transformer.d_model), np.float32), n_q=bad_q))
        refused(lambda: codec.encode(np.zeros(0, np.float32)))
        refused(lambda: codec.encode_latent(np.zeros(0, np.float32)))
        refused(lambda: codec.quantize(np.zeros((0, cfg.transformer.d_model), np.float32)))
        T = codec.encode_frames(pcm.size)
        out, lat, nf = np.zeros((n_q, T), np.int32), np.zeros((T, cfg.transformer.d_model), np.float32), C.c_int64(0)
        small = (lambda: lib.mia_mimi_encode(codec.h, pcm.ctypes.data, pcm.size, n_q, out.ctypes.data, T - 1, C.byref(nf), _lib.MEM_HOST),
                 lambda: lib.mia_mimi_encode_latent(codec.h, pcm.ctypes.data, pcm.size, lat.ctypes.data, T - 1, C.byref(nf), _lib.MEM_HOST))
        for call in small:
            assert call() == _lib.ERR_INVALID_ARGUMENT and b"too small" in lib.mia_last_error(ctx.h)
        assert lib.mia_mimi_encode(codec.h, None, pcm.size, n_q, out.ctypes.data, T, C.byref(nf), _lib.MEM_HOST) == _lib.ERR_INVALID_ARGUMENT
        assert lib.mia_mimi_encode(codec.h, pcm.ctypes.data, pcm.size, n_q, None, T, C.byref(nf), _lib.MEM_HOST) == _lib.ERR_INVALID_ARGUMENT
        assert lib.mia_mimi_encode(codec.h, pcm.ctypes.data, pcm.size, n_q, out.ctypes.data, T, C.byref(nf), 7) == _lib.ERR_INVALID_ARGUMENT
        # one sample past the clip limit (2^27 / nfilters): refused on the count alone, before the samples are looked at
        limit = (1 << 27) // cfg.seanet.nfilters
        assert lib.mia_mimi_encode(codec.h, pcm.ctypes.data, limit + 1, n_q, out.ctypes.data, 1 << 40, C.byref(nf), _lib.MEM_HOST) == _lib.ERR_INVALID_ARGUMENT
        assert b"limit" in lib.mia_last_error(ctx.h)
        # nothing above touched the stream or the handle
        rest = s.decode_frames(codes[:, 8:]).copy()
        assert np.array_equal(np.concatenate([first, rest]), stream_before)
        assert np.array_equal(codec.decode(codes), whole_before)
    finally:
        s.close()


def test_decode_only_handle_refuses_encode_and_half_an_encoder_fails_the_load(ctx):
    from mlx_swift_audio_amd import MiaError, _lib
    from mlx_swift_audio_amd.mimi import MimiCodec
    name = "mimi_micro"
    cfg, w = ec.config(name), ec.weights(name)
    plain = MimiCodec.load(ctx, cfg, mc.weights(name))
    try:
        assert not plain.has_encoder and plain.encode_frames(100) == 0
        for fn in (lambda: plain.encode(ec.pcm(name, 12)), lambda: plain.encode_latent(ec.pcm(name, 12)),
                   lambda: plain.quantize(np.zeros((2, cfg.transformer.d_model), np.float32))):
            with pytest.raises(MiaError, match="no encoder loaded") as e:
                fn()
            assert e.value.code == _lib.ERR_INVALID_ARGUMENT
        # the decode side of a handle with an encoder is the decode-only handle's
        both = MimiCodec.load(ctx, cfg, w)
        try:
            codes = mc.codes(name, 9, 4)
            assert np.array_equal(both.decode(codes), plain.decode(codes))
        finally:
            both.close()
    finally:
        plain.close()
    for missing in ("downsample.conv.conv.weight", "encoder.layers.1.downsample.conv.conv.bias", "quantizer.rvq_rest.input_proj.weight",
                    "encoder_transformer.transformer.layers.1.gating.linear2.weight", "encoder.init_conv1d.conv.conv.weight"):
        with pytest.raises(MiaError, match=missing.replace(".", r"\.")):
            MimiCodec.load(ctx, cfg, {k: v for k, v in w.items() if k != missing})
    with pytest.raises(MiaError, match="multiple of 8"):
        bad = dataclasses.replace(cfg, quantizer_dim=36)
        from mlx_swift_audio_amd import synthetic
        MimiCodec.load(ctx, bad, synthetic.mimi_weights(bad, 1, encoder=True))
