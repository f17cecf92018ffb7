"""Mimi decode on the GPU against the NumPy restatement of the reference (tests/_mimi_ref.py, float64): whole clips against
MimiRef.decode (full bidirectional attention), streams against MimiRef.decode_frames (the literal per-frame step loop).

Measure: max|got - ref64| <= tol * max|ref64| (the waveform is not tanh-bounded).  tol is NOT taken from the GPU: it is 8x the largest
gap between the oracle run in float32 and in float64 over the config's cases, measured on the CPU -- the reference's own arithmetic noise,
with a margin for the deeper reorderings of a tiled dot product (7168 long in mimi_202407's first convolution) against NumPy's pairwise sums.

  float32-vs-float64 gap of the oracle (weights seed 1, codes of _mimi_cases.codes):
    mimi_micro          whole T=9  n_q=1: 5.32e-07   n_q=4: 3.39e-07     whole T=40 n_q=1: 7.65e-07   n_q=4: 7.90e-07
                        stream 21 frames: 2.63e-07                                                   -> tol = 8 * 7.90e-07 = 6.32e-06
    mimi_micro_ctx250   stream 140 frames: 7.42e-07                                                  -> tol = 8 * 7.42e-07 = 5.94e-06
    mimi_202407         whole 6 frames: 1.57e-06     stream 6 frames: 1.32e-06                       -> tol = 8 * 1.57e-06 = 1.25e-05
  (The same cases differ between decode and decode_frames by 0.30, 0.36 and 0.87 of the peak: neither entry can pass as the other.)

Bit-identity between different splits of a stream is not asserted; DESIGN.md ("Mimi") says where it holds.
"""
import numpy as np
import pytest

import _mimi_cases as mc

pytestmark = pytest.mark.gpu

TOL = {"mimi_micro": 6.32e-06, "mimi_micro_ctx250": 5.94e-06, "mimi_202407": 1.25e-05}


@pytest.fixture(scope="module")
def codecs(ctx):
    from mlx_swift_audio_amd.mimi import MimiCodec
    made = {}

    def get(name):
        if name not in made:
            made[name] = MimiCodec.load(ctx, mc.config(name), mc.weights(name))
        return made[name]

    yield get
    for c in made.values():
        c.close()


def _check(name, got, ref, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    gap = mc.rel_gap(got, ref)
    print(f"{what}: rel gap {gap:.3e} (tol {TOL[name]:.3e}, peak {np.abs(ref).max():.3f})")
    assert np.isfinite(got).all() and gap <= TOL[name], (what, gap, TOL[name])


def _stream(codec, codes, split):
    s = codec.new_stream()
    try:
        out, at = [], 0
        for n in split:
            out.append(s.decode_frames(codes[:, at:at + n]).copy())
            at += n
        assert at == codes.shape[1]
        return np.concatenate(out)
    finally:
        s.close()


@pytest.mark.parametrize("name,frames,n_q", mc.WHOLE_CASES)
def test_whole_decode_matches_oracle(codecs, name, frames, n_q):
    codec = codecs(name)
    got = codec.decode(mc.codes(name, frames, n_q))
    assert got.size == codec.output_len(frames) == frames * mc.config(name).samples_per_frame
    _check(name, got, mc.whole_ref(name, frames, n_q), f"whole {name} T={frames} n_q={n_q}")


@pytest.mark.parametrize("split", [[21], [1] * 21, [3, 1, 5, 2, 10], [4, 0, 7, 0, 10]], ids=["one", "ones", "mixed", "zero"])
def test_stream_micro_splits(codecs, split):
    name, frames, n_q = mc.STREAM_CASES[0]
    codec, codes, ref = codecs(name), mc.codes(name, frames, n_q), mc.stream_ref(name, frames, n_q)
    got = _stream(codec, codes, split)
    _check(name, got, ref, f"stream {name} split {split}")
    single = _stream(codec, codes, [frames])
    gap = mc.rel_gap(got, single.astype(np.float64))
    print(f"split {split} against the single call: rel gap {gap:.3e}")
    assert gap <= 2 * TOL[name]          # both are within tol of the same oracle


@pytest.mark.parametrize("split", [[140], [64, 1, 75]], ids=["one", "split"])
def test_stream_real_window_width(codecs, split):
    name, frames, n_q = mc.STREAM_CASES[1]
    codec, codes = codecs(name), mc.codes(name, frames, n_q)
    got = _stream(codec, codes, split)
    _check(name, got, mc.stream_ref(name, frames, n_q), f"stream {name} split {split}")
    single = _stream(codec, codes, [frames])
    assert mc.rel_gap(got, single.astype(np.float64)) <= 2 * TOL[name]


def test_stream_full_geometry(codecs):
    name, frames, n_q = mc.STREAM_CASES[2]
    got = _stream(codecs(name), mc.codes(name, frames, n_q), [2, 1, 3])
    _check(name, got, mc.stream_ref(name, frames, n_q), f"stream {name} split [2, 1, 3]")


def test_stream_is_not_the_whole_decode(codecs):
    name, frames, n_q = mc.STREAM_CASES[0]
    codec, codes = codecs(name), mc.codes(name, frames, n_q)
    assert mc.rel_gap(_stream(codec, codes, [frames]), codec.decode(codes).astype(np.float64)) > 100 * TOL[name]


def test_reset_equals_fresh_stream(codecs):
    name, frames, n_q = mc.STREAM_CASES[0]
    codec, codes = codecs(name), mc.codes(name, frames, n_q)
    fresh = _stream(codec, codes, [5, 16])
    s = codec.new_stream()
    try:
        s.decode_frames(mc.codes(name, 13, n_q))             # other codes, enough frames to have compacted the history
        s.reset()
        again = np.concatenate([s.decode_frames(codes[:, :5]).copy(), s.decode_frames(codes[:, 5:]).copy()])
    finally:
        s.close()
    assert np.array_equal(fresh, again)


def test_two_streams_interleaved(codecs):
    name, frames, n_q = mc.STREAM_CASES[0]
    codec = codecs(name)
    ca, cb = mc.codes(name, frames, n_q), mc.codes(name, frames, 2)
    split = [3, 1, 5, 2, 10]
    solo_a, solo_b = _stream(codec, ca, split), _stream(codec, cb, split)
    a, b = codec.new_stream(), codec.new_stream()
    try:
        oa, ob, at = [], [], 0
        for n in split:
            oa.append(a.decode_frames(ca[:, at:at + n]).copy())
            ob.append(b.decode_frames(cb[:, at:at + n]).copy())
            at += n
    finally:
        a.close()
        b.close()
    assert np.array_equal(np.concatenate(oa), solo_a) and np.array_equal(np.concatenate(ob), solo_b)


def test_device_pcm_equals_host_pcm(codecs, ctx):
    """pcm_mem: the samples written straight into a device buffer are the ones a host call copies back, and none beyond them.  The
    buffer comes from the HIP runtime the library itself is linked against (reached through the library's handle)."""
    import ctypes as C
    from mlx_swift_audio_amd import _lib
    name, frames, n_q = mc.STREAM_CASES[0]
    codec, codes = codecs(name), mc.codes(name, frames, n_q)
    host = _stream(codec, codes, [frames])
    lib, guard = ctx.lib, 5
    nbytes = C.c_size_t((host.size + guard) * 4)
    d = C.c_void_p()
    assert lib.hipMalloc(C.byref(d), nbytes) == 0
    s = codec.new_stream()
    try:
        assert lib.hipMemset(d, 0, nbytes) == 0 and lib.hipDeviceSynchronize() == 0
        ns = C.c_int64(0)
        ctx.check(lib.mia_mimi_stream_decode(s.h, codes.ctypes.data, n_q, frames, d, host.size, C.byref(ns), _lib.MEM_DEVICE))
        ctx.synchronize()
        back = np.empty(host.size + guard, np.float32)
        assert lib.hipMemcpy(C.c_void_p(back.ctypes.data), d, nbytes, 2) == 0          # 2 = hipMemcpyDeviceToHost
        assert ns.value == host.size and np.array_equal(back[:host.size], host) and not back[host.size:].any()
    finally:
        s.close()
        lib.hipFree(d)


def test_error_paths_launch_nothing_and_leave_the_handle_usable(codecs, ctx):
    import ctypes as C
    from mlx_swift_audio_amd import MiaError, _lib
    name, frames, n_q = mc.STREAM_CASES[0]
    codec, codes, cfg = codecs(name), mc.codes(name, frames, n_q), mc.config(name)
    ref_whole, ref_stream = mc.whole_ref(name, 9, 4), mc.stream_ref(name, frames, n_q)
    s = codec.new_stream()
    try:
        first = s.decode_frames(codes[:, :8]).copy()

        def refused(fn):
            with pytest.raises(MiaError) as e:
                fn()
            assert e.value.code == _lib.ERR_INVALID_ARGUMENT, e.value

        bad_hi, bad_lo = codes[:, 8:12].copy(), codes[:, 8:12].copy()
        bad_hi[2, 1] = cfg.quantizer_bins
        bad_lo[0, 3] = -1
        for bad in (bad_hi, bad_lo, np.zeros((0, 4), np.int32), np.zeros((cfg.quantizer_nq + 1, 4), np.int32)):
            refused(lambda: codec.decode(bad))
            refused(lambda: s.decode_frames(bad))
        refused(lambda: s.decode_frames(codes[:2, 8:12]))                     # n_q changed mid-stream
        pcm, ns = np.empty(4 * cfg.samples_per_frame - 1, np.float32), C.c_int64(0)
        small = np.ascontiguousarray(codes[:, 8:12])
        for call, h in ((ctx.lib.mia_mimi_decode, codec.h), (ctx.lib.mia_mimi_stream_decode, s.h)):
            assert call(h, small.ctypes.data, n_q, 4, pcm.ctypes.data, pcm.size, C.byref(ns), _lib.MEM_HOST) == _lib.ERR_INVALID_ARGUMENT
            assert b"too small" in ctx.lib.mia_last_error(ctx.h)
        # nothing above touched the stream or the handle
        rest = s.decode_frames(codes[:, 8:]).copy()
        _check(name, np.concatenate([first, rest]), ref_stream, "stream after refused calls")
        _check(name, codec.decode(mc.codes(name, 9, 4)), ref_whole, "whole decode after refused calls")
    finally:
        s.close()


def test_loader_refuses_what_it_does_not_support(ctx):
    import dataclasses
    from mlx_swift_audio_amd import MiaError
    from mlx_swift_audio_amd.mimi import MimiCodec
    cfg, w = mc.config("mimi_micro"), mc.weights("mimi_micro")
    t, s = cfg.transformer, cfg.seanet
    for bad, text in ((dataclasses.replace(cfg, transformer=dataclasses.replace(t, num_heads=4)), "head_dim"),
                      (dataclasses.replace(cfg, transformer=dataclasses.replace(t, kv_repeat=2)), "kv_repeat"),
                      (dataclasses.replace(cfg, transformer=dataclasses.replace(t, gating=True)), "gated"),
                      (dataclasses.replace(cfg, transformer=dataclasses.replace(t, norm="rms_norm")), "layer_norm"),
                      (dataclasses.replace(cfg, seanet=dataclasses.replace(s, causal=False)), "causal"),
                      (dataclasses.replace(cfg, seanet=dataclasses.replace(s, nfilters=48)), "multiple of 32")):
        with pytest.raises(MiaError, match=text):
            MimiCodec.load(ctx, bad, w)
