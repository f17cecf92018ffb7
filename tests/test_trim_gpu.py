"""AudioTrimmer's frame search on the GPU (csrc/audio_trim.hip behind trim.Clip) against the literal restatement of the Swift in
tests/_trim_ref.py.

Bounds must EQUAL the restatement's on every case of tests/_trim_cases.py; tests/test_trim_host.py certifies on the CPU that every
frame of every case is at least 0.01 dB from the threshold, over 50 times the reference's own fp32 noise, so the demand is fair.
Frame energies: relative error against the correctly rounded float64 mean square (math.fsum of the exact squares) at most
4 * frame * 2^-53 -- the squares are exact in double, a frame takes fewer than `frame` additions of non-negative terms, each off by at
most 2^-53 relative, and the one division fits in the headroom."""
import ctypes as C

import numpy as np
import pytest

import _trim_cases as TC
import _trim_ref as R
from mlx_swift_audio_amd import _lib
from mlx_swift_audio_amd import trim as T

pytestmark = pytest.mark.gpu

BAD, UNSUPPORTED, INVALID_AUDIO = _lib.ERR_INVALID_ARGUMENT, _lib.ERR_UNSUPPORTED, _lib.ERR_INVALID_AUDIO


@pytest.fixture(scope="module")
def ref():
    """The restatement's bounds of every case, computed once."""
    return {name: R.bounds_literal(x, frame, hop, top_db) for name, x, frame, hop, top_db, _ in TC.cases()}


@pytest.fixture(scope="module")
def clips(ctx):
    made = {}

    def get(name):
        if name not in made:
            made[name] = T.Clip(ctx, TC.case(name)[1], TC.SR)
        return made[name]
    yield get
    for c in made.values():
        c.close()


# ---- bounds ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in TC.cases()])
def test_bounds_equal_the_restatement(clips, ref, name):
    _, x, frame, hop, top_db, want = TC.case(name)
    start, end, found = clips(name).bounds(frame, hop, top_db)
    print(f"{name}: gpu {(start, end, found)} restatement {ref[name]}")
    assert ref[name] is not None and found
    assert (start, end) == ref[name]
    if want is not None:
        assert (start, end) == want
    assert int(clips(name).ctx.lib.mia_clip_num_frames(x.size, frame, hop)) == R.num_frames(x.size, frame, hop)


def test_decaying_noise_ends_differ(clips):
    c = clips("decaying_20")
    assert c.bounds(600, 300, 20.0)[1] < c.bounds(600, 300, 60.0)[1]


# ---- frame energies -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,frame,hop", [("noise_floor", 600, 300), ("sizes_22050", 551, 275), ("hop_gt_frame", 200, 330), ("short", 600, 300),
                                            ("decaying_20", 600, 300)])
def test_frame_energy_parity(clips, name, frame, hop):
    x = TC.case(name)[1]
    got = clips(name).frame_energy(frame, hop)
    want = R.mean_squares_exact(x, frame, hop)
    assert got.shape == want.shape == (R.num_frames(x.size, frame, hop),)
    nz = want != 0
    assert np.all(got[~nz] == 0)
    err = float((np.abs(got - want)[nz] / want[nz]).max()) if nz.any() else 0.0
    print(f"{name}: {got.size} frames, largest relative error {err:.3e}, bound {4 * frame * 2.0 ** -53:.3e}")
    assert err <= 4 * frame * 2.0 ** -53
    again = clips(name).frame_energy(frame, hop)
    assert again.tobytes() == got.tobytes()                                     # repeatable to the bit
    part = clips(name).frame_energy(frame, hop, got.size // 2, got.size - got.size // 2)
    assert part.tobytes() == got[got.size // 2:].tobytes()


def test_zero_frames_are_exactly_zero(clips):
    e = clips("lead_trail").frame_energy(600, 300)
    assert e.size == 159 and np.all(e[:38] == 0) and np.all(e[120:] == 0) and np.all(e[40:118] > 0)
    assert np.all(clips("zeros").frame_energy(600, 300) == 0)


def test_energy_does_not_depend_on_position(ctx):
    rng = np.random.Generator(np.random.PCG64(5))
    frame = rng.standard_normal(600).astype(np.float32)
    got = []
    for i, off in enumerate((0, 1, 299, 300, 4097)):
        x = (0.3 * np.random.Generator(np.random.PCG64(100 + i)).standard_normal(6000)).astype(np.float32)      # a different clip each time
        x[off:off + 600] = frame
        c = T.Clip(ctx, x, TC.SR)
        got.append(c.frame_energy(600, 1, off, 1))          # hop 1: frame `off` starts at sample `off`
        if off == 300:
            assert c.frame_energy(600, 300, 1, 1).tobytes() == got[-1].tobytes()
        c.close()
    assert all(g.tobytes() == got[0].tobytes() for g in got), got
    assert got[0][0] == pytest.approx(float((frame.astype(np.float64) ** 2).mean()), rel=1e-12)


# ---- structure ----------------------------------------------------------------------------------------------------------------------------------
def test_launch_count_does_not_depend_on_the_length(clips):
    short, long_ = clips("short"), clips("long")
    short.bounds(600, 300, 60.0)
    long_.bounds(600, 300, 60.0)
    assert short.launches == long_.launches == 2
    assert len(short) == 100 and len(long_) == 700000 and long_.device_ptr != 0


def test_read_returns_the_upload(clips):
    x = TC.case("noise_floor")[1]
    c = clips("noise_floor")
    assert c.read().tobytes() == x.tobytes()
    assert c.read(11987, 5).tobytes() == x[11987:11992].tobytes() and c.read(x.size, 0).size == 0
    out = np.zeros(4, np.float32)
    assert c.ctx.lib.mia_clip_read(c.h, x.size - 3, 4, out.ctypes.data) == BAD and c.ctx.lib.mia_clip_read(c.h, 0, 4, None) == BAD


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_launch_nothing(ctx, clips):
    lib, c = ctx.lib, clips("lead_trail")
    x = np.zeros(16, np.float32)
    assert not lib.mia_clip_create(ctx.h, None, 16, TC.SR)
    assert not lib.mia_clip_create(ctx.h, x.ctypes.data, 0, TC.SR)
    assert not lib.mia_clip_create(ctx.h, x.ctypes.data, -4, TC.SR)
    assert not lib.mia_clip_create(ctx.h, x.ctypes.data, 16, 0)
    assert not lib.mia_clip_create(ctx.h, x.ctypes.data, (1 << 26) + 1, TC.SR)                 # refused before x is read
    s, e, f = C.c_int64(-7), C.c_int64(-7), C.c_int(-7)
    call = lambda frame, hop, top_db, ps=C.byref(s), pe=C.byref(e), pf=C.byref(f): lib.mia_clip_speech_bounds(c.h, frame, hop, top_db, ps, pe, pf)
    for args in ((0, 300, 60.0), (-600, 300, 60.0), (600, 0, 60.0), (600, -1, 60.0), ((1 << 20) + 1, 300, 60.0), (600, 300, float("nan")),
                 (600, 300, float("inf")), (600, 300, float("-inf"))):
        assert call(600, 300, 60.0) == 0 and c.launches == 2
        assert call(*args) == BAD, args
        assert c.launches == 0, args                                                             # nothing was launched
    for nulls in (dict(ps=None), dict(pe=None), dict(pf=None)):
        assert call(600, 300, 60.0) == 0 and c.launches == 2
        assert call(600, 300, 60.0, **nulls) == BAD and c.launches == 0
    assert (s.value, e.value, f.value) == (11700, 36000, 1)                                      # a refused call writes nothing
    assert lib.mia_clip_speech_bounds(None, 600, 300, 60.0, C.byref(s), C.byref(e), C.byref(f)) == BAD
    out = np.full(4, -1.0)
    nf = R.num_frames(len(c), 600, 300)
    for first, count in ((-1, 1), (nf, 1), (nf - 1, 2), (0, 0), (0, nf + 1)):
        assert lib.mia_clip_frame_energy(c.h, 600, 300, first, count, out.ctypes.data) == BAD, (first, count)
    assert lib.mia_clip_frame_energy(c.h, 600, 300, 0, 1, None) == BAD and lib.mia_clip_frame_energy(c.h, 0, 300, 0, 1, out.ctypes.data) == BAD
    assert np.all(out == -1.0)
    assert call(1 << 20, 1, 60.0) == 0 and f.value == 1                                          # the largest frame is accepted: one short frame


def test_too_many_frames_is_unsupported(ctx):
    c = T.Clip(ctx, np.zeros((1 << 22) + 8, np.float32), TC.SR)
    s, e, f = C.c_int64(0), C.c_int64(0), C.c_int(0)
    assert ctx.lib.mia_clip_speech_bounds(c.h, 1, 1, 60.0, C.byref(s), C.byref(e), C.byref(f)) == UNSUPPORTED and c.launches == 0
    assert c.bounds(9, 1, 60.0) == (0, (1 << 22), True)                                          # exactly 2^22 frames, all on the floor
    c.close()


def test_non_finite_sample_is_invalid_audio(ctx):
    x = TC.case("lead_trail")[1].copy()
    x[20000] = np.nan
    c = T.Clip(ctx, x, TC.SR)
    with pytest.raises(_lib.MiaError) as err:
        c.bounds(600, 300, 60.0)
    assert err.value.code == INVALID_AUDIO
    c.close()
    x[20000] = np.inf
    with pytest.raises(_lib.MiaError) as err:
        T.trim_silence(ctx, x, TC.SR)
    assert err.value.code == INVALID_AUDIO
    y = TC.case("tail_click")[1].copy()
    y[-1] = np.nan                                           # behind the last whole frame: in no frame, never seen
    assert T.find_speech_bounds(ctx, y, TC.SR, T.CHATTERBOX) == (0, 12000)


def test_negative_top_db_finds_nothing(ctx, clips):
    x = TC.case("frame_hop_m1")[1]
    assert clips("frame_hop_m1").bounds(600, 300, -1.0) == (0, 0, False)
    cfg = T.AudioTrimConfig(top_db=-1.0)
    assert T.find_speech_bounds(ctx, x, TC.SR, cfg) is None
    got = T.trim_silence(ctx, x, TC.SR, cfg)                 # the reference's fall-back: frames 0 .. numFrames - 1, audio[0 : numFrames * hop]
    assert got.tobytes() == x[:300].tobytes() == R.trim_literal(x, 600, 300, -1.0).tobytes()
    z = TC.case("lead_trail")[1]
    assert T.trim_silence(ctx, z, TC.SR, cfg).tobytes() == z[:159 * 300].tobytes()
    assert clips("lead_trail").bounds(600, 300, 0.0)[2]     # top_db 0: the loudest frame qualifies


# ---- Python layer ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["noise_floor", "no_silence", "short"])
def test_python_functions_agree_with_the_handle(ctx, clips, ref, name):
    x = TC.case(name)[1]
    start, end, found = clips(name).bounds(600, 300, 60.0)
    assert found and clips(name).speech_bounds(T.DEFAULT) == (start, end) == ref[name]
    assert T.find_speech_bounds(ctx, x, TC.SR, T.DEFAULT) == (start, end)
    got = T.trim_silence(ctx, x, TC.SR, T.DEFAULT)
    assert got.tobytes() == x[start:end].tobytes() == R.trim_literal(x, 600, 300, 60.0).tobytes()


def test_python_early_returns(ctx):
    empty = np.zeros(0, np.float32)
    assert T.trim_silence(ctx, empty, TC.SR).size == 0 and T.find_speech_bounds(ctx, empty, TC.SR) is None
    x = TC.case("lead_trail")[1]
    tiny = T.AudioTrimConfig(hop_length=1e-6)                # hop of 0 samples
    assert T.trim_silence(ctx, x, TC.SR, tiny).tobytes() == x.tobytes() and T.find_speech_bounds(ctx, x, TC.SR, tiny) is None


def test_reference_tone_cases(ctx):
    import json
    import os
    gold = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "audio_trimmer_cases.json")))
    sr, tone = gold["sample_rate"], gold["tone"]
    sec = lambda n: float(np.float32(n) / np.float32(sr))

    def build(parts):
        out = []
        for kind, seconds in parts:
            n = int(np.float32(seconds) * np.float32(sr))
            out.append(TC.tone(n, tone["level"], sr, tone["freq"]) if kind == "tone" else TC.zeros(n))
        return np.concatenate(out)
    for case in tone["trim_silence"]:
        x = build(case["parts"])
        d = sec(T.trim_silence(ctx, x, sr).size)
        print(f"trim_silence {case['name']}: {sec(x.size)} s -> {d} s")
        if case.get("shorter"):
            assert d < sec(x.size)
        if "duration_gt" in case:
            assert case["duration_gt"] < d < case["duration_lt"]
        if "duration_equals_original_within" in case:
            assert abs(d - sec(x.size)) <= case["duration_equals_original_within"]
        if case.get("not_empty"):
            assert d > 0
    for case in tone["speech_bounds"]:
        start, end = T.find_speech_bounds(ctx, build(case["parts"]), sr)
        assert case["start_gt"] < sec(start) < case["start_lt"] and case["end_gt"] < sec(end) < case["end_lt"]
    for case in tone["trim"]:
        x = np.full(sr * case["seconds"], case["constant"], np.float32)
        r = T.trim(ctx, x, sr, case["max_duration"])
        assert r.audio.size > 0 and r.sample_rate == sr and r.transcription is None and r.words is None and not r.clipped_at_word_boundary
        assert r.original_duration > 0 and r.trimmed_duration > 0
        if "trimmed_duration_le" in case:
            assert r.trimmed_duration <= case["trimmed_duration_le"]
