"""OuteTTS on the GPU (mlx_swift_audio_amd/outetts.py): text + speaker profile -> ids -> (c1, c2) codes -> DAC waveform, on llama-micro
(max_ctx 1024, random-init, rounded to bf16), the toy tokenizer of tests/_outetts_ref.py (most of the 3 000-id vocabulary is code tokens,
so a random-init model does emit codes), the micro DAC with two codebooks of 1 024 entries and a seeded speaker of 6 words / 60 pairs.

The ids follow _outetts_ref.generate -- the reference's loop restated on the fp32 oracle in OuteTTS's order (temperature, then penalty) --
under test_lm_gpu.py's rule: a first difference must sit at a draw within SAMPLE_TOL (5e-3, test_generate_matches_oracle's) of a CDF
edge or the top-p cut."""
import dataclasses

import numpy as np
import pytest

import _outetts_ref as R
from mlx_swift_audio_amd import outetts as OT
from mlx_swift_audio_amd import synthetic as S

pytestmark = pytest.mark.gpu

SAMPLE_TOL = 5e-3
MAX_TOKENS = 40
SENTENCES = ["The snow fell.", "A cat sat still", "Winter came early?"]


@pytest.fixture(scope="module")
def rig(ctx):
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import codec as HC, lm as HL
    cfg = dataclasses.replace(S.LM_CONFIGS["llama-micro"], max_ctx=1024)
    assert R.VOCAB <= cfg.vocab
    w = S.lm_weights(cfg, seed=14, round_to="bf16")
    model = HL.CausalLM.load(ctx, cfg, w, m.BF16)
    dcfg = dataclasses.replace(S.DAC_CONFIGS["dac_micro"], codebook_size=1024)
    dac = HC.DACCodec.load(ctx, dcfg, S.dac_weights(dcfg, seed=4))
    spk = R.seeded_speaker(5, 6, 60)
    tts = OT.OuteTTS(model, dac, R.processor(), R.EOS_ID, default_speaker=spk)
    u = np.random.default_rng(17).random((len(SENTENCES), MAX_TOKENS)).astype(np.float32)
    yield dict(cfg=cfg, w=w, model=model, dac=dac, tts=tts, spk=spk, u=u)
    dac.close()
    model.close()


def test_generate_chunk_follows_reference_loop(rig):
    from oracle import lm as OL
    tts, u = rig["tts"], rig["u"][0]
    gen, pcm = tts.generate_chunk(SENTENCES[0], u, temperature=0.4, top_p=0.9, max_tokens=MAX_TOKENS)
    prompt = tts.processor.get_completion_prompt_tokens(SENTENCES[0], rig["spk"])
    assert len(prompt) > 150 and R.EOS_ID not in gen
    trace = []
    want = R.generate(OL.LMOracle(rig["cfg"], rig["w"]), prompt, 0.4, 0.9, MAX_TOKENS, R.EOS_ID, u, trace)
    k = next((i for i, (a, b) in enumerate(zip(gen, want)) if a != b), min(len(gen), len(want)))
    print(f"outetts generate_chunk: {len(gen)} ids, {len(want)} from the oracle, first difference at {k}" + (f", boundary distances {trace[k]}" if k < len(trace) else ""))
    if not (k == len(gen) == len(want)):
        assert min(trace[k]) < SAMPLE_TOL, (k, trace[k], gen, want)
    codes = tts.processor.extract_audio_from_tokens(gen)
    assert len(codes[0]) > 0
    want_pcm = rig["dac"].decode_from_codes(np.asarray(codes, np.int32)[None]).reshape(-1)
    assert pcm.dtype == np.float32 and pcm.size == rig["dac"].output_len(len(codes[0])) and np.array_equal(pcm, want_pcm)


def test_generate_chunks_equals_sentence_by_sentence(rig):
    """Temperature 2, top-p 0.95 here: at OuteTTS's 0.4 this random-init model (tied embeddings) mostly repeats its last id, and a
    sentence may never leave codebook 1 (the fp32 oracle gives sentence 1 no pair at all); at 2 the 40 draws are nearly all distinct and
    the oracle finds 14 or more pairs in every sentence, so all three reach the DAC on both sides."""
    tts, u = rig["tts"], rig["u"]
    kw = dict(temperature=2.0, top_p=0.95, max_tokens=MAX_TOKENS)
    rig["model"].set_batch(3)            # same handle capacity on both sides (the capacity selects the step's kernel chain)
    solo = [tts.generate_chunk(s, u[b], **kw) for b, s in enumerate(SENTENCES)]
    both = tts.generate_chunks(SENTENCES, u, **kw)
    rig["model"].set_batch(1)
    assert [g for g, _ in both] == [g for g, _ in solo]
    assert all(a.size > 0 and np.array_equal(a, b) for (_, a), (_, b) in zip(both, solo))


def test_no_code_tokens_raises(rig):
    """A processor whose tokenizer knows no <|c2_*|> token finds no second codebook in whatever the model emits."""
    p = R.processor(drop=tuple(OT.format_c2(i) for i in range(1025)))
    tts = OT.OuteTTS(rig["model"], rig["dac"], p, R.EOS_ID, default_speaker=rig["spk"])
    with pytest.raises(ValueError, match="No audio codes"):
        tts.generate_chunk(SENTENCES[0], rig["u"][0], max_tokens=8)
