"""The packed Whisper step at the DECODER shape of large-v3-turbo (D 1280, 20 heads, 4 layers, vocabulary 51 866), at 4 and 8 bit, with
batches of 3 and of 40 clips: the variants of dec_skinny_fq (csrc/skinny_frag_quant.hip) that the micro checkpoints of
tests/test_whisper_packed_gpu.py (D 128: one block, one wave, at most 16 rows) never launch --
  * 10 and 40 blocks per row: 5 waves per workgroup summed through LDS, 2 blocks per wave through the register ring (q|k|v, cross q, fc1:
    10 blocks = 5 x 2), 1 block per wave behind a 2-way (attention outputs) and a 4-way (fc2: 4 x 5 x 2) cross-workgroup split;
  * above 16 rows: the second 16-row half (activation fragments at + 512, acc[t][1]), a second 32-row block (blockIdx.z = 1, rows 32..39),
    and the 4-tile one-wave logits variant, whose last workgroup holds tiles 3240..3243 of 3242 (the tile clamp);
  * at most 16 rows: the one-tile logits variant over 3242 workgroups.
The encoder is cut to one layer and 100 positions: it does not run on packed weights, and every GEMM of the decode step has large-v3-turbo's
own N and K.  Traced clips sit in each region (rows 5, 20, 37, 39 of 40).  Every position's logits against the oracle on the de-quantised
weights with the shared tolerance (decoder alone: both sides attend the same features), the head replayed exactly, forks from the
oracle's free run explained by the measured errors (tests/_whisper_trace.py).  About 20 s per case, most of it building and
quantising the checkpoint on the host (6-7 s of it in the test body on the GPU machine)."""
import numpy as np
import pytest
import torch

from oracle import whisper as OW

from _whisper_packed import quantised_checkpoint
from _whisper_trace import assert_fork_explained, check_clip, first_fork

pytestmark = pytest.mark.gpu

DIMS = OW.ModelDimensions(128, 100, 1280, 20, 1, 51866, 448, 1280, 20, 4)
N_NEW = 12


@pytest.mark.parametrize("bits,dtype_name", [(4, "bf16"), (8, "f16")])
def test_packed_step_at_turbo_decoder_shape(ctx, bits, dtype_name):
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import whisper as HW
    dense, packed = quantised_checkpoint(DIMS, 3, bits, dtype_name)
    ora = OW.WhisperOracle(DIMS, dense)
    st = OW.SpecialTokens.for_vocab(DIMS.n_vocab)
    kw = dict(timestamps=False, suppress_ids=OW.synthetic_suppress_list(st), blank_ids=[220, 50255], max_new_tokens=N_NEW)
    oo = OW.DecodingOptions(**kw)
    model = HW.WhisperModel.load(ctx, DIMS, dense, m.BF16 if dtype_name == "bf16" else m.F16)
    model.attach_quantized(packed)
    model.use_packed(True)
    rng = np.random.default_rng(7)
    for n_clips, traced in ((40, [5, 20, 37, 39]), (3, [0, 2])):
        mel = OW.round_array((0.5 * rng.standard_normal((n_clips, 2 * DIMS.n_audio_ctx, DIMS.n_mels))).astype(np.float32), dtype_name)
        model.trace_logits(traced)
        res = HW.GreedyDecoder(model, HW.DecodingOptions(**kw)).decode(mel)
        feats = model.audio_features()
        assert len(res) == n_clips and all(len(r.tokens) > 0 for r in res)
        for slot, b in enumerate(traced):
            xa = torch.from_numpy(feats[b:b + 1])
            info = check_clip(model, ora, st, oo, res[b], slot, xa, dtype_name, N_NEW)
            print(f"packed turbo-decoder {bits} bit {dtype_name} B {n_clips} row {b}: rel_rms {info['rel_rms_max']:.5f} rel_max {info['rel_max_max']:.5f}")
            ref = OW.greedy_decode(ora, st, xa, oo)
            k = first_fork(res[b].tokens, ref.tokens)
            if k is not None:
                assert_fork_explained(info, ref, k)
        model.trace_logits([])
    model.close()
