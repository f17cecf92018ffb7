"""Cases of the Marvis tests on packed 6-bit weights (tests/test_marvis_packed_gpu.py): the synthetic checkpoints of _marvis_cases with every
Linear -- the stack Linears, `projection`, `codebook0_head` -- quantised to 6 bits (group 64, f16 scales / biases), as the published
checkpoints store them.  Embedding tables and `audio_head` stay dense and rounded to the dtype.  The oracle (_marvis_ref.MarvisRef, float64)
gets the fp32 de-quantised Linears, which is what the packed frame multiplies: no weight is rounded to 16 bit on that path.

Bounds, all on max |logit error| / std(logits) per head:
 * packed frame, prompt walked through the packed step: the step chain's own TOL of _marvis_cases (0.08 bf16, 0.015 f16);
 * packed frame behind the default prompt pass, which runs on the 16-bit copy (de-quantised weights rounded to the dtype, so the prompt's
   K / V rows carry that rounding): the LM packed-step test's bound against its oracle (tests/test_lm_gpu.py), TOL_PROMPT_PASS.
DERIVED_PROMPT_PASS is what the rule for a wider bound would allow had the chained stacks needed one (derived_bound16 below: the oracle's
float64 run against its own run with every Linear and every activation rounded to the dtype -- more rounding than the GPU path has -- times
4); computed on the CPU, on record only, never taken from GPU output."""
import functools
from unittest import mock

import numpy as np

import _marvis_cases as MC
import _marvis_ref as R
import _quant6 as Q6

TOL_PROMPT_PASS = {"bf16": 0.08, "f16": 0.02}
DERIVED_PROMPT_PASS = {("marvis-micro", "f16"): 0.0236, ("marvis-micro", "bf16"): 0.1386, ("marvis-micro128", "f16"): 0.0178, ("marvis-micro128", "bf16"): 0.1862}

# Peaked checkpoints (seeds found on the CPU, on the oracle alone) on which every draw of the runs below is safe for logits anywhere
# within TOL_PROMPT_PASS["f16"]: SAMPLED among seeds 0 .. 600 (6 frames x 5 codebooks, two uniform tables whose frames part); STOP among
# seeds 0 .. 200 at 2 codebooks and temperature 2.0 -- the oracle draws two frames and then the all-zero one.
SAMPLED = dict(name="marvis-micro", dtype="f16", temperature=0.9, top_p=0.6, weight_seed=140, choice_seeds=(0, 1))
STOP = dict(name="marvis-micro", dtype="f16", codebooks=2, temperature=2.0, top_p=0.8, weight_seed=148)


def stop_want(f, i, ids):
    """the all-zero frame from the second frame on wherever id 0 is a safe pick; before it, an id other than 0"""
    if f >= 1 and 0 in ids:
        return 0
    nz = [t for t in ids if t != 0]
    return nz[0] if f < 1 and nz else None


def is_linear(name: str) -> bool:
    return name.endswith("_proj.weight") or name in ("projection.weight", "codebook0_head.weight")


@functools.lru_cache(maxsize=None)
def checkpoint(name, dtype, seed=3, peaked=False, quantise_embeddings=False):
    """(stored, dense): `stored` = the checkpoint under the keys of sanitize_marvis, Linears as `<p>.weight` uint32 codes + `.scales` /
    `.biases` float16, everything else fp32; `dense` = the same with the Linears de-quantised to fp32 (tests/_quant6.py), which both the
    oracle and MarvisModel.load take.  quantise_embeddings: the two embedding tables stored quantised too."""
    from mlx_swift_audio_amd import checkpoint as CK
    stored, dense = {}, {}
    for k, v in MC.weights(name, dtype, seed, peaked).items():
        if is_linear(k) or (quantise_embeddings and k.endswith("_embeddings.weight")):
            q, s, b = CK.quantize_affine(v, 64, 6, np.float16)
            assert np.array_equal(q, Q6.pack6(Q6.unpack6(q)))
            p = k[:-7]
            stored[p + ".weight"], stored[p + ".scales"], stored[p + ".biases"] = q, s, b
            dense[k] = Q6.dequant6(q, s.astype(np.float32), b.astype(np.float32)).astype(np.float32)
        else:
            stored[k] = dense[k] = v
    return stored, dense


def raw_name(k: str) -> str:
    """a key of the module schema as the published files spell it: checkpoint.sanitize_marvis_name maps it back"""
    for a, b in (("self_attn", "attn"), ("o_proj", "output_proj"), ("gate_proj", "w1"), ("down_proj", "w2"), ("up_proj", "w3"),
                 ("input_layernorm.weight", "sa_norm.scale"), ("post_attention_layernorm.weight", "mlp_norm.scale")):
        k = k.replace(a, b)
    if k in ("backbone.norm.weight", "decoder.norm.weight"):
        k = k.replace("weight", "scale")
    return "model." + k


def _with_dense(name, dtype, seed, peaked):
    """_marvis_cases' oracle-side helpers take their weights from MC.weights(name, dtype, seed, peaked): here they get the de-quantised ones"""
    dense = checkpoint(name, dtype, seed, peaked)[1]      # before the patch: checkpoint() reads MC.weights itself
    return mock.patch.object(MC, "weights", lambda *a, **k: dense)


@functools.lru_cache(maxsize=None)
def forced_run(name, dtype, codebooks=MC.N_CODEBOOKS, rnd=None, seed=3, peaked=False, round_linears=False):
    """the oracle's logits [6][codebooks][V] over the six teacher-forced frames of _marvis_cases on the de-quantised checkpoint
    (round_linears: the Linears rounded to the dtype as well, as the 16-bit copy holds them)"""
    w = checkpoint(name, dtype, seed, peaked)[1]
    if round_linears:
        w = {k: R.round_to(v, dtype).astype(np.float32) if is_linear(k) else v for k, v in w.items()}
    ref = R.MarvisRef(MC.config(name), w, rnd=rnd)
    tk, mk = MC.prompt()
    out = []
    for f in range(6):
        _, lg = ref.generate_frame(codebooks, tk, mk, lambda x, i: 0, MC.FORCED[f])
        out.append(lg)
        tk, mk = MC.feedback(MC.FORCED[f][:codebooks])
    out = np.stack(out)
    out.setflags(write=False)
    return out


def derived_bound16(name, dtype):
    """the rule of _marvis_cases.derived_bound with the weights rounded too"""
    a, b = forced_run(name, dtype), forced_run(name, dtype, rnd=dtype, round_linears=True)
    return 4.0 * float((np.abs(a - b).max(-1) / a.std(-1)).max())


def choose_uniforms(name, dtype, codebooks, n_frames, temperature, top_p, choice_seed, weight_seed, want=None, tokens=None, mask=None, tol=None):
    """_marvis_cases.choose_uniforms on the oracle with the de-quantised weights (peaked checkpoint)"""
    with _with_dense(name, dtype, weight_seed, True):
        return MC.choose_uniforms(name, dtype, codebooks, n_frames, temperature, top_p, choice_seed, weight_seed, True, want, tokens, mask, tol)
