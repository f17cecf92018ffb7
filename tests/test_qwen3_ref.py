"""The CPU reference of the Qwen3 decoder (tests/_qwen3_ref.py) pinned on the CPU: the block with the per-head q / k RMSNorm against
transformers' own Qwen3ForCausalLM (an independent implementation) on the synthetic micro checkpoints, the prompt merge, and the greedy
loop's three rules (stop id excluded, budget respected, lowest index on an exact tie).  The product's merge_embeddings is host code and is
checked against the helper's here as well."""
import dataclasses

import numpy as np
import pytest
import torch

import _qwen3_ref as R
from mlx_swift_audio_amd import synthetic as S


@pytest.mark.parametrize("cfg_name", ["qwen3-micro", "qwen3-micro128"])
def test_block_matches_transformers_qwen3(cfg_name):
    tr = pytest.importorskip("transformers")
    cfg = S.LM_CONFIGS[cfg_name]
    w = S.lm_weights(cfg, seed=3)
    hc = tr.Qwen3Config(vocab_size=cfg.vocab, hidden_size=cfg.hidden, intermediate_size=cfg.inter, num_hidden_layers=cfg.n_layers,
                        num_attention_heads=cfg.n_heads, num_key_value_heads=cfg.n_kv_heads, head_dim=cfg.head_dim,
                        max_position_embeddings=cfg.max_ctx, rms_norm_eps=cfg.rms_eps, tie_word_embeddings=True, attention_bias=False,
                        rope_parameters={"rope_type": "default", "rope_theta": cfg.rope_theta}, use_sliding_window=False)
    hc._attn_implementation = "eager"
    hf = tr.Qwen3ForCausalLM(hc).to(torch.float32).eval()
    sd = {k: torch.from_numpy(v) for k, v in w.items()}
    sd["lm_head.weight"] = sd["model.embed_tokens.weight"]
    missing, unexpected = hf.load_state_dict(sd, strict=False)
    assert not unexpected and all("rotary" in k or "inv_freq" in k for k in missing), (missing, unexpected)
    ora = R.Qwen3Oracle(cfg, w)
    ids = [5, 17, 256, 999, 2048, 3, 42, 7, 7, 1500, 11, 2999]
    with torch.no_grad():
        out = hf(input_ids=torch.tensor([ids]), use_cache=True)
        d = np.abs(ora.forward(ids).numpy() - out.logits[0].numpy()).max()
        print(cfg_name, "12 ids, max |delta|", d)
        assert d <= 1e-4, d
        past = out.past_key_values
        for t in (11, 0, 1234):                                         # single-token steps on the cache
            out = hf(input_ids=torch.tensor([[t]]), past_key_values=past, use_cache=True)
            past = out.past_key_values
            d = np.abs(ora.forward([t]).numpy()[-1] - out.logits[0, -1].numpy()).max()
            print(cfg_name, "step", t, "max |delta|", d)
            assert d <= 1e-4, d


def test_dropping_the_norm_moves_the_logits():
    """What the GPU tests rely on: an implementation that ignores q_norm / k_norm is far outside every tolerance used there."""
    from oracle import lm as OL
    cfg = S.LM_CONFIGS["qwen3-micro"]
    w = S.lm_weights(cfg, seed=2)
    ids = [5, 17, 256, 999, 2048, 3, 42, 7, 7, 1500]
    a, b = R.Qwen3Oracle(cfg, w).forward(ids).numpy()[-1], OL.LMOracle(cfg, w).forward(ids).numpy()[-1]
    assert np.abs(a - b).max() > 0.5 * a.std()


def test_merge_embeddings_marker_positions():
    from mlx_swift_audio_amd import lm as HL
    rng = np.random.default_rng(0)
    emb = rng.standard_normal((50, 8)).astype(np.float32)
    audio = rng.standard_normal((5, 8)).astype(np.float32)
    SOS, EOS = 40, 41

    def both(ids):
        got = R.merge_embeddings(emb, ids, audio, SOS, EOS)
        dec = HL.FunASRDecoder(None, emb)
        np.testing.assert_array_equal(dec.merge_embeddings(ids, audio, SOS, EOS), got)
        return got

    mid = both([1, 2, SOS, 9, 9, 9, EOS, 3, 4])                          # placeholders between the markers are replaced
    np.testing.assert_array_equal(mid, np.concatenate([emb[[1, 2, SOS]], audio, emb[[EOS, 3, 4]]]))
    ends = both([SOS, 9, EOS])                                          # markers at both ends
    np.testing.assert_array_equal(ends, np.concatenate([emb[[SOS]], audio, emb[[EOS]]]))
    adj = both([7, SOS, EOS])                                           # no placeholder at all
    np.testing.assert_array_equal(adj, np.concatenate([emb[[7, SOS]], audio, emb[[EOS]]]))
    first = both([SOS, 1, SOS, EOS, 2, EOS])                            # the FIRST occurrence of each marker counts
    np.testing.assert_array_equal(first, np.concatenate([emb[[SOS]], audio, emb[[EOS, 2, EOS]]]))
    for ids in ([1, 2, 3], [1, SOS, 3], [EOS, 2]):                      # a missing marker: text rows alone
        np.testing.assert_array_equal(both(ids), emb[ids])


def _untied(seed):
    cfg = dataclasses.replace(S.LM_CONFIGS["qwen3-micro"], tie_embeddings=False)
    return cfg, S.lm_weights(cfg, seed=seed)


def test_greedy_loop_stop_and_budget():
    cfg, w = _untied(1)
    ora = R.Qwen3Oracle(cfg, w)
    prompt = w["model.embed_tokens.weight"][[4, 5, 6, 7]]
    free = R.greedy(ora, prompt, (cfg.vocab - 1,), 12)
    assert len(free) == 12 and (cfg.vocab - 1) not in free             # the budget is respected
    assert R.greedy(ora, prompt, (cfg.vocab - 1,), 5) == free[:5]
    stop = free[6]
    k = free.index(stop)
    cut = R.greedy(ora, prompt, (stop, cfg.vocab - 1), 12)
    assert cut == free[:k] and stop not in cut                         # ends at the FIRST occurrence; the stop id is not emitted
    assert R.greedy(ora, prompt, (free[0],), 12) == []                 # a stop id as the very first pick


def test_greedy_lowest_index_wins_an_exact_tie():
    assert R.argmax_lowest(np.array([1.0, 3.0, 3.0, 2.0, 3.0], np.float32)) == 1
    cfg, w = _untied(1)
    w = dict(w)
    head = w["lm_head.weight"].copy()
    head[[9, 700, 2500]] = 40.0 * head[700]                             # three bit-identical rows that dominate whenever h . row > 0
    head[[12, 1900]] = -40.0 * head[700]                                # ... and two for the other sign
    w["lm_head.weight"] = head
    ora = R.Qwen3Oracle(cfg, w)
    margins = []
    out = R.greedy(ora, w["model.embed_tokens.weight"][[4, 5, 6]], (cfg.vocab - 1,), 8, margins)
    assert len(out) == 8 and set(out) <= {9, 12}, out                   # always the lowest index of the tied group
    assert max(margins) == 0.0                                          # every step was an exact tie
