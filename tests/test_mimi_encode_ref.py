"""The NumPy restatement of the Mimi encoder (tests/_mimi_encode_ref.py) against the rules it restates, on the CPU: the length chain
against a literal getExtraPaddingForConv1d, the edge padding, the argmin's tie rule, the round trip's length, the synthetic weights'
two generators, and the float32-vs-float64 numbers from which test_mimi_encode_gpu.py takes its tolerances (printed: run with -s)."""
import math

import numpy as np

import _mimi_cases as mc
import _mimi_encode_cases as ec
from _mimi_encode_ref import MimiEncodeRef, chain_lengths, extra_padding, streamable_conv1d
from _mimi_ref import MimiRef


def _literal_out_len(length, k, stride):
    """Rows of StreamableConv1d.callAsFunction: pad k - stride in front, getExtraPaddingForConv1d behind, then a plain convolution."""
    total = k - stride
    padded = length + total + extra_padding(length, k, stride, total)
    return (padded - k) // stride + 1


def test_length_chain_against_the_literal_padding_rule():
    cfg = ec.config("mimi_micro")
    oracle = ec.oracle("mimi_micro")
    for n in range(1, 3 * cfg.samples_per_frame + 2):
        L = n
        for r in reversed(cfg.seanet.ratios):
            assert extra_padding(L, 2 * r, r, r) == math.ceil(L / r) * r - L
            L = _literal_out_len(L, 2 * r, r)
        for k in (cfg.seanet.ksize, cfg.seanet.residual_ksize, 1):
            assert extra_padding(n, k, 1, k - 1) == 0 and _literal_out_len(n, k, 1) == n          # stride 1: nothing behind
        T = _literal_out_len(L, 2 * cfg.upsample_stride, cfg.upsample_stride)
        assert (L, T) == chain_lengths(cfg, n)
        if n in (1, 5, 12, 13, 25, 37):
            x = oracle.seanet(ec.pcm("mimi_micro", n))
            assert x.shape == (L, cfg.seanet.dimension) and oracle.downsample(x).shape[0] == T
    assert chain_lengths(ec.config("mimi_202407"), 3 * 1920) == (6, 3) and chain_lengths(ec.config("mimi_202407"), 3 * 1920 + 777) == (7, 4)
    assert chain_lengths(ec.config("mimi_202407"), 1) == (1, 1) and chain_lengths(ec.config("mimi_202407"), 240000) == (250, 125)


def test_edge_padding_is_numpy_edge_mode():
    rng = np.random.default_rng(0)
    w = rng.standard_normal((6, 4, 6))
    for P in (1, 2, 3, 7, 8):
        x = rng.standard_normal((P, 6))
        back = math.ceil(P / 2) * 2 - P
        staged = np.pad(x, ((2, back), (0, 0)), mode="edge")
        assert np.array_equal(staged[:2], np.stack([x[0], x[0]])) and (back == 0 or np.array_equal(staged[-1], x[-1]))
        ref = np.stack([sum(staged[2 * t + k] @ w[:, k, :].T for k in range(4)) for t in range(math.ceil(P / 2))])
        assert np.allclose(streamable_conv1d(x, w, None, 2, mode="edge"), ref, rtol=0, atol=1e-12)
        assert not np.allclose(streamable_conv1d(x, w, None, 2, mode="constant"), ref)


def test_argmin_takes_the_lowest_index_on_equal_distances():
    cfg, w = ec.config("mimi_micro"), dict(ec.weights("mimi_micro"))
    z = ec.latent_draw("mimi_micro", 4, 0)
    for stage, p in ((0, "quantizer.rvq_first.vq.layers.0.codebook."), (2, "quantizer.rvq_rest.vq.layers.1.codebook.")):
        win = int(MimiEncodeRef(cfg, w).quantize(z)[0][stage, 0])
        twin = (win + cfg.quantizer_bins // 2) % cfg.quantizer_bins
        for t in ("embedding_sum", "cluster_usage"):
            a = w[p + t].copy()
            a[twin] = a[win]
            w[p + t] = a
        codes, gap, _ = MimiEncodeRef(cfg, w).quantize(z)
        assert codes[stage, 0] == min(win, twin) and gap[stage, 0] == 0.0
    # the codes of the first n stages do not depend on the later ones
    full = MimiEncodeRef(cfg, w).quantize(z)[0]
    for k in (1, 2, 3):
        assert np.array_equal(MimiEncodeRef(cfg, w).quantize(z, n_q=k)[0], full[:k])


def test_round_trip_length_is_the_input_rounded_up_to_frames():
    cfg, w = ec.config("mimi_micro"), ec.weights("mimi_micro")
    dec = MimiRef(cfg, w)
    for n in (1, 12, 13, 12 * 9, 12 * 9 + 5):
        codes = ec.oracle("mimi_micro").encode(ec.pcm("mimi_micro", n))
        assert codes.shape == (cfg.quantizer_nq, math.ceil(n / cfg.samples_per_frame))
        assert dec.decode(codes).size == math.ceil(n / cfg.samples_per_frame) * cfg.samples_per_frame


def test_encoder_tensors_come_from_a_second_generator():
    """mimi_weights(encoder=True) adds tensors and changes none: the decode tests' checkpoints are the same bits."""
    for name in ("mimi_micro", "mimi_202407"):
        plain, both = mc.weights(name), ec.weights(name)
        assert set(plain) < set(both)
        assert all(np.array_equal(plain[k], both[k]) for k in plain)
        added = set(both) - set(plain)
        assert all(k.startswith(("encoder.", "encoder_transformer.", "downsample.")) or ".input_proj." in k for k in added)


def test_float32_noise_of_the_oracle_is_what_the_gpu_tolerances_assume():
    """Prints the tables of test_mimi_encode_gpu.py's docstring and checks that the constants there still cover them."""
    import test_mimi_encode_gpu as G
    worst = {}
    for name, n in ec.LATENT_CASES:
        gap = ec.rel_gap(ec.latent_ref(name, n, np.float32), ec.latent_ref(name, n))
        print(f"latent {name} n={n}: float32-vs-float64 {gap:.3e}, rms {np.sqrt((ec.latent_ref(name, n) ** 2).mean()):.2f}")
        worst[name] = max(worst.get(name, 0.0), gap)
    for name, g in worst.items():
        assert 8 * g <= G.TOL[name] * 1.01 and G.TOL[name] <= 8 * g * 1.25, (name, g, G.TOL[name])
    quant = [ec.quant_ref(*c) for c in ec.QUANT_CASES]
    gap_tol = 8.0 * max(noise for _, _, noise in quant)
    for (name, T, seed), (codes, gap, noise) in zip(ec.QUANT_CASES, quant):
        flips = int((ec.oracle(name, np.float32).quantize(ec.latent_draw(name, T, seed))[0] != codes).sum())
        print(f"quantize {name} T={T} seed={seed}: noise {noise:.2e}, smallest gap {gap.min():.2e}, float32 flips {flips}, GAP_TOL {gap_tol:.2e}")
        assert gap.min() > gap_tol and flips == 0
    enc = [ec.encode_ref(*c) for c in ec.ENCODE_CASES]
    for (name, n), (codes, gap, noise) in zip(ec.ENCODE_CASES, enc):
        print(f"encode {name} n={n}: noise {noise:.2e}, smallest gap {gap.min():.2e}")
        assert gap.min() > 8.0 * max(x for _, _, x in enc)
