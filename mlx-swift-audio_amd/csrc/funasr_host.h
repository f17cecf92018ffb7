// funasr_host.h -- host-only pieces of the Fun-ASR audio half: the front end's tables and lengths, and the shape rules of the SenseVoice
// handle.  Plain C++ (no HIP), so a stand-alone program can exercise it under the host sanitizers (tools/funasr_host_check.cpp).
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/mia.h"
#include "frontend_tables.h"      // the twiddles and the compact filter form, shared with the other front ends

namespace funasr {

constexpr int NFFT = 400, HOP = 160, NFREQ = 200, NMEL = 80, LFR_M = 7, LFR_N = 6;   // FunASRAudio.swift:13-20; bins 0..199 (:76)

// hammingWindow (STT/FunASR/FunASRAudio.swift:35-45): symmetric, 0.54 - 0.46 cos(2 pi n / (N - 1))
inline void hamming_window(std::vector<float>& w) {
  w.resize(NFFT);
  const double f = 2.0 * M_PI / (double)(NFFT - 1);
  for (int n = 0; n < NFFT; ++n) w[n] = (float)(0.54 - 0.46 * cos((double)n * f));
}

// funASRMelFilters (FunASRAudio.swift:322-396), HTK scale + Slaney normalisation -> dense [NMEL][NFREQ].  The bin frequencies are the
// reference's linspace(0, 8000, 200) (:363-364) -- 8000 / 199 Hz apart, not the DFT's 40 Hz -- reproduced as it stands.
inline void mel_filters(std::vector<float>& dense) {
  const double m_max = 2595.0 * log10(1.0 + 8000.0 / 700.0);
  std::vector<double> f(NMEL + 2);
  for (int i = 0; i < NMEL + 2; ++i) f[i] = 700.0 * (pow(10.0, (m_max * (double)i / (double)(NMEL + 1)) / 2595.0) - 1.0);
  dense.assign((size_t)NMEL * NFREQ, 0.0f);
  for (int m = 0; m < NMEL; ++m) {
    const double enorm = 2.0 / (f[m + 2] - f[m]);
    for (int k = 0; k < NFREQ; ++k) {
      const double hz = 8000.0 * (double)k / (double)(NFREQ - 1);
      const double down = (hz - f[m]) / (f[m + 1] - f[m]), up = (f[m + 2] - hz) / (f[m + 2] - f[m + 1]);
      const double w = fmax(0.0, fmin(down, up)) * enorm;
      dense[(size_t)m * NFREQ + k] = (float)w;
    }
  }
}

inline int64_t n_frames(int64_t n_samples) { return 1 + n_samples / HOP; }                       // :262 after the 200 + 200 reflect pad
inline int64_t t_lfr(int64_t n_samples) { return (n_frames(n_samples) + LFR_N - 1) / LFR_N; }    // :117

// FSMN context (MultiHeadAttentionSANM.swift:73-79)
inline int fsmn_left(int kernel_size, int sanm_shift) { return (kernel_size - 1) / 2 + (sanm_shift > 0 ? sanm_shift : 0); }

// shape rules of mia_sensevoice_load; nullptr when the handle can be built
inline const char* config_check(const mia_sensevoice_config& c) {
  if (c.input_dim <= 0 || c.input_dim % 4 || c.input_dim > 4096) return "input_dim must be a positive multiple of 4, <= 4096";
  if (c.n_heads <= 0 || c.encoder_dim != c.n_heads * 128) return "encoder_dim must be n_heads * 128 (head dim 128)";
  if (c.encoder_dim > 4096) return "encoder_dim must be <= 4096";
  if (c.ffn_dim <= 0 || c.ffn_dim % 64) return "ffn_dim must be a positive multiple of 64";
  if (c.kernel_size <= 0 || c.sanm_shift < 0) return "kernel_size must be > 0 and sanm_shift >= 0";
  if (c.kernel_size - 1 - fsmn_left(c.kernel_size, c.sanm_shift) < 0) return "sanm_shift leaves a negative right context (kernel_size - 1 - left < 0)";
  if (c.n_encoders0 != 1 || c.n_encoders < 0 || c.n_tp_encoders < 0) return "n_encoders0 must be 1; n_encoders, n_tp_encoders >= 0";
  if (c.adaptor_k <= 0 || c.adaptor_k > 64) return "adaptor_k must be in 1..64";
  if (c.adaptor_heads <= 0 || c.llm_dim != c.adaptor_heads * 128) return "llm_dim must be adaptor_heads * 128 (head dim 128)";
  if (c.llm_dim % 256 || c.llm_dim > 4096) return "llm_dim must be a multiple of 256 (block ffn = llm_dim / 4, a multiple of 64), <= 4096";
  if (c.adaptor_ffn_dim <= 0 || c.adaptor_ffn_dim % 64) return "adaptor_ffn_dim must be a positive multiple of 64";
  if (c.adaptor_layers < 0) return "adaptor_layers must be >= 0";
  return nullptr;
}

}  // namespace funasr
