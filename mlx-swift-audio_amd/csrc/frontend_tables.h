// frontend_tables.h -- host-only builders of the front ends' tables (windows, twiddles, DFT rows, filterbanks), one copy each.  Plain
// C++ (no HIP), so a stand-alone program can exercise it under the host sanitizers (tools/frontend_tables_check.cpp).  The fp32
// expressions keep the order of the Swift they restate: the operation order is what makes the tables what the tests pin.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace fe {

// Whisper's Hann (WhisperAudio.swift:32-44): symmetric, 0.5 (1 - cos(2 pi i / (n - 1)))
inline void hann_symmetric(int n, std::vector<float>& w) {
  w.resize(n);
  const float factor = 2.0f * (float)M_PI / (float)(n - 1);
  for (int i = 0; i < n; ++i) w[i] = 0.5f * (1.0f - cosf((float)i * factor));
}

// hanningWindow(n + 1)[0..<n] (S3TokenizerUtils.swift:117,213-221): periodic
inline void hann_periodic(int n, std::vector<float>& w) {
  w.resize(n);
  const int Lw = n + 1;
  const float factor = (float)M_PI / (float)(Lw - 1);
  for (int i = 0; i < n; ++i) w[i] = 0.5f + 0.5f * cosf((float)(1 - Lw + 2 * i) * factor);
}

// CAM++'s Povey window: a symmetric Hann to the power 0.85
inline void povey_window(int n, std::vector<float>& w) {
  w.resize(n);
  for (int i = 0; i < n; ++i) w[i] = powf(0.5f - 0.5f * cosf(2.0f * (float)M_PI * (float)i / (float)(n - 1)), 0.85f);
}

// 400-point twiddles [k][cos | sin][nbp] of the log-mel kernels; k j is reduced mod 400 before the angle is formed (exact), and the
// columns from n_live_bins up stay zero
inline void twiddle_400(int n_live_bins, int nbp, std::vector<float>& tw) {
  constexpr int N = 400;
  tw.assign((size_t)N * 2 * nbp, 0.0f);
  for (int k = 0; k < N; ++k)
    for (int j = 0; j < n_live_bins; ++j) {
      const double ang = 2.0 * M_PI * (double)(k * j % N) / (double)N;
      tw[((size_t)k * 2 + 0) * nbp + j] = (float)cos(ang);
      tw[((size_t)k * 2 + 1) * nbp + j] = (float)sin(ang);
    }
}

// DFT basis rows [2 nbp][stride] of the front ends that transform with a GEMM: row k = cos(2 pi k n / nfft) win[n], row nbp + k =
// -sin(..) win[n] for the bins k < n_bins and the samples n < n_live; everything else zero.  win == nullptr: no window folded in.
inline void dft_rows(int nfft, int n_bins, int nbp, int n_live, int stride, const float* win, std::vector<float>& dft) {
  dft.assign((size_t)2 * nbp * stride, 0.0f);
  for (int k = 0; k < n_bins; ++k)
    for (int n = 0; n < n_live; ++n) {
      const double ang = 2.0 * M_PI * (double)((int64_t)k * n % nfft) / (double)nfft, wn = win ? (double)win[n] : 1.0;
      dft[(size_t)k * stride + n] = (float)(cos(ang) * wn);
      dft[(size_t)(nbp + k) * stride + n] = (float)(-sin(ang) * wn);
    }
}

// Slaney mel scale + Slaney normalisation in fp32 scalar math (S3TokenizerUtils.swift:301-375), f_min 0 -> dense [n_mels][n_bins]
inline void slaney_filters(int n_mels, int n_bins, float sample_rate, int n_fft, float f_max, std::vector<float>& dense) {
  const float f_sp = 200.0f / 3.0f, min_log_hz = 1000.0f;
  const float min_log_mel = min_log_hz / f_sp;
  const float logstep = logf(6.4f) / 27.0f;
  auto hz_to_mel = [&](float hz) { return hz >= min_log_hz ? min_log_mel + logf(hz / min_log_hz) / logstep : hz / f_sp; };
  auto mel_to_hz = [&](float mel) { return mel >= min_log_mel ? min_log_hz * expf(logstep * (mel - min_log_mel)) : f_sp * mel; };
  const float mel_min = hz_to_mel(0.0f), mel_max = hz_to_mel(f_max);
  std::vector<float> pts(n_mels + 2);
  for (int i = 0; i < n_mels + 2; ++i) pts[i] = mel_to_hz(mel_min + (float)i * (mel_max - mel_min) / (float)(n_mels + 1));
  dense.assign((size_t)n_mels * n_bins, 0.0f);
  for (int m = 0; m < n_mels; ++m) {
    const float fl = pts[m], fc = pts[m + 1], fr = pts[m + 2];
    const float enorm = 2.0f / (pts[m + 2] - pts[m]);
    for (int k = 0; k < n_bins; ++k) {
      const float freq = (float)k * sample_rate / (float)n_fft;
      float w = 0.0f;
      if (freq >= fl && freq <= fc) w = (freq - fl) / (fc - fl);
      else if (freq > fc && freq <= fr) w = (fr - freq) / (fr - fc);
      dense[(size_t)m * n_bins + k] = w * enorm;
    }
  }
}

// CAM++'s HTK triangles on ROUNDED FFT-bin edges, no normalisation (computeMelFiltersHTK) -> dense [n_mels][n_bins]
inline void htk_bin_filters(int n_mels, int n_bins, float sample_rate, int n_fft, float f_min, float f_max, std::vector<float>& dense) {
  auto hz_to_mel = [](float hz) { return 2595.0f * log10f(1.0f + hz / 700.0f); };
  auto mel_to_hz = [](float mel) { return 700.0f * (powf(10.0f, mel / 2595.0f) - 1.0f); };
  const float mel_min = hz_to_mel(f_min), mel_max = hz_to_mel(f_max);
  std::vector<int> bins(n_mels + 2);
  for (int i = 0; i < n_mels + 2; ++i) bins[i] = (int)roundf(mel_to_hz(mel_min + (float)i * (mel_max - mel_min) / (float)(n_mels + 1)) * (float)n_fft / sample_rate);
  dense.assign((size_t)n_mels * n_bins, 0.0f);
  for (int q = 1; q <= n_mels; ++q) {
    const int lo = bins[q - 1], c = bins[q], hi = bins[q + 1];
    float* row = dense.data() + (size_t)(q - 1) * n_bins;
    if (c != lo) for (int k = lo; k < c; ++k) if (k >= 0 && k < n_bins) row[k] = (float)(k - lo) / (float)(c - lo);
    if (hi != c) for (int k = c; k < hi; ++k) if (k >= 0 && k < n_bins) row[k] = (float)(hi - k) / (float)(hi - c);
  }
}

// dense rows -> the compact form the kernels stage: meta [n_filters][3] = (first bin, count, offset into w), w = the weights of
// [first, first + count) back to back.  An all-zero filter is (0, 0, offset); w never comes out empty (one 0.0f).
inline void compact_filters(const std::vector<float>& dense, int n_filters, int n_bins, std::vector<float>& w, std::vector<int>& meta) {
  w.clear();
  meta.assign((size_t)n_filters * 3, 0);
  for (int m = 0; m < n_filters; ++m) {
    const float* row = dense.data() + (size_t)m * n_bins;
    int lo = -1, hi = -1;
    for (int k = 0; k < n_bins; ++k)
      if (row[k] != 0.0f) { if (lo < 0) lo = k; hi = k; }
    if (lo < 0) { lo = 0; hi = -1; }
    meta[m * 3 + 0] = lo; meta[m * 3 + 1] = hi - lo + 1; meta[m * 3 + 2] = (int)w.size();
    w.insert(w.end(), row + lo, row + hi + 1);
  }
  if (w.empty()) w.push_back(0.0f);
}

// the last bin any filter of a compact bank touches (0 for an all-zero bank): what a transform restricted to the live bins must reach
inline int last_live_bin(const std::vector<int>& meta) {
  int kmax = 0;
  for (size_t m = 0; m < meta.size() / 3; ++m) kmax = std::max(kmax, meta[m * 3] + meta[m * 3 + 1] - 1);
  return kmax;
}

}  // namespace fe
