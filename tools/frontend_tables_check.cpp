// frontend_tables_check.cpp -- stand-alone exerciser of the host-only table builders of the front ends (csrc/frontend_tables.h, and the
// Fun-ASR window and filterbank of csrc/funasr_host.h), with each front end's own sizes.  Meant for the host sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include tools/frontend_tables_check.cpp -o frontend_tables_check
//   frontend_tables_check tables.bin
// Checks the rules the kernels rely on (exit status 1 on a broken one) and writes every table to the file: records of a text line
// "name f32|i32 count\n" followed by count 4-byte values.  tests/test_frontend_tables_host.py compares them with the oracle's.
#include <cstdio>
#include <cstdlib>

#include "../mlx-swift-audio_amd/csrc/funasr_host.h"

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } \
  } while (0)

static FILE* g_out;
static void put(const char* front, const char* name, const char* type, const void* p, size_t n) {
  fprintf(g_out, "%s_%s %s %zu\n", front, name, type, n);
  fwrite(p, 4, n, g_out);
}
static void put(const char* front, const char* name, const std::vector<float>& v) { put(front, name, "f32", v.data(), v.size()); }
static void put(const char* front, const char* name, const std::vector<int>& v) { put(front, name, "i32", v.data(), v.size()); }

constexpr int kStagedNnz = 1024;      // MAX_NNZ of logmel.hip and funasr_frontend.hip: the filter weights they stage in LDS

// compact form of a dense bank: it reproduces the dense rows exactly, everything outside [first, first + count) is zero; writes both
static int bank(const char* front, const char* suffix, const std::vector<float>& dense, int n_filters, int n_bins, int max_nnz, std::vector<int>& meta) {
  std::vector<float> w;
  fe::compact_filters(dense, n_filters, n_bins, w, meta);
  CHECK(dense.size() == (size_t)n_filters * n_bins && meta.size() == (size_t)n_filters * 3 && !w.empty());
  size_t nnz = 0;
  for (int m = 0; m < n_filters; ++m) {
    const int lo = meta[m * 3], cnt = meta[m * 3 + 1], off = meta[m * 3 + 2];
    CHECK(lo >= 0 && cnt >= 0 && lo + cnt <= n_bins && off == (int)nnz && (size_t)(off + cnt) <= w.size());
    for (int c = 0; c < cnt; ++c) CHECK(w[off + c] == dense[(size_t)m * n_bins + lo + c]);
    for (int k = 0; k < n_bins; ++k) if (k < lo || k >= lo + cnt) CHECK(dense[(size_t)m * n_bins + k] == 0.0f);
    if (cnt > 0) CHECK(w[off] != 0.0f && w[off + cnt - 1] != 0.0f);
    nnz += (size_t)cnt;
  }
  CHECK(nnz == w.size() || (nnz == 0 && w.size() == 1 && w[0] == 0.0f));
  if (max_nnz) CHECK((int)w.size() <= max_nnz);
  char name[32];
  snprintf(name, sizeof name, "dense%s", suffix); put(front, name, dense);
  snprintf(name, sizeof name, "w%s", suffix); put(front, name, w);
  snprintf(name, sizeof name, "meta%s", suffix); put(front, name, meta);
  return 0;
}

// [400][cos | sin][nbp]: the padded columns are exactly zero, column 0 is (1, 0)
static int twiddles(const char* front, int n_live, int nbp) {
  std::vector<float> tw;
  fe::twiddle_400(n_live, nbp, tw);
  CHECK(tw.size() == (size_t)400 * 2 * nbp);
  for (int k = 0; k < 400; ++k) {
    CHECK(tw[(size_t)k * 2 * nbp] == 1.0f && tw[((size_t)k * 2 + 1) * nbp] == 0.0f);
    for (int c = 0; c < 2; ++c)
      for (int j = n_live; j < nbp; ++j) CHECK(tw[((size_t)k * 2 + c) * nbp + j] == 0.0f);
  }
  put(front, "tw", tw);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 2 || !(g_out = fopen(argv[1], "wb"))) { fprintf(stderr, "usage: frontend_tables_check <output file>\n"); return 2; }
  std::vector<float> win, dense, dft;
  std::vector<int> meta;

  // ---- log-mel (logmel.hip): 16 kHz, 400-point, 201 bins padded to 224; window kind 0 = Whisper, 1 = S3 tokenizer
  fe::hann_symmetric(400, win);
  CHECK(win.size() == 400 && win[0] == 0.0f);
  for (int n = 0; n < 200; ++n) CHECK(fabsf(win[n] - win[399 - n]) < 1e-6f);            // symmetric: w[n] = w[N - 1 - n]
  put("logmel", "win0", win);
  fe::hann_periodic(400, win);
  CHECK(win.size() == 400 && fabsf(win[0]) < 1e-6f && win[399] > 1e-5f);                // periodic: the closing zero is sample 400
  for (int n = 1; n < 200; ++n) CHECK(fabsf(win[n] - win[400 - n]) < 1e-6f);            // ... and the symmetry is about sample 200
  put("logmel", "win1", win);
  if (twiddles("logmel", 201, 224)) return 1;
  fe::slaney_filters(80, 201, 16000.0f, 400, 8000.0f, dense);
  if (bank("logmel", "80", dense, 80, 201, kStagedNnz, meta)) return 1;
  fe::slaney_filters(128, 201, 16000.0f, 400, 8000.0f, dense);
  if (bank("logmel", "128", dense, 128, 201, kStagedNnz, meta)) return 1;

  // ---- S3Gen mel (mel_s3gen.hip): 24 kHz, 1920-point, 961 bins; the transform stops at the last bin the filters touch
  fe::slaney_filters(80, 961, 24000.0f, 1920, 8000.0f, dense);
  if (bank("s3gen", "", dense, 80, 961, 0, meta)) return 1;                              // read from global memory: no staging limit
  const int kmax = fe::last_live_bin(meta), nbp = (kmax + 1 + 31) / 32 * 32;
  CHECK(kmax == 640 && nbp == 672);                                                      // 8 kHz at 12.5 Hz per bin
  put("s3gen", "nbp", std::vector<int>{nbp});
  fe::hann_periodic(1920, win);
  fe::dft_rows(1920, kmax + 1, nbp, 1920, 1920, win.data(), dft);
  CHECK(dft.size() == (size_t)2 * nbp * 1920);
  for (int n = 0; n < 1920; ++n) CHECK(dft[n] == win[n] && dft[(size_t)nbp * 1920 + n] == 0.0f);      // bin 0: cos = 1, sin = 0
  for (int k = kmax + 1; k < nbp; ++k) CHECK(dft[(size_t)k * 1920 + 7] == 0.0f && dft[(size_t)(nbp + k) * 1920 + 7] == 0.0f);
  put("s3gen", "dft", dft);

  // ---- Fun-ASR (funasr_frontend.hip): Hamming, bins 0..199 padded to 224, HTK filters on the reference's 200-point grid
  funasr::hamming_window(win);
  put("funasr", "win", win);
  if (twiddles("funasr", funasr::NFREQ, 224)) return 1;
  funasr::mel_filters(dense);
  if (bank("funasr", "", dense, funasr::NMEL, funasr::NFREQ, kStagedNnz, meta)) return 1;

  // ---- CAM++ (campplus.hip): Povey window of 400, 512-point DFT over the 400 live samples (rows of 416), 257 bins padded to 288
  fe::povey_window(400, win);
  CHECK(win.size() == 400 && win[0] == 0.0f);
  for (int n = 0; n < 200; ++n) CHECK(fabsf(win[n] - win[399 - n]) < 1e-6f);
  put("cam", "win", win);
  fe::dft_rows(512, 257, 288, 400, 416, nullptr, dft);
  CHECK(dft.size() == (size_t)2 * 288 * 416);
  for (int k = 0; k < 2 * 288; ++k)
    for (int n = 400; n < 416; ++n) CHECK(dft[(size_t)k * 416 + n] == 0.0f);            // the row padding
  for (int n = 0; n < 400; ++n) CHECK(dft[n] == 1.0f && dft[(size_t)256 * 416 + n] == ((n & 1) ? -1.0f : 1.0f));      // bins 0 and 256
  put("cam", "dft", dft);
  fe::htk_bin_filters(80, 257, 16000.0f, 512, 20.0f, 8000.0f, dense);
  if (bank("cam", "", dense, 80, 257, 0, meta)) return 1;

  if (fclose(g_out) != 0) return 2;
  puts("ok");
  return 0;
}
