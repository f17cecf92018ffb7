// funasr_host_check.cpp -- stand-alone exerciser of the host-only code of Fun-ASR's audio half (csrc/funasr_host.h): the window and
// filterbank builders, the compact filter form, the length rules and the SenseVoice shape rules.  Meant for the host sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include tools/funasr_host_check.cpp -o funasr_host_check
// Prints the table facts tests/golden/funasr_fbank.npz freezes (first / last non-zero bin per filter) and exits non-zero on a broken rule.
#include <cstdio>
#include <cstdlib>

#include "../mlx-swift-audio_amd/csrc/funasr_host.h"

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } \
  } while (0)

int main() {
  using namespace funasr;
  std::vector<float> win, dense, w;
  std::vector<int> meta;
  hamming_window(win);
  CHECK(win.size() == (size_t)NFFT);
  CHECK(fabsf(win[0] - 0.08f) < 1e-6f && fabsf(win[NFFT - 1] - 0.08f) < 1e-6f);          // symmetric: both ends 0.54 - 0.46
  for (int n = 0; n < NFFT / 2; ++n) CHECK(fabsf(win[n] - win[NFFT - 1 - n]) < 1e-6f);
  mel_filters(dense);
  CHECK(dense.size() == (size_t)NMEL * NFREQ);
  fe::compact_filters(dense, NMEL, NFREQ, w, meta);
  CHECK(meta.size() == (size_t)NMEL * 3 && w.size() <= 1024);
  size_t nnz = 0;
  printf("first:");
  for (int m = 0; m < NMEL; ++m) {
    const int lo = meta[m * 3], cnt = meta[m * 3 + 1], off = meta[m * 3 + 2];
    CHECK(lo >= 0 && cnt >= 1 && lo + cnt <= NFREQ && off >= 0 && (size_t)(off + cnt) <= w.size());
    for (int c = 0; c < cnt; ++c) CHECK(w[off + c] == dense[(size_t)m * NFREQ + lo + c] && w[off + c] >= 0.f);
    for (int k = 0; k < NFREQ; ++k) if (k < lo || k >= lo + cnt) CHECK(dense[(size_t)m * NFREQ + k] == 0.f);
    nnz += (size_t)cnt;
    printf(" %d", lo);
  }
  printf("\nlast:");
  for (int m = 0; m < NMEL; ++m) printf(" %d", meta[m * 3] + meta[m * 3 + 1] - 1);
  printf("\nnnz: %zu\n", nnz);
  CHECK(nnz == w.size());

  const int64_t L[5] = {160, 959, 960, 16000, 16001}, F[5] = {2, 6, 7, 101, 101}, R[5] = {1, 1, 2, 17, 17};
  for (int i = 0; i < 5; ++i) CHECK(n_frames(L[i]) == F[i] && t_lfr(L[i]) == R[i]);
  CHECK(fsmn_left(11, 0) == 5 && fsmn_left(11, 2) == 7 && fsmn_left(1, 0) == 0);

  mia_sensevoice_config c = {560, 512, 4, 2048, 11, 0, 1, 49, 20, 2, 1024, 2048, 2, 8};
  CHECK(config_check(c) == nullptr);
  mia_sensevoice_config micro = {560, 256, 2, 512, 11, 2, 1, 2, 2, 2, 256, 512, 1, 2};
  CHECK(config_check(micro) == nullptr);
  { auto b = c; b.sanm_shift = 6; CHECK(config_check(b) != nullptr); }        // right context -1
  { auto b = c; b.sanm_shift = 5; CHECK(config_check(b) == nullptr); }        // right context 0
  { auto b = c; b.encoder_dim = 384; CHECK(config_check(b) != nullptr); }     // head dim 96
  { auto b = c; b.llm_dim = 896; b.adaptor_heads = 7; CHECK(config_check(b) != nullptr); }
  { auto b = c; b.ffn_dim = 2000; CHECK(config_check(b) != nullptr); }
  { auto b = c; b.adaptor_k = 0; CHECK(config_check(b) != nullptr); }
  { auto b = c; b.n_encoders0 = 2; CHECK(config_check(b) != nullptr); }
  { auto b = c; b.input_dim = 562; CHECK(config_check(b) != nullptr); }
  puts("ok");
  return 0;
}
