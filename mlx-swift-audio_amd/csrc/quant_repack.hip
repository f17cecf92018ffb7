// quant_repack.hip -- host repack of packed MLX-affine Linears into fragment order, their lookup and upload (quant_repack.h); no device code.
#include "quant_repack.h"

#include <string.h>

#include <algorithm>

#include "../../include/mia.h"

namespace {

float q_to_f32(const void* p, size_t i, int sdt) {
  if (sdt == MIA_F32) return ((const float*)p)[i];
  const uint16_t v = ((const uint16_t*)p)[i];
  return sdt == MIA_F16 ? f16_to_f32(v) : bf16_to_f32(v);
}

}  // namespace

void q_repack_host(const std::vector<Q4Src>& src, const std::vector<std::pair<int, int>>& rows, int K, int bits, int sdt, float mag,
                   std::vector<uint32_t>& wf, std::vector<float>& st) {
  // bits 6: a full low-nibble plane and a 2-bit high plane of half its size (skinny_quant.hip): 384 words per (tile, block)
  const int N = (int)rows.size(), tiles = (N + 15) / 16, nblk = K / 128, np = bits == 4 ? 1 : 2, wpr = K * bits / 32, gpr = K / 64;
  const size_t blk_words = bits == 6 ? 384 : (size_t)np * 256;
  wf.assign((size_t)tiles * nblk * blk_words, 0u);
  st.assign((size_t)tiles * nblk * 16 * 4, 0.f);
  const float tmul = mag * (np == 2 ? 17.0f : 1.0f);
  for (int t = 0; t < tiles; ++t)
    for (int r = 0; r < 16; ++r) {
      const int n = std::min(t * 16 + r, N - 1);                      // the last tile repeats its final row (never stored)
      const Q4Src& q = src[rows[n].first];
      const uint32_t* wrow = q.w + (size_t)rows[n].second * wpr;
      const size_t g0 = (size_t)rows[n].second * gpr;
      // MLX packing: the row is one little-endian bit stream, code k at bits [k bits, (k + 1) bits) -- a 6-bit code may straddle two words
      auto code = [&](int k) -> uint32_t {
        const int bit = k * bits, w = bit >> 5, sh = bit & 31;
        uint32_t v = wrow[w] >> sh;
        if (sh + bits > 32) v |= wrow[w + 1] << (32 - sh);
        return v & ((1u << bits) - 1u);
      };
      for (int b = 0; b < nblk; ++b) {
        uint32_t* blk = &wf[((size_t)t * nblk + b) * blk_words];
        for (int c = 0; c < 4; ++c)
          for (int stp = 0; stp < 4; ++stp) {
            const int k0 = b * 128 + 32 * stp + 8 * c;
            for (int p = 0; p < (bits == 6 ? 1 : np); ++p) {
              uint32_t word = 0;
              for (int i = 0; i < 4; ++i) {
                const uint32_t q0 = (code(k0 + 2 * i) >> (4 * p)) & 15u, q1 = (code(k0 + 2 * i + 1) >> (4 * p)) & 15u;
                word |= (q0 << (4 * i)) | (q1 << (16 + 4 * i));
              }
              blk[((size_t)p * 64 + 16 * c + r) * 4 + stp] = word;
            }
            if (bits == 6) {               // high plane: word stp / 2 of the lane, the K-step's four pairs at pair slots 4 (stp & 1) ..
              uint32_t half = 0;
              for (int i = 0; i < 4; ++i) {
                const uint32_t q0 = code(k0 + 2 * i) >> 4, q1 = code(k0 + 2 * i + 1) >> 4;
                half |= (q0 << (2 * i)) | (q1 << (16 + 2 * i));
              }
              blk[256 + (size_t)(16 * c + r) * 2 + (stp >> 1)] |= half << (8 * (stp & 1));
            }
          }
        for (int g = 0; g < 2; ++g) {
          const float sc = q_to_f32(q.s, g0 + 2 * b + g, sdt), bi = q_to_f32(q.b, g0 + 2 * b + g, sdt);
          float* d = &st[(((size_t)t * nblk + b) * 16 + r) * 4 + 2 * g];
          d[0] = sc;
          d[1] = (float)((double)bi - (double)tmul * (double)sc);
        }
      }
    }
}

bool q_find_linear(TensorLoader& L, const std::string& p, int N, int K, int bits, bool f32_scales, int* sdt, Q4Src& q) {
  const mia_tensor_view* t[3];
  const char* suffix[3] = {".weight", ".scales", ".biases"};
  for (int i = 0; i < 3; ++i)
    if (!(t[i] = L.find(p + suffix[i]))) return L.fail(MIA_ERR_INVALID_ARGUMENT, "missing tensor '" + p + suffix[i] + "'");
  const mia_tensor_view *w = t[0], *s = t[1], *b = t[2];
  const bool ok = w->dtype == MIA_U32 && w->ndim == 2 && w->shape[0] == N && w->shape[1] == (int64_t)K * bits / 32 && s->ndim == 2 && s->shape[0] == N &&
                  s->shape[1] == K / 64 && b->ndim == 2 && b->shape[0] == N && b->shape[1] == K / 64 && s->dtype == b->dtype &&
                  (s->dtype == MIA_F16 || s->dtype == MIA_BF16 || (f32_scales && s->dtype == MIA_F32));
  if (!ok)
    return L.fail(MIA_ERR_INVALID_ARGUMENT, "'" + p + "' is not a " + std::to_string(bits) + "-bit group-64 Linear of the expected shape (scales / biases" +
                                                (f32_scales ? ": f16, bf16 or f32)" : " must be f16 or bf16)"));
  if (*sdt < 0) *sdt = s->dtype;
  if (*sdt != s->dtype) return L.fail(MIA_ERR_INVALID_ARGUMENT, "mixed scale dtypes");
  q = Q4Src{(const uint32_t*)w->data, s->data, b->data};
  return true;
}

bool q_upload(TensorLoader& L, const std::vector<Q4Src>& src, const std::vector<std::pair<int, int>>& rows, int K, int bits, int sdt, float mag,
              uint32_t** wfrag, float** stfrag) {
  std::vector<uint32_t> wf;
  std::vector<float> st;
  q_repack_host(src, rows, K, bits, sdt, mag, wf, st);
  *wfrag = (uint32_t*)L.alloc(wf.size() * 4);
  *stfrag = L.up(st);
  if (!*wfrag || !*stfrag) return false;
  if (hipMemcpy(*wfrag, wf.data(), wf.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return L.fail(MIA_ERR_DEVICE, "upload of the packed weights failed");
  return L.err.empty();
}

// Test hook (include/mia.h): the repack alone, host memory in and out -- needs no device.
extern "C" int mia_quant_repack(const uint32_t* codes, const void* scales, const void* biases, int N, int K, int bits, int scale_dtype,
                                int compute_dtype, uint32_t* wfrag, float* stfrag) {
  if (!codes || !scales || !biases || !wfrag || !stfrag || N <= 0 || K <= 0 || K % 128 != 0 || (bits != 4 && bits != 6 && bits != 8)) return MIA_ERR_INVALID_ARGUMENT;
  if (scale_dtype != MIA_F16 && scale_dtype != MIA_BF16 && scale_dtype != MIA_F32) return MIA_ERR_INVALID_ARGUMENT;
  if (compute_dtype != MIA_F16 && compute_dtype != MIA_BF16) return MIA_ERR_INVALID_ARGUMENT;
  std::vector<Q4Src> src{Q4Src{codes, scales, biases}};
  std::vector<std::pair<int, int>> rows;
  for (int i = 0; i < N; ++i) rows.push_back({0, i});
  std::vector<uint32_t> wf;
  std::vector<float> st;
  q_repack_host(src, rows, K, bits, scale_dtype, compute_dtype == MIA_F16 ? 1024.0f : 128.0f, wf, st);
  memcpy(wfrag, wf.data(), wf.size() * 4);
  memcpy(stfrag, st.data(), st.size() * 4);
  return MIA_OK;
}
