// quant_repack.h -- host repack of MLX-affine 4- / 8-bit Linears (group 64) into the fragment-ordered arrays the packed skinny GEMMs
// read (layout and arithmetic: skinny_quant.hip), and the lookup / upload both attach calls are made of (lm_load.hip, whisper_load.hip).
#pragma once
#include <stdint.h>

#include <string>
#include <utility>
#include <vector>

#include "tensor_loader.h"

// one Linear as stored: packed codes [N][K * bits / 32], scales / biases [N][K / 64] (16-bit: f16 | bf16, or f32; see q_repack_host's sdt)
struct Q4Src { const uint32_t* w; const void* s; const void* b; };

// rows[i] = (tensor index, row): the fused matrix's row i.  bits 4 | 8; sdt = MIA_F16 | MIA_BF16 | MIA_F32 (type of scales and biases);
// mag = the 16-bit float the codes are OR-ed into (128 for bf16, 1024 for f16 compute).  K must be a multiple of 128.
//   wf [ceil(N / 16)][K / 128][bits / 4][64][4] words, st [ceil(N / 16)][K / 128][16][4] floats
void q_repack_host(const std::vector<Q4Src>& src, const std::vector<std::pair<int, int>>& rows, int K, int bits, int sdt, float mag,
                   std::vector<uint32_t>& wf, std::vector<float>& st);

// The `<p>.weight / .scales / .biases` triple of one packed Linear [N][K] in L's tensors, validated (codes MIA_U32, the shapes above, scales
// and biases of one 16-bit type, or f32 where the model takes it: f32_scales).  *sdt: the scale type of the attach, -1 before the
// first Linear; a Linear of another type is an error.  Errors go to L (MIA_ERR_INVALID_ARGUMENT).
bool q_find_linear(TensorLoader& L, const std::string& p, int N, int K, int bits, bool f32_scales, int* sdt, Q4Src& q);
// q_repack_host, then both arrays uploaded through L (into L.allocs: the attach's own list, which joins the handle's only when every
// matrix is in place).  A refused allocation is MIA_ERR_OUT_OF_MEMORY, a failed copy MIA_ERR_DEVICE.
bool q_upload(TensorLoader& L, const std::vector<Q4Src>& src, const std::vector<std::pair<int, int>>& rows, int K, int bits, int sdt, float mag,
              uint32_t** wfrag, float** stfrag);
