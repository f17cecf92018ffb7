// quant_repack.h -- host repack of MLX-affine 4- / 8-bit Linears (group 64) into the fragment-ordered arrays the packed skinny GEMMs
// read (layout and arithmetic: skinny_quant.hip).  Shared by the LM loader (lm_load.hip) and the Whisper loader (whisper_load.hip).
#pragma once
#include <stdint.h>

#include <utility>
#include <vector>

// one Linear as stored: packed codes [N][K * bits / 32], scales / biases [N][K / 64] (16-bit: f16 | bf16, or f32; see q_repack_host's sdt)
struct Q4Src { const uint32_t* w; const void* s; const void* b; };

// rows[i] = (tensor index, row): the fused matrix's row i.  bits 4 | 8; sdt = MIA_F16 | MIA_BF16 | MIA_F32 (type of scales and biases);
// mag = the 16-bit float the codes are OR-ed into (128 for bf16, 1024 for f16 compute).  K must be a multiple of 128.
//   wf [ceil(N / 16)][K / 128][bits / 4][64][4] words, st [ceil(N / 16)][K / 128][16][4] floats
void q_repack_host(const std::vector<Q4Src>& src, const std::vector<std::pair<int, int>>& rows, int K, int bits, int sdt, float mag,
                   std::vector<uint32_t>& wf, std::vector<float>& st);
