/* mia_gemm_quant.h -- the descriptor of mia_op_gemm_quant (include/mia.h, "operator level"): the many-row GEMM on packed 4- / 6- / 8-bit
 * weights, C fp32 [M][ldc] = A [M][lda] . Wq^T (+ R [M][ldr]).  Field order follows mia_skinny_desc.  DEVICE pointers.
 * mia.h declares the type; a caller that fills one includes this file as well.  The ctypes mirror is _abi.GemmQuantDesc
 * (tests/test_gemm_quant_abi.py compares the two field for field). */
#ifndef MIA_GEMM_QUANT_H
#define MIA_GEMM_QUANT_H
#include "mia.h"

struct mia_gemm_quant_desc {
  const void* A; int64_t lda;
  const uint32_t* wfrag; const float* stfrag; int32_t bits;
  float* C; int64_t ldc;
  const float* R; int64_t ldr;
  int32_t M, N, K, dtype;
};

#endif
