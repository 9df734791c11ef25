// score_shared.h -- wave helpers the tiled score kernels of both protocols share (sync.hip k_score2,
// ft4.hip k_score4): the packed pair type, the wave maximum and the LDS pair load.
#pragma once
#include "ft8_internal.h"

namespace ft8 {
namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));

// maximum over the wave (no NaN), on order-preserving integer keys (a float max would re-quiet
// every DPP operand): rotations inside each 16-lane row (DPP row_ror 8, 4, 2, 1), then the four
// row maxima in scalar registers -- instead of six ds_bpermute rounds
__device__ __forceinline__ int fkey(float v) {
  const int i = __float_as_int(v);
  return i ^ ((i >> 31) & 0x7fffffff);
}
template <int CTRL>
__device__ __forceinline__ int dpp_max(int k) {
  return max(k, __builtin_amdgcn_mov_dpp(k, CTRL, 0xf, 0xf, false));
}
__device__ __forceinline__ float wave_max(float v) {
  int k = fkey(v);
  k = dpp_max<0x128>(k);  // row_ror:8
  k = dpp_max<0x124>(k);  // row_ror:4
  k = dpp_max<0x122>(k);  // row_ror:2
  k = dpp_max<0x121>(k);  // row_ror:1
  const int m = max(max(__builtin_amdgcn_readlane(k, 0), __builtin_amdgcn_readlane(k, 16)),
                    max(__builtin_amdgcn_readlane(k, 32), __builtin_amdgcn_readlane(k, 48)));
  return __int_as_float(m ^ ((m >> 31) & 0x7fffffff));
}

// volatile LDS load: one ds_read_b64 per pair.  The compiler would otherwise merge neighbouring
// pairs into ds_read2_b64, which moves half as many bytes per LDS cycle (measured: k_score2 0.27
// vs 0.30 ms per 256-slot step).
template <int BPT>
__device__ __forceinline__ f32x2 ld2(const float* p) {
  if constexpr (BPT % 2 == 0) return *(const volatile __attribute__((address_space(3))) f32x2*)p;
  else return f32x2{p[0], p[1]};
}

}  // namespace
}  // namespace ft8
