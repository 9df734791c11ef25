// llr_shared.h -- what the LLR kernels of both protocols share (bp.hip k_llr, ft4.hip k_llr4): Python's
// max(), the correctly rounded square root and NumPy's pairwise sum of ftx_normalize_logl
// (ft8_decode.py:190-198), for the four candidates of a wave side by side.
#pragma once
#include "ft8_internal.h"

namespace ft8 {
namespace {

// correctly rounded sqrt (math.sqrt): hardware estimate + Tuckerman's test with exact fma residuals
__device__ double sqrt_rn(double x) {
  double y = __builtin_sqrt(x);
  if (!(x > 0.0) || __builtin_isinf(x)) return y;
  for (int it = 0; it < 4; ++it) {
    const double lo = __longlong_as_double(__double_as_longlong(y) - 1);
    const double hi = __longlong_as_double(__double_as_longlong(y) + 1);
    if (__builtin_fma(y, lo, -x) >= 0.0) { y = lo; continue; }   // y*y^- >= x: too large
    if (__builtin_fma(y, hi, -x) < 0.0) { y = hi; continue; }    // y*y^+ <  x: too small
    break;
  }
  return y;
}

__device__ __forceinline__ double pymax4(double a, double b, double c, double d) {
  double m = a;          // builtin max(): first maximum under '>'
  m = b > m ? b : m;
  m = c > m ? c : m;
  m = d > m ? d : m;
  return m;
}
__device__ __forceinline__ double pymax2(double a, double b) { return b > a ? b : a; }

constexpr int kLlrCpw = 4;                  // k_llr / k_llr4: candidates per wave
constexpr int kLlrRow = FT8_LDPC_N + 2;     // LDS row of one candidate's 174 doubles (padded)

// numpy pairwise sum (loops_utils.h.src) of x[u][0..174) for the wave's kLlrCpw candidates at once:
// pw(0,80) + pw(80,94).  Lanes 16 u + l hold candidate u's 16 partial sums (l < 8: the 8
// accumulators of [0, 80), l >= 8: those of [80, 168)), lane 16 u combines them with the tail
// [168, 174) in numpy's order; every lane receives its candidate's sum.  (One candidate per wave,
// as in round 4, kept 48 of the 64 lanes idle through both sums of the normalisation.)
__device__ double pairwise174x4(const double (*x)[kLlrRow], double (*part)[16], int lane) {
  const int u = lane >> 4, l = lane & 15;
  const double* xu = x[u];
  double r;
  if (l < 8) {
    r = xu[l];
    for (int i = 8; i < 80; i += 8) r += xu[i + l];
  } else {
    const int j = l - 8;
    r = xu[80 + j];
    for (int i = 8; i < 88; i += 8) r += xu[80 + i + j];
  }
  part[u][l] = r;
  __syncthreads();
  double tot = 0.0;
  if (l == 0) {
    const double* pu = part[u];
    const double s1 = ((pu[0] + pu[1]) + (pu[2] + pu[3])) + ((pu[4] + pu[5]) + (pu[6] + pu[7]));
    double s2 = ((pu[8] + pu[9]) + (pu[10] + pu[11])) + ((pu[12] + pu[13]) + (pu[14] + pu[15]));
    for (int i = 168; i < 174; ++i) s2 += xu[i];
    tot = 0.0 + (s1 + s2);  // add.reduce starts from the identity
  }
  __syncthreads();
  return __shfl(tot, lane & ~15);
}

}  // namespace
}  // namespace ft8
