// ap.hip -- a-priori decoding: the kernels around k_bp that retry failed candidates with the bits of
// a hypothesis clamped to certainty (include/ft8hip.h, "a-priori decoding").
//
// One AP pass over records res[n_slots][N] and the LLRs plain BP consumed:
//   k_ap_amax   once: a = 1.01 max |L| of every candidate that is to be retried, 0 elsewhere
//   per hypothesis h, in order:
//     k_ap_list   per slot, the failed candidates (ok == 0, a != 0) in candidate order -> list, count
//     k_ap_clamp  the listed candidates' LLRs with the hypothesis' bits set to +a / -a -> llr_h
//     k_bp        unchanged (launch_bp, mode 0: it skips list positions >= count) -> plain, res_h
//     k_ap_merge  the acceptance test; an accepted attempt rewrites its record in res
// A rescued record has ok = 1, so the next hypothesis' k_ap_list leaves it out: the first accepted
// hypothesis wins.  No kernel here uses LDS; a wave handles one candidate (or one slot's list).
#include "ft8_internal.h"

namespace ft8 {
namespace {

constexpr int kApWaves = 4;  // candidates per 256-thread workgroup

__device__ __forceinline__ int slot_count(const ApLaunch& a, int slot) {
  return a.cand_count ? min(a.N, a.cand_count[slot]) : a.N;
}

// one wave per candidate: amax[item] = 1.01 max |L| (one multiply in double), or 0 where the candidate
// is not to be retried: past the slot's count, already ok, a NaN among its LLRs (NumPy's max then is
// NaN), or all LLRs zero
__global__ __launch_bounds__(kApWaves* kWave) void k_ap_amax(ApLaunch a) {
  const int lane = threadIdx.x % kWave;
  const int64_t item = (int64_t)blockIdx.x * kApWaves + threadIdx.x / kWave;
  if (item >= (int64_t)a.n_slots * a.N) return;
  const int slot = (int)(item / a.N), cidx = (int)(item % a.N);
  if (cidx >= slot_count(a, slot) || a.res[item].ok) {
    if (lane == 0) a.amax[item] = 0.0;
    return;
  }
  const double* L = a.llr + item * FT8_LDPC_N;
  double m = 0.0;
  bool nan = false;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int i = lane + kWave * j;
    if (i < FT8_LDPC_N) {
      const double v = L[i];
      nan |= v != v;
      m = fmax(m, fabs(v));
    }
  }
  for (int d = kWave / 2; d > 0; d >>= 1) m = fmax(m, __shfl_xor(m, d));
  const bool any_nan = __ballot(nan) != 0;
  if (lane == 0) a.amax[item] = any_nan ? 0.0 : 1.01 * m;
}

// one wave per slot: the candidates to retry, in candidate order (ballot / popcount scan as k_compact)
__global__ __launch_bounds__(kWave) void k_ap_list(ApLaunch a) {
  const int slot = blockIdx.x, lane = threadIdx.x;
  const int nc = slot_count(a, slot);
  const int64_t s0 = (int64_t)slot * a.N;
  int base = 0;
  for (int c0 = 0; c0 < nc; c0 += kWave) {
    const int c = c0 + lane;
    const bool take = c < nc && !a.res[s0 + c].ok && a.amax[s0 + c] != 0.0;
    const unsigned long long m = __ballot(take);
    if (take) {
      const int64_t pos = s0 + base + __popcll(m & ((1ull << lane) - 1ull));
      a.list[pos] = c;
      a.cand[2 * pos] = a.cand_in ? a.cand_in[2 * (s0 + c)] : 0;
      a.cand[2 * pos + 1] = a.cand_in ? a.cand_in[2 * (s0 + c) + 1] : 0;
      a.score[pos] = a.score_in ? a.score_in[s0 + c] : 0.0;
    }
    base += __popcll(m);
  }
  if (lane == 0) a.count[slot] = base;
}

// bit i (< 80) of a 10-byte MSB-first field
__device__ __forceinline__ bool bit77(const uint8_t* b, int i) { return (b[i >> 3] >> (7 - (i & 7))) & 1; }

// one wave per list position: llr_h = the candidate's LLRs, masked bits at +a / -a
__global__ __launch_bounds__(kApWaves* kWave) void k_ap_clamp(ApLaunch a) {
  const int lane = threadIdx.x % kWave;
  const int64_t pos = (int64_t)blockIdx.x * kApWaves + threadIdx.x / kWave;
  if (pos >= (int64_t)a.n_slots * a.N) return;
  const int slot = (int)(pos / a.N), j = (int)(pos % a.N);
  if (j >= a.count[slot]) return;
  const int64_t src = (int64_t)slot * a.N + a.list[pos];
  const double amp = a.amax[src];
  const double* L = a.llr + src * FT8_LDPC_N;
  double* out = a.llr_h + pos * FT8_LDPC_N;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int i = lane + kWave * k;
    if (i < FT8_LDPC_N) {
      double v = L[i];
      if (i < 77 && bit77(a.hyp.mask, i)) v = bit77(a.hyp.value, i) ? amp : -amp;
      out[i] = v;
    }
  }
}

// one wave per list position: the acceptance test of the attempt k_bp just made
__global__ __launch_bounds__(kApWaves* kWave) void k_ap_merge(ApLaunch a) {
  const int lane = threadIdx.x % kWave;
  const int64_t pos = (int64_t)blockIdx.x * kApWaves + threadIdx.x / kWave;
  if (pos >= (int64_t)a.n_slots * a.N) return;
  const int slot = (int)(pos / a.N), j = (int)(pos % a.N);
  if (j >= a.count[slot]) return;
  const ft8_result& r = a.res_h[pos];
  if (!r.ok) return;  // 1. the tail says ok
  // 2. the decoded payload agrees with the hypothesis on every masked bit
  const bool differ = lane < 10 && ((r.payload[lane] ^ a.hyp.value[lane]) & a.hyp.mask[lane]) != 0;
  if (__ballot(differ) != 0) return;
  // 3. hard errors of the attempt's decisions against the signs of the unclamped LLRs
  const int64_t src = (int64_t)slot * a.N + a.list[pos];
  const double* L = a.llr + src * FT8_LDPC_N;
  const uint8_t* plain = a.plain + pos * FT8_LDPC_N;
  int hard = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int i = lane + kWave * k;
    const bool err = i < FT8_LDPC_N && (plain[i] != 0) != (L[i] > 0.0);
    hard += __popcll(__ballot(err));
  }
  if (hard > a.max_hard) return;
  if (lane == 0) {
    ft8_result w = a.res[src];
    w.ok = 1;
    for (int i = 0; i < 10; ++i) w.payload[i] = r.payload[i];
    w.crc_extracted = r.crc_extracted;
    w.crc_calculated = r.crc_calculated;
    w.ldpc_errors = r.ldpc_errors;
    w.pass_index = (uint8_t)(w.pass_index | ((a.h + 1) << 4));
    a.res[src] = w;
    if (a.hard) a.hard[src] = (int16_t)hard;
  }
}

unsigned item_blocks(const ApLaunch& a) {
  return (unsigned)(((int64_t)a.n_slots * a.N + kApWaves - 1) / kApWaves);
}

}  // namespace

hipError_t launch_ap_amax(const ApLaunch& a, hipStream_t s) {
  if (a.n_slots <= 0 || a.N <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_ap_amax, dim3(item_blocks(a)), dim3(kApWaves * kWave), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_ap_prepare(const ApLaunch& a, hipStream_t s) {
  if (a.n_slots <= 0 || a.N <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_ap_list, dim3(a.n_slots), dim3(kWave), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_ap_clamp, dim3(item_blocks(a)), dim3(kApWaves * kWave), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_ap_merge(const ApLaunch& a, hipStream_t s) {
  if (a.n_slots <= 0 || a.N <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_ap_merge, dim3(item_blocks(a)), dim3(kApWaves * kWave), 0, s, a);
  return hipGetLastError();
}

}  // namespace ft8
