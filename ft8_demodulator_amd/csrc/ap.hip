// ap.hip -- the retry pass's list kernel (k_retry_list, shared with coherent.hip: ft8_internal.h,
// "retry pass"), and a-priori decoding: the kernels around k_bp that retry failed candidates with the
// bits of a hypothesis clamped to certainty (include/ft8hip.h, "a-priori decoding").
//
// One AP pass over records res[n_slots][N] and the LLRs plain BP consumed:
//   k_ap_amax   once: a = 1.01 max |L| of every candidate that is to be retried, 0 elsewhere
//   per hypothesis h, in order:
//     k_retry_list  the failed candidates with a != 0 (the list's gate), M = N -> list, count
//     k_ap_clamp    the listed candidates' LLRs with the hypothesis' bits set to +a / -a -> llr_h
//     k_bp          unchanged (launch_bp, mode 0: it skips list positions >= count) -> plain, res_h
//     k_ap_merge    the acceptance test; an accepted attempt rewrites its record in res
// A rescued record has ok = 1, so the next hypothesis' list leaves it out: the first accepted
// hypothesis wins.  No kernel here uses LDS; a wave handles one candidate (or one slot's list).
#include "ft8_internal.h"

namespace ft8 {
namespace {

constexpr int kApWaves = 4;  // candidates per 256-thread workgroup

// one wave per candidate: amax[item] = 1.01 max |L| (one multiply in double), or 0 where the candidate
// is not to be retried: past the slot's count, already ok, a NaN among its LLRs (NumPy's max then is
// NaN), or all LLRs zero
__global__ __launch_bounds__(kApWaves* kWave) void k_ap_amax(ApLaunch a) {
  const RetryLists& r = a.r;
  const int lane = threadIdx.x % kWave;
  const int64_t item = (int64_t)blockIdx.x * kApWaves + threadIdx.x / kWave;
  if (item >= (int64_t)r.n_slots * r.N) return;
  const int slot = (int)(item / r.N), cidx = (int)(item % r.N);
  if (cidx >= slot_count(r, slot) || r.res[item].ok) {
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

// one wave per slot: the first M candidates to retry, in candidate order (ballot / popcount scan as
// k_compact); a round that starts with the list full is not run
__global__ __launch_bounds__(kWave) void k_retry_list(RetryLists r) {
  const int slot = blockIdx.x, lane = threadIdx.x;
  const int nc = slot_count(r, slot);
  const int64_t s0 = (int64_t)slot * r.N, l0 = (int64_t)slot * r.M;
  int base = 0;
  for (int c0 = 0; c0 < nc && base < r.M; c0 += kWave) {
    const int c = c0 + lane;
    const bool take = c < nc && !r.res[s0 + c].ok && (!r.gate || r.gate[s0 + c] != 0.0);
    const unsigned long long m = __ballot(take);
    const int at = base + __popcll(m & ((1ull << lane) - 1ull));
    if (take && at < r.M) {
      const int64_t pos = l0 + at;
      r.list[pos] = c;
      r.cand[2 * pos] = r.cand_in ? r.cand_in[2 * (s0 + c)] : 0;
      r.cand[2 * pos + 1] = r.cand_in ? r.cand_in[2 * (s0 + c) + 1] : 0;
      r.score[pos] = r.score_in ? r.score_in[s0 + c] : 0.0;
    }
    base += __popcll(m);
  }
  if (lane == 0) r.count[slot] = min(base, r.M);
}

// bit i (< 80) of a 10-byte MSB-first field
__device__ __forceinline__ bool bit77(const uint8_t* b, int i) { return (b[i >> 3] >> (7 - (i & 7))) & 1; }

// one wave per list position: llr_h = the candidate's LLRs, masked bits at +a / -a
__global__ __launch_bounds__(kApWaves* kWave) void k_ap_clamp(ApLaunch a) {
  const RetryLists& r = a.r;
  const int lane = threadIdx.x % kWave;
  const int64_t pos = (int64_t)blockIdx.x * kApWaves + threadIdx.x / kWave;
  if (pos >= (int64_t)r.n_slots * r.N) return;
  const int slot = (int)(pos / r.N), j = (int)(pos % r.N);
  if (j >= r.count[slot]) return;
  const int64_t src = (int64_t)slot * r.N + r.list[pos];
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
  const RetryLists& r = a.r;
  const int lane = threadIdx.x % kWave;
  const int64_t pos = (int64_t)blockIdx.x * kApWaves + threadIdx.x / kWave;
  if (pos >= (int64_t)r.n_slots * r.N) return;
  const int slot = (int)(pos / r.N), j = (int)(pos % r.N);
  if (j >= r.count[slot]) return;
  const ft8_result& got = a.res_h[pos];
  if (!got.ok) return;  // 1. the tail says ok
  // 2. the decoded payload agrees with the hypothesis on every masked bit
  const bool differ = lane < 10 && ((got.payload[lane] ^ a.hyp.value[lane]) & a.hyp.mask[lane]) != 0;
  if (__ballot(differ) != 0) return;
  // 3. hard errors of the attempt's decisions against the signs of the unclamped LLRs
  const int64_t src = (int64_t)slot * r.N + r.list[pos];
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
    retry_accept(r.res + src, got, (a.h + 1) << 4);
    if (a.hard) a.hard[src] = (int16_t)hard;
  }
}

unsigned item_blocks(const ApLaunch& a) {
  return (unsigned)(((int64_t)a.r.n_slots * a.r.N + kApWaves - 1) / kApWaves);
}

}  // namespace

hipError_t launch_ap_amax(const ApLaunch& a, hipStream_t s) {
  if (a.r.n_slots <= 0 || a.r.N <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_ap_amax, dim3(item_blocks(a)), dim3(kApWaves * kWave), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_retry_list(const RetryLists& r, hipStream_t s) {
  if (r.n_slots <= 0 || r.M <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_retry_list, dim3(r.n_slots), dim3(kWave), 0, s, r);
  return hipGetLastError();
}

hipError_t launch_ap_clamp(const ApLaunch& a, hipStream_t s) {
  if (a.r.n_slots <= 0 || a.r.N <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_ap_clamp, dim3(item_blocks(a)), dim3(kApWaves * kWave), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_ap_merge(const ApLaunch& a, hipStream_t s) {
  if (a.r.n_slots <= 0 || a.r.N <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_ap_merge, dim3(item_blocks(a)), dim3(kApWaves * kWave), 0, s, a);
  return hipGetLastError();
}

}  // namespace ft8
