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

// bit i (< 80) of a 10-byte MSB-first field
__device__ __forceinline__ bool bit77(const uint8_t* b, int i) { return (b[i >> 3] >> (7 - (i & 7))) & 1; }

// The three blocks the AP kernels and the coherent-AP kernels share; a wave works on one LLR vector L[174].
// a = 1.01 max |L| (one multiply in double after the reduction), 0 where any of L is NaN (NumPy's max
// then is NaN); the same value in every lane
__device__ __forceinline__ double wave_amax(const double* L, int lane) {
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
  return any_nan ? 0.0 : 1.01 * m;
}
// out = L with the hypothesis' masked bits at +amp / -amp
__device__ __forceinline__ void wave_clamp(const double* L, const ft8_ap_hyp& hyp, double amp, double* out, int lane) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int i = lane + kWave * k;
    if (i < FT8_LDPC_N) {
      double v = L[i];
      if (i < 77 && bit77(hyp.mask, i)) v = bit77(hyp.value, i) ? amp : -amp;
      out[i] = v;
    }
  }
}
// acceptance tests 2 and 3 of an attempt that decoded to `got` with the hard decisions `plain`: -1 where
// the payload differs from the hypothesis on a masked bit, else the hard errors of the decisions against
// the signs of the unclamped L (three ballots); the same value in every lane
__device__ __forceinline__ int wave_hard_errors(const ft8_result& got, const ft8_ap_hyp& hyp, const double* L,
                                                const uint8_t* plain, int lane) {
  const bool differ = lane < 10 && ((got.payload[lane] ^ hyp.value[lane]) & hyp.mask[lane]) != 0;
  if (__ballot(differ) != 0) return -1;
  int hard = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int i = lane + kWave * k;
    const bool err = i < FT8_LDPC_N && (plain[i] != 0) != (L[i] > 0.0);
    hard += __popcll(__ballot(err));
  }
  return hard;
}

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
  const double amp = wave_amax(L, lane);
  if (lane == 0) a.amax[item] = amp;
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
  wave_clamp(L, a.hyp, amp, out, lane);
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
  // 2. the decoded payload agrees with the hypothesis on every masked bit; 3. hard errors of the attempt's
  // decisions against the signs of the unclamped LLRs
  const int64_t src = (int64_t)slot * r.N + r.list[pos];
  const int hard = wave_hard_errors(got, a.hyp, a.llr + src * FT8_LDPC_N, a.plain + pos * FT8_LDPC_N, lane);
  if (hard < 0 || hard > a.max_hard) return;
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

// k_ap_clamp and k_ap_merge walk the lists with the records' stride: M = N (ApLaunch, ft8_internal.h)
hipError_t launch_ap_clamp(const ApLaunch& a, hipStream_t s) {
  if (a.r.M != a.r.N) return hipErrorInvalidValue;
  if (a.r.n_slots <= 0 || a.r.N <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_ap_clamp, dim3(item_blocks(a)), dim3(kApWaves * kWave), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_ap_merge(const ApLaunch& a, hipStream_t s) {
  if (a.r.M != a.r.N) return hipErrorInvalidValue;
  if (a.r.n_slots <= 0 || a.r.N <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_ap_merge, dim3(item_blocks(a)), dim3(kApWaves * kWave), 0, s, a);
  return hipGetLastError();
}

// ---- a-priori retries on the coherent LLRs (ft8_internal.h, CohApLaunch) ----------------------------
//   k_cohap_amax   one wave per (position, set): a_n, 0 where the position or the set is not tried
//   k_cohap_list   one wave per slot: the attempts (j, h, n) with a_n != 0, hypothesis outer and set inner
//                  within a position, compacted -> att (k_bp's candidate lists) and where
//   k_cohap_clamp  one wave per listed attempt: set n's LLRs with hypothesis h's bits at +a_n / -a_n
//   k_bp           unchanged, once over all attempts -> plain, res_a
//   k_cohap_merge  one wave per position: the first attempt in order that passes the acceptance test
//                  rewrites the record
namespace {

__device__ __forceinline__ int cohap_count(const CohApLaunch& a, int slot) {
  return a.count ? min(a.M, max(a.count[slot], 0)) : a.M;
}
// attempts per slot (the stride of the attempt lists) and per position
__device__ __forceinline__ int64_t cohap_stride(const CohApLaunch& a) { return (int64_t)a.M * a.H * a.S; }
// the record of list position pos = slot * M + j, null where the list names none
__device__ __forceinline__ ft8_result* cohap_record(const CohApLaunch& a, int slot, int j) {
  const int orig = a.list ? a.list[(int64_t)slot * a.M + j] : j;
  return orig >= 0 && orig < a.N ? a.res + (int64_t)slot * a.N + orig : nullptr;
}

__global__ __launch_bounds__(kApWaves* kWave) void k_cohap_amax(CohApLaunch a) {
  const int lane = threadIdx.x % kWave;
  const int64_t item = (int64_t)blockIdx.x * kApWaves + threadIdx.x / kWave;
  if (item >= (int64_t)a.n_slots * a.M * a.S) return;
  const int64_t pos = item / a.S;
  const int n = (int)(item % a.S), slot = (int)(pos / a.M), j = (int)(pos % a.M);
  bool tried = j < cohap_count(a, slot) && (!a.fit || a.fit[pos].status == 0) && (!a.valid || ((a.valid[pos] >> n) & 1));
  if (tried) {
    const ft8_result* rec = cohap_record(a, slot, j);
    tried = rec && !rec->ok;
  }
  if (!tried) {
    if (lane == 0) a.amax[item] = 0.0;
    return;
  }
  const double* L = a.llr + pos * a.pos_stride + n * a.set_stride;
  const double amp = wave_amax(L, lane);
  if (lane == 0) a.amax[item] = amp;
}

__global__ __launch_bounds__(kWave) void k_cohap_list(CohApLaunch a) {
  const int slot = blockIdx.x, lane = threadIdx.x;
  const int per = a.H * a.S;
  const int64_t A = cohap_stride(a), l0 = (int64_t)slot * A;
  const int64_t total = (int64_t)cohap_count(a, slot) * per;   // <= A
  int64_t base = 0;
  for (int64_t c0 = 0; c0 < total; c0 += kWave) {
    const int64_t idx = c0 + lane;
    const int j = (int)(idx / per), n = (int)(idx % a.S);
    const int64_t pos = (int64_t)slot * a.M + j;
    const bool take = idx < total && a.amax[pos * a.S + n] != 0.0;
    const unsigned long long m = __ballot(take);
    const int64_t at = base + __popcll(m & ((1ull << lane) - 1ull));
    if (idx < total) a.where[l0 + idx] = take ? (int32_t)at : -1;
    if (take) {   // at < total <= A
      a.att.list[l0 + at] = (int32_t)idx;
      a.att.cand[2 * (l0 + at)] = a.cand ? a.cand[2 * pos] : 0;
      a.att.cand[2 * (l0 + at) + 1] = a.cand ? a.cand[2 * pos + 1] : 0;
      a.att.score[l0 + at] = a.score ? a.score[pos] : 0.0;
    }
    base += __popcll(m);
  }
  if (lane == 0) a.att.count[slot] = (int32_t)base;
}

__global__ __launch_bounds__(kApWaves* kWave) void k_cohap_clamp(CohApLaunch a) {
  const int lane = threadIdx.x % kWave;
  const int64_t A = cohap_stride(a);
  const int64_t ap = (int64_t)blockIdx.x * kApWaves + threadIdx.x / kWave;
  if (ap >= (int64_t)a.n_slots * A) return;
  const int slot = (int)(ap / A);
  if (ap % A >= a.att.count[slot]) return;
  const int64_t idx = a.att.list[ap];
  if (idx < 0 || idx >= A) return;
  const int n = (int)(idx % a.S), h = (int)(idx / a.S % a.H), j = (int)(idx / ((int64_t)a.H * a.S));
  const int64_t pos = (int64_t)slot * a.M + j;
  const double amp = a.amax[pos * a.S + n];
  const double* L = a.llr + pos * a.pos_stride + n * a.set_stride;
  double* out = a.llr_a + ap * FT8_LDPC_N;
  wave_clamp(L, a.hyp[h], amp, out, lane);
}

__global__ __launch_bounds__(kApWaves* kWave) void k_cohap_merge(CohApLaunch a) {
  const int lane = threadIdx.x % kWave;
  const int64_t pos = (int64_t)blockIdx.x * kApWaves + threadIdx.x / kWave;
  if (pos >= (int64_t)a.n_slots * a.M) return;
  const int slot = (int)(pos / a.M), j = (int)(pos % a.M);
  if (j >= cohap_count(a, slot)) return;
  ft8_result* rec = cohap_record(a, slot, j);
  if (!rec || rec->ok) return;
  const int64_t A = cohap_stride(a), l0 = (int64_t)slot * A;
  for (int h = 0; h < a.H; ++h) {
    for (int n = 0; n < a.S; ++n) {
      const int32_t w = a.where[l0 + ((int64_t)j * a.H + h) * a.S + n];
      if (w < 0 || w >= a.att.count[slot]) continue;   // not listed: the (position, set) is not tried
      const ft8_result& got = a.res_a[l0 + w];
      if (!got.ok) continue;  // 1. the tail says ok
      // 2. the decoded payload agrees with the hypothesis on every masked bit; 3. hard errors of the attempt's
      // decisions against the signs of set n's unclamped LLRs
      const int hard = wave_hard_errors(got, a.hyp[h], a.llr + pos * a.pos_stride + n * a.set_stride,
                                        a.plain + (l0 + w) * FT8_LDPC_N, lane);
      if (hard < 0 || hard > a.max_hard) continue;
      if (lane == 0) {
        const int bits = (a.drift && a.drift[pos].rate_hz_per_s != 0.f ? 6 : 2) | (n > 0 ? 8 : 0) | ((h + 1) << 4);
        retry_accept(rec, got, bits);
        if (a.hard) a.hard[rec - a.res] = (int16_t)hard;
      }
      return;
    }
  }
}

bool cohap_valid(const CohApLaunch& a) {
  return a.n_slots > 0 && a.M > 0 && a.H > 0 && a.H <= FT8_AP_MAX_HYP && a.S > 0 && a.S <= 3;
}
unsigned cohap_blocks(int64_t waves) { return (unsigned)((waves + kApWaves - 1) / kApWaves); }

}  // namespace

hipError_t launch_cohap_amax(const CohApLaunch& a, hipStream_t s) {
  if (!cohap_valid(a)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_cohap_amax, dim3(cohap_blocks((int64_t)a.n_slots * a.M * a.S)), dim3(kApWaves * kWave), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_cohap_list(const CohApLaunch& a, hipStream_t s) {
  if (!cohap_valid(a)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_cohap_list, dim3(a.n_slots), dim3(kWave), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_cohap_clamp(const CohApLaunch& a, hipStream_t s) {
  if (!cohap_valid(a)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_cohap_clamp, dim3(cohap_blocks((int64_t)a.n_slots * a.M * a.H * a.S)), dim3(kApWaves * kWave), 0,
                     s, a);
  return hipGetLastError();
}

hipError_t launch_cohap_merge(const CohApLaunch& a, hipStream_t s) {
  if (!cohap_valid(a)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_cohap_merge, dim3(cohap_blocks((int64_t)a.n_slots * a.M)), dim3(kApWaves * kWave), 0, s, a);
  return hipGetLastError();
}

}  // namespace ft8
