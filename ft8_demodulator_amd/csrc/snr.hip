// snr.hip -- the signal report of a decode: the slot's noise floor (k_noise_floor, k_noise_rank) and
// the power of the decoded message's own tones against it (k_snr).  Build-defined, outside reference
// parity (the reference stops at the payload).  The estimator, step by step, is in DESIGN.md section
// 10 and is restated in NumPy by ft8_demodulator_amd/snr.py (snr_reference), which the tests compare
// against.
//
// Every waterfall value is widened to double and all arithmetic is double.  The kernels add in a
// fixed order (a column's rows in time order, a message's symbols in symbol order), so a result
// depends on the values alone: not on the grid, the pipeline setting or the run.
#include "ft8_internal.h"
#include "tx_device.h"

namespace ft8 {

// dB -> linear power, P = 10^(v / 10), evaluated as 2^(v log2(10) / 10): one multiply and exp2
// instead of a division and exp10, about half the FP64 instructions of the kernel that evaluates it
// for every waterfall value.  The roundings of the constant and of the product move the result by at
// most |v| / 10 * 5.1e-16 relative (8e-15 at -150 dB) beside exp2's own last-place error.
template <typename T>
__device__ __forceinline__ double lin_power(T v) {
  return exp2((double)v * 0.33219280948873623);  // log2(10) / 10
}

// ---- k_noise_floor, k_noise_rank ----------------------------------------------------------------------
// k_noise_floor: A[f], the time mean of every column's linear power.  Grid (column chunks of
// kNfCols, slots), one column per lane: consecutive lanes read consecutive bins of a row, every
// value is read once, and a lane adds its column's rows in the order t = 0 .. T - 1 (no atomics, no
// reordering), with the loads of kNfRows rows issued before their powers are added.  This is the hot
// part (the whole waterfall, 366 MB for 256 slots at 12 kHz); one workgroup per slot, the shape that
// would let one kernel finish the quantile too, streams it at less than half the rate (DESIGN.md
// section 6d), so the quantile is a kernel of its own.
//
// k_noise_rank: the element of rank `rank` of A sorted ascending, NaNs after every number, on an
// order-preserving 64-bit key per column; one workgroup per slot.  F <= kNfStageF: the keys, padded
// with the largest key to a power of two, are sorted in LDS (bitonic, one compare-exchange per lane
// and step) and the key at `rank` is the floor -- equal values need no tie-break, whichever of them
// stands at the rank has the value.  Wider waterfalls (64 KB of LDS would not hold their keys) count
// instead: lane l counts the columns that order before its own (key, then column index) and the one
// column whose count is `rank` is the floor; F^2 comparisons, so slow, but no F is refused.
constexpr int kNfCols = 128;
constexpr int kNfRows = 8;
constexpr int kNfThreads = 1024;
constexpr int kNfStageF = 8192;
constexpr int kNfMaxGridY = 65535;

inline __host__ __device__ int nf_pow2(int F) {
  int n = 1;
  while (n < F) n <<= 1;
  return n;
}

__device__ __forceinline__ unsigned long long nf_key(double v) { return v != v ? ~0ull : order_key(v); }

template <typename T>
__global__ __launch_bounds__(kNfCols) void k_noise_floor(const T* wf, int nT, int F, double* colmean) {
  const int s = blockIdx.y, f = blockIdx.x * kNfCols + threadIdx.x;
  if (f >= F) return;
  const T* W = wf + (size_t)s * nT * F + f;
  double sum = 0.0;
  int t = 0;
  for (; t + kNfRows <= nT; t += kNfRows) {
    T v[kNfRows];
#pragma unroll
    for (int u = 0; u < kNfRows; ++u) v[u] = W[(size_t)(t + u) * F];
#pragma unroll
    for (int u = 0; u < kNfRows; ++u) sum += lin_power(v[u]);
  }
  for (; t < nT; ++t) sum += lin_power(W[(size_t)t * F]);
  colmean[(size_t)s * F + f] = sum / (double)nT;
}

__global__ __launch_bounds__(kNfThreads) void k_noise_rank(const double* colmean, int F, int rank, int staged,
                                                           double* floor_out) {
  FT8_RACE_PROLOGUE();
  extern __shared__ unsigned long long s_key[];  // staged: [nf_pow2(F)]
  const int s = blockIdx.x, tid = threadIdx.x;
  const double* A = colmean + (size_t)s * F;
  if (staged) {
    const int n2 = nf_pow2(F);
    for (int f = tid; f < n2; f += kNfThreads) s_key[f] = f < F ? nf_key(A[f]) : ~0ull;
    __syncthreads();
    for (int k = 2; k <= n2; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int p = tid; p < n2 / 2; p += kNfThreads) {
          const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), l = i | j;  // the pair (i, i ^ j), i < l
          const unsigned long long a = s_key[i], b = s_key[l];
          if ((a > b) == ((i & k) == 0)) {
            s_key[i] = b;
            s_key[l] = a;
          }
        }
        __syncthreads();
      }
    }
    if (tid == 0) floor_out[s] = key_value(s_key[rank]);  // the NaN key reads back as a NaN
    return;
  }
  for (int f = tid; f < F; f += kNfThreads) {
    const unsigned long long kf = nf_key(A[f]);
    int before = 0;
    for (int g = 0; g < F; ++g) {
      const unsigned long long kg = nf_key(A[g]);
      before += (kg < kf || (kg == kf && g < f)) ? 1 : 0;
    }
    if (before == rank) floor_out[s] = A[f];
  }
}

hipError_t launch_noise_floor(const void* wf, int wf_f64, int n_slots, int T, int F, int rank, double* floor_out,
                              double* colmean, hipStream_t s) {
  if (n_slots <= 0) return hipSuccess;
  const size_t esz = wf_f64 ? 8 : 4;
  for (int s0 = 0; s0 < n_slots; s0 += kNfMaxGridY) {  // gridDim.y holds 65535 slots
    const dim3 grid((F + kNfCols - 1) / kNfCols, n_slots - s0 < kNfMaxGridY ? n_slots - s0 : kNfMaxGridY);
    const char* w = (const char*)wf + esz * (size_t)s0 * T * F;
    double* A = colmean + (size_t)s0 * F;
    if (wf_f64) hipLaunchKernelGGL(k_noise_floor<double>, grid, dim3(kNfCols), 0, s, (const double*)w, T, F, A);
    else hipLaunchKernelGGL(k_noise_floor<float>, grid, dim3(kNfCols), 0, s, (const float*)w, T, F, A);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  const int staged = F <= kNfStageF;
  const size_t lds = staged ? sizeof(unsigned long long) * (size_t)nf_pow2(F) : 0;
  return lds_launch(k_noise_rank, dim3(n_slots), dim3(kNfThreads), lds, s, (const double*)colmean, F, rank, staged,
                    floor_out);
}

// ---- k_snr ------------------------------------------------------------------------------------------
// One wave (one 64-lane workgroup) per record.  The wave re-encodes the payload into LDS
// (encode_tones_wave), then lane k (and k + 64) reads symbol k's tone bin at each of the (2 r + 1)^2
// grid offsets and leaves the linear powers in LDS; lane o then adds offset o's powers in symbol
// order and lane 0 takes the first largest mean in scan order (dt outer, df inner, ascending).  Rows
// outside [0, T) are skipped, offsets whose 8 tone bins do not all lie in [0, F) are not considered:
// no index leaves the slot's waterfall.
constexpr int kSnrMaxOff = 9;  // radius <= 1

template <typename T>
__global__ __launch_bounds__(kWave) void k_snr(const T* wf, int nT, int F, int sps, int bpt, const ft8_result* rec,
                                               const int32_t* counts, int cap, const double* floor_in, int radius,
                                               double bw_db, ft8_snr_rec* out) {
  __shared__ uint8_t s_tones[80];
  __shared__ double s_p[kSnrMaxOff][tx::kSymbols];
  __shared__ double s_m[kSnrMaxOff];
  __shared__ int s_n[kSnrMaxOff];
  const int lane = threadIdx.x;
  const int64_t i = blockIdx.x;
  const int s = (int)(i / cap), r = (int)(i % cap);
  const int n = counts ? min(max(counts[s], 0), cap) : cap;
  const ft8_result* R = rec + i;
  ft8_snr_rec o{};
  if (r >= n || R->ok == 0) {  // the whole workgroup leaves: no barrier is skipped by a part of it
    o.status = 3;
    if (lane == 0) out[i] = o;
    return;
  }
  tx::encode_tones_wave(R->payload, lane, s_tones);
  __syncthreads();
  const int side = 2 * radius + 1, n_off = side * side;
  const int64_t at = R->abs_time, af = R->abs_freq;
  const int64_t f_span = 7 * (int64_t)bpt;
  const T* W = wf + (size_t)s * nT * F;
  for (int k = lane; k < tx::kSymbols; k += kWave) {
    const int64_t col = (int64_t)s_tones[k] * bpt;
    for (int q = 0; q < n_off; ++q) {
      const int dt = q / side - radius, df = q % side - radius;
      const int64_t row = at + dt + (int64_t)k * sps, f0 = af + df;
      double p = 0.0;
      if (f0 >= 0 && f0 + f_span <= (int64_t)F - 1 && row >= 0 && row < nT) p = lin_power(W[row * F + f0 + col]);
      s_p[q][k] = p;
    }
  }
  __syncthreads();
  if (lane < n_off) {
    const int dt = lane / side - radius, df = lane % side - radius;
    const int64_t f0 = af + df;
    double sum = 0.0;
    int cnt = 0;
    if (f0 >= 0 && f0 + f_span <= (int64_t)F - 1) {
      for (int k = 0; k < tx::kSymbols; ++k) {
        const int64_t row = at + dt + (int64_t)k * sps;
        if (row < 0 || row >= nT) continue;
        sum += s_p[lane][k];
        ++cnt;
      }
    }
    const double m = cnt > 0 ? sum / (double)cnt : 0.0;
    s_m[lane] = m;
    s_n[lane] = (cnt > 0 && m == m) ? cnt : 0;  // no usable row, or a NaN mean: skipped
  }
  __syncthreads();
  if (lane != 0) return;
  int best = -1;
  for (int q = 0; q < n_off; ++q)
    if (s_n[q] > 0 && (best < 0 || s_m[q] > s_m[best])) best = q;
  if (best < 0) {
    o.status = 2;
    out[i] = o;
    return;
  }
  const double n0 = floor_in[s];
  double sig = s_m[best] - n0;
  if (sig < 1e-3 * n0) {
    sig = 1e-3 * n0;
    o.status = 1;
  }
  o.snr_db = 10.0 * log10(sig / n0) + bw_db;
  o.signal_db = (float)(10.0 * log10(sig));
  o.noise_db = (float)(10.0 * log10(n0));
  o.dt = (int8_t)(best / side - radius);
  o.df = (int8_t)(best % side - radius);
  o.n_symbols = (uint8_t)s_n[best];
  out[i] = o;
}

hipError_t launch_snr(const void* wf, int wf_f64, int n_slots, int T, int F, int sps, int bpt, const ft8_result* rec,
                      const int32_t* counts, int cap, const double* floor_in, int radius, double bw_db,
                      ft8_snr_rec* out, hipStream_t s) {
  if (n_slots <= 0 || cap <= 0) return hipSuccess;
  const dim3 grid((unsigned)((int64_t)n_slots * cap));
  if (wf_f64)
    hipLaunchKernelGGL(k_snr<double>, grid, dim3(kWave), 0, s, (const double*)wf, T, F, sps, bpt, rec, counts, cap,
                       floor_in, radius, bw_db, out);
  else
    hipLaunchKernelGGL(k_snr<float>, grid, dim3(kWave), 0, s, (const float*)wf, T, F, sps, bpt, rec, counts, cap,
                       floor_in, radius, bw_db, out);
  return hipGetLastError();
}

}  // namespace ft8
