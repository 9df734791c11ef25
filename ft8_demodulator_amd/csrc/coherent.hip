// coherent.hip -- coherent re-demodulation of candidates from the samples (FT8_FLAG_COHERENT,
// ft8_coherent_llr; include/ft8hip.h, "coherent re-demodulation"; gfx950).
//
// Build-defined: the reference forms its LLRs once, from the dB bins of a one-symbol Hann STFT
// (ft8_decode.py:151-188).  Here a candidate BP failed on is demodulated again from the samples:
//   k_retry_list (ap.hip; the retry pass of ft8_internal.h) lists each slot's first M failed candidates
//   k_coherent   one 256-lane workgroup per list position (a slot's positions on one XCD):
//     1. baseband: the samples around the candidate are mixed down to the centre of the 8-tone band
//        and box-car decimated to Q samples per symbol (D = nsps / Q input samples each): the front
//        end it shares with k_sub_est (baseband.h);
//    1b. drift (ft8_set_coherent_drift / ft8_coherent_drift_llr only): the baseband is de-chirped in
//        place by each of n_rates linear drift rates and step 2 repeated; the best rate's copy goes on;
//     2. sync: over start offsets of +-hop/2 (steps of D samples) and tone-0 offsets of +-bin/2 (5
//        points) the 21 Costas symbols are correlated (coherent within a symbol, power summed over the
//        symbols that lie inside the slot); first largest wins, the tone-0 offset refined by a parabola;
//     3. the 58 x 8 tone spectra at the refined point (matched rectangular windows), the reference's
//        Gray map and max-of-4 LLRs in double, ftx_normalize_logl with NumPy's pairwise sums.
//    4b. multi-symbol sets (ft8_set_coherent_nsym / ft8_coherent_nsym_llr only): phase 3 keeps the complex
//        correlations, rotated to a common phase reference; per group of 2 or 3 adjacent data symbols one
//        wave forms the power of every joint tone tuple and the per-bit maxima, and each further set is
//        normalised like the first;
//   k_bp         unchanged (launch_bp, mode 0 over the compacted lists), once per set
//   k_coh_merge  one wave per list position: a valid fit whose attempt decoded rewrites its record
// No atomics; every sample index is range-checked or proven in range in 64-bit arithmetic.
#include <type_traits>

#include "baseband.h"

namespace ft8 {
namespace {

constexpr int kCohThreads = kBbThreads;
constexpr int kCohMaxT = 2 * (kBbMaxQ / 2) + 1;  // start offsets: 2 ceil(Q / (2 sps)) + 1
constexpr int kCohNF = 5;                        // tone-0 offsets (j - 2) bin / 4
constexpr int kSymbols = kBbSymbols, kSync = 21, kData = 58;
constexpr double kToneHz = 6.25;

__host__ __device__ inline int coh_rot_words(int Q) { return kCohNF * 8 * (Q + 1); }
// multi-symbol sets: the 58 x 8 rotated correlations of phase 3 follow rows 0 .. 7 of the rotation table,
// in rows 8 .. 39, which are dead by then (Q >= 14: they fit; below, the table's allocation grows)
__host__ __device__ inline int coh_multi_words(int Q) {
  const int need = 8 * (Q + 1) + kData * 8;
  return need > coh_rot_words(Q) ? need : coh_rot_words(Q);
}

__device__ __forceinline__ int costas_tone(int i) {  // 3 1 4 0 6 5 2, packed in nibbles
  return (int)((0x2560413u >> (4 * i)) & 7u);
}
__device__ __forceinline__ int gray_map(int j) {     // FT8_Gray_map 0 1 3 2 5 6 4 7
  return (int)((0x74652310u >> (4 * j)) & 7u);
}

// blank LLRs (of every set) and a fit that carries only its status
__device__ void coh_blank(double* llr, ft8_coh_fit* fit, int status, int sets = 1, int64_t set_stride = 0) {
  for (int n = 0; n < sets; ++n)
    for (int i = threadIdx.x; i < FT8_LDPC_N; i += kCohThreads) llr[n * set_stride + i] = 0.0;
  if (threadIdx.x == 0) {
    ft8_coh_fit f{};
    f.status = (uint8_t)status;
    *fit = f;
  }
}

// lane-owned elements of z in the drift search: ceil(max Mz / 256), Mz = 79 Q + 2 (Mt + 1), Mt <= Q / 2
constexpr int kCohOwn = (kSymbols * kBbMaxQ + 2 * (kBbMaxQ / 2 + 1) + kCohThreads - 1) / kCohThreads;

// Drift: step 1b of the contract, the sync of phase 2 repeated over n_rates de-chirped copies of z.
// The copies are made in place: z goes from rate i to i + 1 by one complex multiply per element with
// exp(-i pi (r_{i+1} - r_i) tau_m^2), a factor that is the same for every i (the rates are equidistant)
// and that each lane keeps in registers for the elements it owns; only the running best and its two
// tone-0 neighbours are kept, and one more rotation takes z to the winning rate before phase 3.
// The drift kernels take the search's settings as a further argument (CohDrift among G), the
// multi-symbol kernels theirs (CohMulti); without either (G empty) the kernel and its argument are the
// plain pass's.
template <typename T>
__device__ __forceinline__ T coh_arg() { return T{}; }
template <typename T, typename H, typename... R>
__device__ __forceinline__ T coh_arg(const H& h, const R&... r) {
  if constexpr (std::is_same_v<T, H>) return h;
  else return coh_arg<T>(r...);
}

template <typename InT, typename... G>
__global__ __launch_bounds__(kCohThreads) void k_coherent(CohLaunch a, G... opt) {
  FT8_RACE_PROLOGUE();
  constexpr bool Drift = (std::is_same_v<G, CohDrift> || ...);
  constexpr bool Multi = (std::is_same_v<G, CohMulti> || ...);
  [[maybe_unused]] const CohDrift g = coh_arg<CohDrift>(opt...);
  [[maybe_unused]] const CohMulti ms = coh_arg<CohMulti>(opt...);
  // dynamic LDS: z and the D twiddles of phase 1 (baseband.h's layout), then the rotation table
  // [5 * 8][Q + 1] of phase 2 (phase 3 rebuilds its first 8 rows for the refined offset)
  extern __shared__ float4 s_dyn[];
  float2* s_z = reinterpret_cast<float2*>(s_dyn);
  __shared__ float s_part[kCohMaxT * kCohNF * 3];
  __shared__ float s_metric[kCohMaxT * kCohNF];
  __shared__ float s_pow[kData * 8];
  __shared__ double s_llr[FT8_LDPC_N + 2];
  __shared__ double s_sq[FT8_LDPC_N + 2];
  __shared__ double s_sum[16];
  __shared__ double s_bc;
  __shared__ int s_flag, s_best;
  __shared__ float s_win[3];  // Drift: the winning metric between its two tone-0 neighbours
  __shared__ int s_rate;      // Drift: the winning rate index

  // list position -> (slot, candidate).  Per-slot lists: a slot's positions on one XCD (workgroup id
  // % 8, as k_sub_est), so its samples are served from that XCD's L2
  int64_t pos;
  int slot;
  if (a.slot_of) {
    pos = blockIdx.x;
    if (pos >= a.n) return;
    slot = a.slot_of[pos];
  } else {
    const int w = blockIdx.x, j8 = w / 8;
    slot = (w % 8) + 8 * (j8 / a.M);
    const int j = j8 % a.M;
    if (slot >= a.b.n_slots || j >= a.count[slot]) return;
    pos = (int64_t)slot * a.M + j;
  }
  double* llr_out = a.llr + pos * (Multi ? ms.pos_stride : (int64_t)FT8_LDPC_N);
  ft8_coh_fit* fit_out = a.fit + pos;
  // status 2 or 3: zeros in every set, no set valid
  auto blank = [&](int status) {
    if constexpr (Multi) {
      coh_blank(llr_out, fit_out, status, ms.nsym, ms.set_stride);
      if (ms.valid && threadIdx.x == 0) ms.valid[pos] = 0;
    } else {
      coh_blank(llr_out, fit_out, status);
    }
  };
  if (slot < 0 || slot >= a.b.n_slots) {
    blank(3);
    if constexpr (Drift)
      if (g.out && threadIdx.x == 0) g.out[pos] = ft8_coh_drift{};
    return;
  }
  const Baseband& bb = a.b;
  const InT* x = reinterpret_cast<const InT*>(bb.x) + (int64_t)slot * bb.slot_stride;
  const BbGeom geo = bb_geom(bb.nsps, bb.hop, bb.Q);
  const int nsps = bb.nsps, Q = geo.Q, D = geo.D, Mt = geo.Mt, Mg = geo.Mg, Mz = geo.Mz, nT = geo.nT;
  const double fs = bb.fs;
  const double bin = fs / (double)bb.nfft;
  const int64_t s0 = ((int64_t)bb.t_lo + a.cand[2 * pos]) * bb.hop;
  const double fmix = (double)((int64_t)bb.f_lo + a.cand[2 * pos + 1]) * bin + 3.5 * kToneHz;
  const int64_t nb = bb_nb(geo, s0);
  // symbol k at start offset d - Mt is present when its nsps input samples lie in [0, n_samples)
  auto present = [&](int d, int k) {
    const int64_t first = nb + ((int64_t)(1 + d) + (int64_t)k * Q) * D;
    return first >= 0 && first + nsps <= bb.n_samples;
  };

  // ---- nothing to measure: no Costas symbol inside the slot at any start offset
  if (threadIdx.x == 0) s_flag = 0;
  __syncthreads();
  for (int e = threadIdx.x; e < nT * kSync; e += kCohThreads) {
    const int d = e / kSync, si = e - d * kSync;
    if (present(d, (si / 7) * 36 + si % 7)) s_flag = 1;
  }
  __syncthreads();
  if (!s_flag) {
    blank(2);
    if constexpr (Drift)
      if (g.out && threadIdx.x == 0) g.out[pos] = ft8_coh_drift{};
    return;
  }

  // ---- 1. the mixed-down, decimated baseband z (baseband.h)
  float2* s_tw = s_z + bb_z_words(Q);
  float2* s_R = s_z + bb_tail_at(Q, D);
  bb_twiddles(s_tw, D, fmix, fs);
  // rotation powers of phase 2, each from its exact phase: row j * 8 + t, entry q
  for (int e = threadIdx.x; e < coh_rot_words(Q); e += kCohThreads) {
    const int ft = e / (Q + 1), q = e - ft * (Q + 1);
    const int t = ft & 7, j = ft >> 3;
    const double nu = (double)t - 3.5 + ((double)(j - 2) * bin / 4.0) / kToneHz;  // tones relative to fmix
    s_R[e] = bb_rot(nu * (double)q / (double)Q);
  }
  __syncthreads();
  bb_mix_down<InT, kBbLd>(x, bb.n_samples, nb, geo, fmix, fs, s_tw, s_z);
  __syncthreads();

  // ---- 2. sync: item (start offset d, tone-0 offset j, Costas block b) sums its 7 symbols' powers in
  // symbol order; window element q of symbol k at offset d is z[1 + k Q + d + q]
  // Drift (step 1b of the contract): the rates r_i = (i - ic) rstep, i ascending, each searched as
  // below on z de-chirped in place; tau_m is the centre of decimation block m relative to the centre of
  // the nominal signal.  A lane owns z[tid + 256 u], as in phase 1.
  const int R = Drift ? g.n_rates : 1, ic = (R - 1) / 2;
  const double rstep = Drift ? 2.0 * (double)g.max_rate / (double)(R - 1) : 0.0;
  auto tau2 = [&](int m) {
    const double t = (((double)(m - Mg) + 0.5) * (double)D - 39.5 * (double)nsps) / fs;
    return t * t;
  };
  int zi[kCohOwn];     // the element's word in s_z, -1 past Mz
  float2 wr[kCohOwn];  // exp(-i pi rstep tau^2) from its exact phase
  auto rotate = [&](auto factor) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < kCohOwn; ++u)
      if (zi[u] >= 0) {
        const float2 z = s_z[zi[u]], w = factor(u);
        s_z[zi[u]] = make_float2(z.x * w.x - z.y * w.y, z.x * w.y + z.y * w.x);
      }
  };
  // by dr Hz/s, the factor from its exact phase
  auto rotate_exact = [&](double dr) __attribute__((always_inline)) {
    rotate([&](int u) { return bb_rot(0.5 * dr * tau2(threadIdx.x + u * kCohThreads)); });
  };
  if constexpr (Drift) {
#pragma unroll
    for (int u = 0; u < kCohOwn; ++u) {
      const int m = threadIdx.x + u * kCohThreads;
      zi[u] = m < Mz ? bb_z_at(Q, m) : -1;
      wr[u] = bb_rot(0.5 * rstep * tau2(m));
    }
    rotate_exact((double)(-ic) * rstep);
    __syncthreads();
  }
  int ri = 0;
  do {  // one trip without Drift
    if constexpr (Drift)
      if (ri > 0) {
        rotate([&](int u) { return wr[u]; });
        __syncthreads();
      }
    for (int e = threadIdx.x; e < nT * kCohNF * 3; e += kCohThreads) {
      const int d = e / (kCohNF * 3), r = e - d * (kCohNF * 3);
      const int j = r / 3, b = r - 3 * j;
      float sum = 0.f;
      for (int i = 0; i < 7; ++i) {
        const int k = 36 * b + i;
        if (!present(d, k)) continue;
        const float2* Wp = s_R + (j * 8 + costas_tone(i)) * (Q + 1);
        const float2* zp = s_z + (k + 1) * (Q + 1);
        float cx = 0.f, cy = 0.f;
        for (int q = 0; q < Q; ++q) {
          const int jj = d + q;  // < 3 Q: the row padding without a division
          const float2 z = zp[jj + (jj >= Q) + (jj >= 2 * Q)], W = Wp[q];
          cx = fmaf(z.x, W.x, fmaf(-z.y, W.y, cx));
          cy = fmaf(z.x, W.y, fmaf(z.y, W.x, cy));
        }
        sum += cx * cx + cy * cy;
      }
      s_part[e] = sum;
    }
    __syncthreads();
    for (int h = threadIdx.x; h < nT * kCohNF; h += kCohThreads)
      s_metric[h] = (s_part[3 * h] + s_part[3 * h + 1]) + s_part[3 * h + 2];
    __syncthreads();
    if (threadIdx.x == 0) {  // the first largest, start offset outer, tone-0 offset inner
      int b = 0;
      for (int h = 1; h < nT * kCohNF; ++h)
        if (s_metric[h] > s_metric[b]) b = h;
      if constexpr (!Drift) {
        s_best = b;
      } else if (ri == 0 || s_metric[b] > s_win[1]) {  // ... and the rate outermost
        s_win[0] = b > 0 ? s_metric[b - 1] : 0.f;
        s_win[1] = s_metric[b];
        s_win[2] = b + 1 < nT * kCohNF ? s_metric[b + 1] : 0.f;
        s_best = b;
        s_rate = ri;
      }
    }
    // Drift: thread 0 reads s_metric before it arrives at the next trip's barriers, and until then the
    // others write only s_z and s_part
  } while (Drift && ++ri < R);
  __syncthreads();
  if constexpr (Drift) {
    // z stands at rate R - 1; phase 3's barrier after its table orders this before the spectra
    if (s_rate != R - 1) rotate_exact((double)(s_rate - (R - 1)) * rstep);
  }
  const int hb = s_best;
  const int db = hb / kCohNF, jb = hb - db * kCohNF;
  double delta = 0.0;
  if (jb > 0 && jb < kCohNF - 1) {
    const double m_ = Drift ? s_win[0] : s_metric[hb - 1], m0 = Drift ? s_win[1] : s_metric[hb],
                 mp = Drift ? s_win[2] : s_metric[hb + 1];
    const double den = m_ - 2.0 * m0 + mp;
    if (den < 0.0) delta = 0.5 * (m_ - mp) / den;
  }
  const double df = ((double)(jb - 2) + delta) * bin / 4.0;

  // ---- 3. spectra of the data symbols at (db, df); the rotations replace rows 0 .. 7 of the table
  for (int e = threadIdx.x; e < 8 * (Q + 1); e += kCohThreads) {
    const int t = e / (Q + 1), q = e - t * (Q + 1);
    s_R[e] = bb_rot(((double)t - 3.5 + df / kToneHz) * (double)q / (double)Q);
  }
  __syncthreads();
  for (int e = threadIdx.x; e < kData * 8; e += kCohThreads) {
    const int kd = e >> 3, t = e & 7;
    const int k = kd + (kd < 29 ? 7 : 14);
    const float2* Wp = s_R + t * (Q + 1);
    const float2* zp = s_z + (k + 1) * (Q + 1);
    float cx = 0.f, cy = 0.f;
    for (int q = 0; q < Q; ++q) {
      const int jj = db + q;
      const float2 z = zp[jj + (jj >= Q) + (jj >= 2 * Q)], W = Wp[q];
      cx = fmaf(z.x, W.x, fmaf(-z.y, W.y, cx));
      cy = fmaf(z.x, W.y, fmaf(z.y, W.x, cy));
    }
    s_pow[e] = cx * cx + cy * cy;
    if constexpr (Multi) {
      // step 4b, items 1 and 2: c'_k[t], carried to symbol 0's phase reference; 0 for an absent symbol
      const float2 w = bb_rot((df / kToneHz - 3.5) * (double)k);
      s_R[8 * (Q + 1) + e] =
          present(db, k) ? make_float2(cx * w.x - cy * w.y, cx * w.y + cy * w.x) : make_float2(0.f, 0.f);
    }
  }
  __syncthreads();
  if (threadIdx.x < kData) {  // ft8_extract_symbol in double
    const int kd = threadIdx.x;
    const int k = kd + (kd < 29 ? 7 : 14);
    double l0 = 0.0, l1 = 0.0, l2 = 0.0;
    if (present(db, k)) {
      double s2[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) s2[j] = 10.0 * log10(1e-12 + (double)s_pow[kd * 8 + gray_map(j)]);
      auto max4 = [](double p, double q, double r, double s) { return fmax(fmax(p, q), fmax(r, s)); };
      l0 = max4(s2[4], s2[5], s2[6], s2[7]) - max4(s2[0], s2[1], s2[2], s2[3]);
      l1 = max4(s2[2], s2[3], s2[6], s2[7]) - max4(s2[0], s2[1], s2[4], s2[5]);
      l2 = max4(s2[1], s2[3], s2[5], s2[7]) - max4(s2[0], s2[2], s2[4], s2[6]);
    }
    s_llr[3 * kd] = l0;
    s_llr[3 * kd + 1] = l1;
    s_llr[3 * kd + 2] = l2;
  }
  __syncthreads();
  // ftx_normalize_logl with NumPy's pairwise sums (k_llr's: 8 accumulators, blocks of 80 + 94)
  auto pairwise174 = [&](const double* v) {
    const int l = threadIdx.x;
    if (l < 8) {
      double r = v[l];
      for (int i = 8; i < 80; i += 8) r += v[i + l];
      s_sum[l] = r;
    } else if (l < 16) {
      const int j = l - 8;
      double r = v[80 + j];
      for (int i = 8; i < 88; i += 8) r += v[80 + i + j];
      s_sum[l] = r;
    }
    __syncthreads();
    if (l == 0) {
      const double* p = s_sum;
      const double s1 = ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]));
      double s2 = ((p[8] + p[9]) + (p[10] + p[11])) + ((p[12] + p[13]) + (p[14] + p[15]));
      for (int i = 168; i < FT8_LDPC_N; ++i) s2 += v[i];
      s_bc = 0.0 + (s1 + s2);
    }
    __syncthreads();
    const double tot = s_bc;
    __syncthreads();
    return tot;
  };
  const double mean = pairwise174(s_llr) / 174.0;
  for (int i = threadIdx.x; i < FT8_LDPC_N; i += kCohThreads) {
    const double dd = s_llr[i] - mean;
    s_sq[i] = dd * dd;
  }
  __syncthreads();
  const double var = pairwise174(s_sq) / 174.0;
  const bool valid = var > 0.0;  // false for 0 and NaN
  const double scale = valid ? sqrt(24.0 / var) : 0.0;
  for (int i = threadIdx.x; i < FT8_LDPC_N; i += kCohThreads) llr_out[i] = valid ? s_llr[i] * scale : 0.0;
  if (threadIdx.x == 0) {
    int ns = 0;
    for (int si = 0; si < kSync; ++si) ns += present(db, (si / 7) * 36 + si % 7) ? 1 : 0;
    ft8_coh_fit f{};
    f.dt_s = (float)((double)(db - Mt) * (double)D / fs);
    f.df_hz = (float)df;
    f.metric = Drift ? s_win[1] : s_metric[hb];
    f.n_sync = (uint8_t)ns;
    f.status = valid ? 0 : 2;
    f.dt_index = (int8_t)(db - Mt);
    f.df_index = (uint8_t)jb;
    *fit_out = f;
    if constexpr (Drift)
      if (g.out) {
        ft8_coh_drift w;
        w.rate_hz_per_s = (float)((double)(s_rate - ic) * rstep);
        w.rate_index = s_rate;
        g.out[pos] = w;
      }
  }
  if constexpr (Multi) {
    // ---- 4b. sets 2 .. S: joint metrics over groups of n adjacent data symbols.  One wave per group:
    // lane (j1, j2) fixes the first two tones (tone gray_map(j) carries the bits of j), loops over the
    // third and keeps, per symbol, bit and bit value, the largest power over its tuples; float max is
    // exact, so the wave reduction's order does not matter.  0 is the identity: powers are >= 0 and
    // every (symbol, bit, value) has a tuple.  The maxima replace s_pow, which set 1 has consumed.
    const float2* s_c = s_R + 8 * (Q + 1);
    float* s_max = s_pow;  // [58][bit][value]
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    const int j1 = lane >> 3, j2 = lane & 7;
    int vbits = valid ? 1 : 0;
    // set 1's normalisation above, for a further set (set 1 keeps its own statements: as a call of this
    // lambda it changed the register allocation of the plain and the drift instantiations)
    auto normalise = [&](double* out) {
      const double mean_n = pairwise174(s_llr) / 174.0;
      for (int i = threadIdx.x; i < FT8_LDPC_N; i += kCohThreads) {
        const double dd = s_llr[i] - mean_n;
        s_sq[i] = dd * dd;
      }
      __syncthreads();
      const double var_n = pairwise174(s_sq) / 174.0;
      const bool ok = var_n > 0.0;
      const double scale_n = ok ? sqrt(24.0 / var_n) : 0.0;
      for (int i = threadIdx.x; i < FT8_LDPC_N; i += kCohThreads) out[i] = ok ? s_llr[i] * scale_n : 0.0;
      return ok;
    };
    for (int n = 2; n <= ms.nsym; ++n) {
      double* out_n = llr_out + (int64_t)(n - 1) * ms.set_stride;
      if (!valid) {  // workgroup-uniform: an invalid fit has no further sets
        for (int i = threadIdx.x; i < FT8_LDPC_N; i += kCohThreads) out_n[i] = 0.0;
        continue;
      }
      const int per_half = (29 + n - 1) / n;
      for (int gi = wave; gi < 2 * per_half; gi += kCohThreads / kWave) {
        const int h = gi / per_half, r = gi - h * per_half;
        const int kd0 = 29 * h + r * n, len = min(n, 29 - r * n);
        const float2 c1 = s_c[kd0 * 8 + gray_map(j1)];
        const float2 c2 = len > 1 ? s_c[(kd0 + 1) * 8 + gray_map(j2)] : make_float2(0.f, 0.f);
        const float bx = c1.x + c2.x, by = c1.y + c2.y;
        float v[18];
#pragma unroll
        for (int e = 0; e < 18; ++e) v[e] = 0.f;
        float pm = 0.f;
        const int n3 = len > 2 ? 8 : 1;
        for (int j3 = 0; j3 < n3; ++j3) {
          const float2 c3 = len > 2 ? s_c[(kd0 + 2) * 8 + gray_map(j3)] : make_float2(0.f, 0.f);
          const float x = bx + c3.x, y = by + c3.y;
          const float p = x * x + y * y;
          pm = fmaxf(pm, p);
#pragma unroll
          for (int b = 0; b < 3; ++b) {
            const bool one = (j3 >> (2 - b)) & 1;
            v[12 + 2 * b] = fmaxf(v[12 + 2 * b], one ? 0.f : p);
            v[12 + 2 * b + 1] = fmaxf(v[12 + 2 * b + 1], one ? p : 0.f);
          }
        }
#pragma unroll
        for (int b = 0; b < 3; ++b) {
          const bool one1 = (j1 >> (2 - b)) & 1, one2 = (j2 >> (2 - b)) & 1;
          v[2 * b] = one1 ? 0.f : pm;
          v[2 * b + 1] = one1 ? pm : 0.f;
          v[6 + 2 * b] = one2 ? 0.f : pm;
          v[6 + 2 * b + 1] = one2 ? pm : 0.f;
        }
#pragma unroll
        for (int e = 0; e < 18; ++e) {
#pragma unroll
          for (int o = kWave / 2; o > 0; o >>= 1) v[e] = fmaxf(v[e], __shfl_xor(v[e], o, kWave));
          if (lane == e && e < 6 * len) s_max[kd0 * 6 + e] = v[e];
        }
      }
      __syncthreads();
      if (threadIdx.x < kData) {
        const int kd = threadIdx.x;
#pragma unroll
        for (int b = 0; b < 3; ++b)
          s_llr[3 * kd + b] = 10.0 * log10(1e-12 + (double)s_max[kd * 6 + 2 * b + 1]) -
                              10.0 * log10(1e-12 + (double)s_max[kd * 6 + 2 * b]);
      }
      __syncthreads();
      if (normalise(out_n)) vbits |= 1 << (n - 1);
    }
    if (ms.valid && threadIdx.x == 0) ms.valid[pos] = (uint8_t)vbits;
  }
}

// the validity bytes of one set (max_nsym = 1 of the stage call): bit 0 for a valid fit
__global__ void k_coh_valid1(const ft8_coh_fit* fit, uint8_t* valid, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) valid[i] = fit[i].status == 0 ? 1 : 0;
}

// one wave per list position: a valid fit whose attempt the tail accepted rewrites its record
__global__ __launch_bounds__(4 * kWave) void k_coh_merge(CohPass a) {
  const RetryLists& r = a.r;
  const int lane = threadIdx.x % kWave;
  const int64_t pos = (int64_t)blockIdx.x * 4 + threadIdx.x / kWave;
  if (pos >= (int64_t)r.n_slots * r.M) return;
  const int slot = (int)(pos / r.M), j = (int)(pos % r.M);
  if (j >= r.count[slot]) return;
  const ft8_result& got = a.res_c[pos];
  if (!got.ok || a.fit[pos].status != 0) return;
  ft8_result* rec = r.res + (int64_t)slot * r.N + r.list[pos];
  // a.valid (null with one set): set a.set must be valid, and the first set that decodes wins
  if (a.valid && (!((a.valid[pos] >> a.set) & 1) || rec->ok)) return;
  // a.drift (null without the drift search): a rescue at a rate other than 0 also sets bit 2; a set
  // after the first sets bit 3
  const int bits = (a.drift && a.drift[pos].rate_hz_per_s != 0.f ? 6 : 2) | (a.set > 0 ? 8 : 0);
  if (lane == 0) retry_accept(rec, got, bits);
}

}  // namespace

size_t coherent_lds_bytes(int nsps, int Q, bool multi) {
  return sizeof(float2) * ((size_t)bb_tail_at(Q, nsps / Q) + (size_t)(multi ? coh_multi_words(Q) : coh_rot_words(Q)));
}

hipError_t launch_coherent(const CohLaunch& a, const CohDrift& g, const CohMulti& m, hipStream_t s) {
  const int64_t grid = a.slot_of ? (int64_t)a.n : (int64_t)((a.b.n_slots + 7) / 8) * 8 * a.M;
  if (grid <= 0) return hipSuccess;
  if (!bb_valid(a.b)) return hipErrorInvalidValue;
  const size_t lds = coherent_lds_bytes(a.b.nsps, a.b.Q, coherent_multi_on(m));
  if (coherent_multi_on(m)) {
    if (m.nsym > 3) return hipErrorInvalidValue;
    const dim3 gr((unsigned)grid), bl(kCohThreads);
    if (coherent_drift_on(g)) {
      if (a.b.dtype == FT8_I16) return lds_launch(k_coherent<int16_t, CohDrift, CohMulti>, gr, bl, lds, s, a, g, m);
      return lds_launch(k_coherent<float, CohDrift, CohMulti>, gr, bl, lds, s, a, g, m);
    }
    if (a.b.dtype == FT8_I16) return lds_launch(k_coherent<int16_t, CohMulti>, gr, bl, lds, s, a, m);
    return lds_launch(k_coherent<float, CohMulti>, gr, bl, lds, s, a, m);
  }
  if (coherent_drift_on(g)) {
    if (a.b.dtype == FT8_I16)
      return lds_launch(k_coherent<int16_t, CohDrift>, dim3((unsigned)grid), dim3(kCohThreads), lds, s, a, g);
    return lds_launch(k_coherent<float, CohDrift>, dim3((unsigned)grid), dim3(kCohThreads), lds, s, a, g);
  }
  if (a.b.dtype == FT8_I16) return lds_launch(k_coherent<int16_t>, dim3((unsigned)grid), dim3(kCohThreads), lds, s, a);
  return lds_launch(k_coherent<float>, dim3((unsigned)grid), dim3(kCohThreads), lds, s, a);
}

hipError_t launch_coh_valid1(const ft8_coh_fit* fit, uint8_t* valid, int n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_coh_valid1, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, fit, valid, n);
  return hipGetLastError();
}

hipError_t launch_coh_merge(const CohPass& a, hipStream_t s) {
  if (a.r.n_slots <= 0 || a.r.M <= 0) return hipSuccess;
  const unsigned blocks = (unsigned)(((int64_t)a.r.n_slots * a.r.M + 3) / 4);
  hipLaunchKernelGGL(k_coh_merge, dim3(blocks), dim3(4 * kWave), 0, s, a);
  return hipGetLastError();
}

}  // namespace ft8
