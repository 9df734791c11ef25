// baseband.h -- the baseband front end of k_sub_est (subtract.hip, phase 2) and k_coherent
// (coherent.hip, phase 1) as device functions (gfx950): a candidate's samples are mixed down to the
// centre of the 8-tone band and box-car decimated to Q samples per symbol (D = nsps / Q input samples
// each) into padded LDS rows of Q + 1.  The one definition of the LDS layout, the search geometry, the
// sample loads, the exact-phase rotation and the mix-down loop; both launchers size their LDS from it.
// The rotation tables of the phases that follow stay in their kernels: their phase arguments are
// rounded differently (nu D q / fs in k_sub_est, nu q / Q in k_coherent), so one table would change bits.
#pragma once
#include "ft8_internal.h"

namespace ft8 {

constexpr int kBbThreads = 256;  // lanes of a workgroup; a lane owns z[tid + 256 j]
constexpr int kBbMaxQ = 32;
constexpr int kBbSymbols = 79;
constexpr int kBbLd = 8;         // 4-sample loads bb_mix_down issues before it uses the first

// ---- LDS layout: z | twiddles | the kernel's own rotation table --------------------------------
// z is stored in rows of Q + 1 (one pad): row r + 1 holds z[1 + r Q .. 1 + (r + 1) Q), r = -1 .. 81,
// so symbol k's window starts a row and the lanes' reads (one symbol per lane) are 2 (Q + 1) dwords
// apart -- distinct banks for even Q.  Unpadded, the lanes of a ds_read_b64 were 2 Q dwords apart: at
// Q = 32 one bank for all 32 lanes of a group (32-way conflicts; 169 M conflict cycles per 334-slot
// launch, r4_v30_sub_pmc.json).
// float2 words of the rows, rounded up to a 16-B multiple
__host__ __device__ inline int bb_z_words(int Q) { return ((kBbSymbols + 4) * (Q + 1) + 1) & ~1; }
// ... of the decimation's D twiddles
__host__ __device__ inline int bb_tw_words(int D) { return (D + 1) & ~1; }
// ... before what follows z and the twiddles
__host__ __device__ inline int bb_tail_at(int Q, int D) { return bb_z_words(Q) + bb_tw_words(D); }
// z[m] -> its padded position (m >= 0; Mg - Mt = 1 is the first window's start)
__device__ __forceinline__ int bb_z_at(int Q, int m) {
  const int u = m - 1 + Q;
  return u + (int)((unsigned)u / (unsigned)Q);
}

// ---- search geometry: start offsets of +-hop/2 in steps of D samples ------------------------------
struct BbGeom {
  int Q, D;
  int Mt;  // ceil((hop / 2) / D): start offsets -Mt .. Mt
  int Mg;  // decimated samples before the nominal start
  int Mz;  // decimated samples in all
  int nT;  // start offsets searched
};
__host__ __device__ inline BbGeom bb_geom(int nsps, int hop, int Q) {
  const int sps = nsps / hop;
  BbGeom g;
  g.Q = Q;
  g.D = nsps / Q;
  g.Mt = (Q + 2 * sps - 1) / (2 * sps);
  g.Mg = g.Mt + 1;
  g.Mz = kBbSymbols * Q + 2 * g.Mg;
  g.nT = 2 * g.Mt + 1;
  return g;
}
// first input sample of z[0] for a nominal start s0 (negative at the slot's head)
__host__ __device__ inline int64_t bb_nb(const BbGeom& g, int64_t s0) { return s0 - (int64_t)g.Mg * g.D; }
// what both kernels assume of a launch's Baseband
inline bool bb_valid(const Baseband& b) {
  return b.Q > 0 && b.Q <= kBbMaxQ && b.nsps % b.Q == 0 && b.hop > 0 && b.nsps % b.hop == 0;
}

// ---- sample loads ----------------------------------------------------------------------------------
template <typename InT>
__device__ __forceinline__ float bb_sample(const InT* x, int64_t i);
template <>
__device__ __forceinline__ float bb_sample<float>(const float* x, int64_t i) { return x[i]; }
template <>
__device__ __forceinline__ float bb_sample<int16_t>(const int16_t* x, int64_t i) {
  return (float)x[i] / 32767.0f;  // read_wave_file scaling, as the STFT applies it
}
// four consecutive samples in one load (float: 16 B, 4-byte aligned; int16: 8 B, 2-byte aligned)
template <typename InT>
__device__ __forceinline__ float4 bb_load4(const InT* p);
template <>
__device__ __forceinline__ float4 bb_load4<float>(const float* p) {
  float4 v;
  __builtin_memcpy(&v, p, sizeof(v));
  return v;
}
template <>
__device__ __forceinline__ float4 bb_load4<int16_t>(const int16_t* p) {
  short4 v;
  __builtin_memcpy(&v, p, sizeof(v));
  return make_float4((float)v.x / 32767.0f, (float)v.y / 32767.0f, (float)v.z / 32767.0f, (float)v.w / 32767.0f);
}

// exp(-2 pi i cyc) from the exact phase
__device__ __forceinline__ float2 bb_rot(double cyc) {
  float s, c;
  sincospif((float)(-2.0 * (cyc - floor(cyc))), &s, &c);
  return make_float2(c, s);
}

// t_i = exp(-2 pi i fmix i / fs), i < D; the caller's barrier orders it before bb_mix_down
__device__ __forceinline__ void bb_twiddles(float2* s_tw, int D, double fmix, double fs) {
  for (int i = threadIdx.x; i < D; i += kBbThreads) s_tw[i] = bb_rot(fmix * (double)i / fs);
}

// z[m] = w_m sum_i x[nb + m D + i] t_i over samples [nb + m D, nb + (m + 1) D), m < Mz, with t_i from
// s_tw and w_m = exp(-2 pi i fmix (nb + m D) / fs) from its exact phase: two fmas per sample, in
// ascending sample order on either path.  (Round 4 rotated a per-z phasor by one complex multiply per
// sample, ~20 VALU per sample with its per-sample range tests.)  A window inside the slot (all but the
// slot's edges) reads its samples four at a time, unchecked; else every sample is tested.
template <typename InT, int LD>
__device__ __forceinline__ void bb_mix_down(const InT* x, int64_t n_samples, int64_t nb, const BbGeom& g, double fmix,
                                            double fs, const float2* s_tw, float2* s_z) {
  const int D = g.D;
  const bool inside = nb >= 0 && nb + (int64_t)g.Mz * D <= n_samples;  // workgroup-uniform
#pragma unroll 1
  for (int m = threadIdx.x; m < g.Mz; m += kBbThreads) {
    const int64_t n0 = nb + (int64_t)m * D;
    const InT* xp = x + n0;
    float ax = 0.f, ay = 0.f;
    if (inside && (D & 3) == 0) {
      // LD loads of four samples are issued before the first is used: one load per trip left a lane's
      // L2 hits a full latency apart.  The fmas keep their order.  Past D a trip repeats the last
      // in-range load and does not use it.
      for (int i0 = 0; i0 < D; i0 += 4 * LD) {
        float4 v[LD];
#pragma unroll
        for (int u = 0; u < LD; ++u) v[u] = bb_load4<InT>(xp + min(i0 + 4 * u, D - 4));
#pragma unroll
        for (int u = 0; u < LD; ++u) {
          const int i = i0 + 4 * u;
          if (i < D) {
            const float4 t01 = *reinterpret_cast<const float4*>(s_tw + i);
            const float4 t23 = *reinterpret_cast<const float4*>(s_tw + i + 2);
            ax = fmaf(v[u].x, t01.x, ax);
            ay = fmaf(v[u].x, t01.y, ay);
            ax = fmaf(v[u].y, t01.z, ax);
            ay = fmaf(v[u].y, t01.w, ay);
            ax = fmaf(v[u].z, t23.x, ax);
            ay = fmaf(v[u].z, t23.y, ay);
            ax = fmaf(v[u].w, t23.z, ax);
            ay = fmaf(v[u].w, t23.w, ay);
          }
        }
      }
    } else {
      for (int i = 0; i < D; ++i) {
        const int64_t n = n0 + i;
        if (n >= 0 && n < n_samples) {
          const float v = bb_sample<InT>(xp, i);
          const float2 t = s_tw[i];
          ax = fmaf(v, t.x, ax);
          ay = fmaf(v, t.y, ay);
        }
      }
    }
    const float2 w = bb_rot(fmix * (double)n0 / fs);
    s_z[bb_z_at(g.Q, m)] = make_float2(ax * w.x - ay * w.y, ax * w.y + ay * w.x);
  }
}

}  // namespace ft8
