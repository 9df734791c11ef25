// ft4.hip -- the FT4 front end and transmit side on gfx950 (ft8hip.h, "FT4"; ft8_demodulator_amd/ft4.py
// restates every kernel here in NumPy).  Everything behind the LLRs -- k_bp, the selection kernels, the
// a-priori and OSD passes, k_compact, the message layer -- is the FT8 path's, unchanged.
//
// k_score4 / k_score4g  the sync score over the FT4 grid: ft8_sync_score with four 4-symbol sync groups at
//              symbols 0, 33, 66, 99 and four tones, the up-to-48 dB differences of a grid point added
//              SEQUENTIALLY in the contract's order (m, k, then tone-1, tone+1, time-1, time+1) in the
//              waterfall's dtype.  Both write what launch_score promises launch_select.
//              k_score4 (float32 waterfall, bins_per_tone = steps_per_symbol in 1..4) is built like
//              k_score2: a workgroup owns 128 grid columns x 22 grid rows of one residue class mod sps
//              and stages one sync band at a time in LDS -- (22 + 3) rows of stride sps x (128 + 3 bpt)
//              columns, 13 KB at bpt = sps = 2: the time neighbours of a group's symbols never leave the
//              group -- with band m + 1's loads in flight while band m is scored; a wave owns a row, a
//              lane two adjacent columns (packed float32 adds); bands wholly inside the waterfall are
//              straight-line code, edge bands keep the per-term tests; slots map to XCDs by id % 8.
//              k_score4g is the one-thread-per-grid-point form for float64 waterfalls and every other
//              oversampling (k_score's role): full grid, summaries by atomics.
// k_llr4       4-FSK LLRs of 87 data symbols, a wave per four candidates like k_llr: lane 4 g + i
//              fetches tone i of symbol 16 r + g in round r (six gathers per candidate, all issued
//              before the first is used), the powers reach their symbol through LDS, then the shared
//              normaliser (llr_shared.h).
// k_ft4_encode, k_ft4_synth, k_ft4_unscramble  the transmit chain of ft4_device.h and the descrambler.
#include <climits>

#include "ft4_device.h"
#include "llr_shared.h"
#include "score_shared.h"

namespace ft8 {
namespace {

constexpr int kScoreThreads = 256;
constexpr size_t kScoreLdsBudget = 64 * 1024;

struct Score4Args {
  const void* wf;
  int T, F, sps, bpt, num_blocks;
  int t0, NT, NF;
  int rlo, nrows;    // k_score4g: staged rows [rlo, rlo + nrows)
  void* scores;
  uint64_t* smask;   // [slot][NT][nseg][2] passing columns per 128-column segment
  int nseg;
  RowSummary* rowsum;
  double min_score;
  int cmp_f64;
  int n_slots, n_bands, n_ctiles;  // k_score4 grid
};

// ---- k_score4g: one thread per grid point --------------------------------------------------------
template <typename T, bool LDS, int TW>
__global__ __launch_bounds__(kScoreThreads) void k_score4g(Score4Args a) {
  FT8_RACE_PROLOGUE();
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  T* tile = reinterpret_cast<T*>(smem);
  const int slot = blockIdx.y;
  const int c0 = blockIdx.x * TW;
  const T* wf = reinterpret_cast<const T*>(a.wf) + (int64_t)slot * a.T * a.F;
  const int ncols = min(TW + 3 * a.bpt, a.F - c0);
  if constexpr (LDS) {
    const int n = a.nrows * ncols;
    for (int i = threadIdx.x; i < n; i += kScoreThreads) {
      const int r = i / ncols, c = i - r * ncols;
      tile[i] = wf[(int64_t)(a.rlo + r) * a.F + c0 + c];
    }
    __syncthreads();
  }
  auto get = [&](int row, int col) -> T {
    if constexpr (LDS) return tile[(row - a.rlo) * ncols + (col - c0)];
    else return wf[(int64_t)row * a.F + col];
  };
  const int lane_col = threadIdx.x % TW;
  const int rgroup = threadIdx.x / TW;
  constexpr int kGroups = kScoreThreads / TW;
  const int af = c0 + lane_col;
  T* out = reinterpret_cast<T*>(a.scores) + (int64_t)slot * a.NT * a.NF;
  RowSummary* rs = a.rowsum + (int64_t)slot * a.NT * a.nseg;
  const int sps = a.sps, bpt = a.bpt, nb = a.num_blocks;
  for (int ti = rgroup; ti < a.NT; ti += kGroups) {
    if (af >= a.NF) continue;
    const int at = a.t0 + ti;
    const int base = floordiv(at, sps);
    T score = (T)0;
    int n = 0;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int block = ft4::kSyncStride * m + k;
        const int ba = base + block;
        if (ba < 0 || ba >= nb) continue;
        const int tone = ft4::costas(m, k);
        const int row = at + block * sps;
        const int col = af + tone * bpt;
        const T p = get(row, col);
        if (tone > 0) { score += (T)(p - get(row, col - bpt)); n++; }
        if (tone < 3) { score += (T)(p - get(row, col + bpt)); n++; }
        if (k > 0 && ba > 0) { score += (T)(p - get(row - sps, col)); n++; }
        if (k < 3 && ba + 1 < nb) { score += (T)(p - get(row + sps, col)); n++; }
      }
    }
    T res;
    if (n == 0 || isnan(score) || isinf(score)) res = (T)-INFINITY;
    else res = score / (T)n;
    out[(int64_t)ti * a.NF + af] = res;
    if (passes(res, a.min_score, a.cmp_f64)) {
      RowSummary* e = rs + (int64_t)ti * a.nseg + af / kSegCols;
      atomicAdd(&e->count, 1u);
      atomicMax(&e->maxkey, order_key((double)res));
      const int c = af % kSegCols;
      atomicOr(reinterpret_cast<unsigned long long*>(
                   &a.smask[(((int64_t)slot * a.NT + ti) * a.nseg + af / kSegCols) * 2 + (c & 1)]),
               1ull << (c >> 1));
    }
  }
}

// ---- k_score4 --------------------------------------------------------------------------------------
constexpr int kS4TW = 128;                 // grid columns per workgroup (64 lanes x 2)
constexpr int kS4R = 22;                   // grid rows per workgroup (82 rows per class at 12 kHz: 4 tiles)
constexpr int kS4Waves = 8;                // row j of the workgroup on wave j % 8
constexpr int kS4Rows = (kS4R + kS4Waves - 1) / kS4Waves;  // rows per wave
constexpr int kS4Threads = kS4Waves * kWave;
constexpr int kS4Sym = 4;                  // symbols of a sync group

// A workgroup's 22 grid rows are one residue class mod sps, consecutive in it: abs_time a0 + sps j.
// Every waterfall row those grid points read for sync band m is a0 + 33 m sps + sps (j + k), k < 4: the
// time neighbours exist only inside the group (k > 0, k < 3), so the band's tile is 22 + 3 rows of stride sps.
template <int BPT, int SPS>
struct S4Geom {
  static constexpr int P = (kS4TW + 3 * BPT + 3) & ~3;   // staged columns (multiple of 4: float4 rows)
  static constexpr int H = kS4R + kS4Sym - 1;            // staged rows of one sync band
  static constexpr int kFloats = H * P;                  // the LDS tile: one band at a time
  static constexpr int Q = P / 4;                        // float4 per staged row
  static constexpr int kIter = (H * Q + kS4Threads - 1) / kS4Threads;  // float4 staged per thread
};

// The thread's part of the staging, computed once per workgroup: for each of its float4s the band-0 row
// (a sentinel far below 0 when the float4 lies past the tile or past column F) and its element offset
// row * F + col; band m adds 33 m SPS rows to both.
template <int BPT, int SPS>
struct S4Stage {
  int row0[S4Geom<BPT, SPS>::kIter];
  int off0[S4Geom<BPT, SPS>::kIter];
};
template <int BPT, int SPS>
__device__ __forceinline__ S4Stage<BPT, SPS> s4_stage(int F, int a0, int c0) {
  using G = S4Geom<BPT, SPS>;
  S4Stage<BPT, SPS> st;
#pragma unroll
  for (int it = 0; it < G::kIter; ++it) {
    const int idx = (int)threadIdx.x + it * kS4Threads;
    const int rw = idx / G::Q, q4 = idx - rw * G::Q;
    const int row = a0 + SPS * rw, col = c0 + 4 * q4;
    const bool ok = idx < G::H * G::Q && col < F;
    st.row0[it] = ok ? row : INT_MIN / 2;
    st.off0[it] = row * F + col;   // the tiled path takes slot waterfalls below 2^31 floats only
  }
  return st;
}
template <int BPT, int SPS>
__device__ __forceinline__ void s4_load(const float* wf, int T, int F, const S4Stage<BPT, SPS>& st, int m,
                                        float4 (&v)[S4Geom<BPT, SPS>::kIter]) {
  using G = S4Geom<BPT, SPS>;
  const int drow = ft4::kSyncStride * m * SPS;    // wave-uniform
  const float* wb = wf + (int64_t)drow * F;
#pragma unroll
  for (int it = 0; it < G::kIter; ++it) {
    const int row = st.row0[it] + drow;
    v[it] = make_float4(0.f, 0.f, 0.f, 0.f);
    if ((unsigned)row < (unsigned)T) v[it] = *reinterpret_cast<const float4*>(wb + st.off0[it]);
  }
}

// sync band M of one grid row: tb = the row's first tile row at the lane's columns, lo = the block of the
// band's first symbol
template <int BPT, int P, int M>
__device__ __forceinline__ void s4_band(const float* tb, int lo, int nb, f32x2& score, int& n) {
  if (lo >= 0 && lo <= nb - kS4Sym) {
    // every symbol of the band in range, and with it every neighbour: straight-line code (12 differences)
#pragma unroll
    for (int k = 0; k < kS4Sym; ++k) {
      const int tone = ft4::costas(M, k);
      const float* rp = tb + k * P + tone * BPT;
      const f32x2 pw = ld2<BPT>(rp);
      if (tone > 0) score += pw - ld2<BPT>(rp - BPT);
      if (tone < 3) score += pw - ld2<BPT>(rp + BPT);
      if (k > 0) score += pw - ld2<BPT>(rp - P);
      if (k < 3) score += pw - ld2<BPT>(rp + P);
    }
    n += 12;
  } else if (lo + kS4Sym - 1 >= 0 && lo < nb) {
    // a band crossing the waterfall's first or last block: the contract's per-term tests
#pragma unroll
    for (int k = 0; k < kS4Sym; ++k) {
      const int ba = lo + k;
      if (ba < 0 || ba >= nb) continue;
      const int tone = ft4::costas(M, k);
      const float* rp = tb + k * P + tone * BPT;
      const f32x2 pw = ld2<BPT>(rp);
      if (tone > 0) { score += pw - ld2<BPT>(rp - BPT); n++; }
      if (tone < 3) { score += pw - ld2<BPT>(rp + BPT); n++; }
      if (k > 0 && ba > 0) { score += pw - ld2<BPT>(rp - P); n++; }
      if (k < 3 && ba + 1 < nb) { score += pw - ld2<BPT>(rp + P); n++; }
    }
  }
}

template <int BPT, int SPS, bool COMPACT>
__global__ __launch_bounds__(kS4Threads) void k_score4(Score4Args a) {
  FT8_RACE_PROLOGUE();
  static_assert(kS4TW == kSegCols, "a workgroup's columns are one score segment");
  using G = S4Geom<BPT, SPS>;
  constexpr int P = G::P;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* tile = reinterpret_cast<float*>(smem);
  // workgroup -> (slot, row tile, column tile); slot % 8 == workgroup id % 8 keeps a slot on one XCD
  const int id = blockIdx.x;
  const int per = a.n_bands * a.n_ctiles;
  const int q = id >> 3;
  const int slot = (q / per) * 8 + (id & 7);
  if (slot >= a.n_slots) return;
  const int r = q % per;
  const int band = r / a.n_ctiles, ct = r - band * a.n_ctiles;
  // band -> (residue class of the grid rows mod SPS, 22-row tile of the class)
  const int nbpc = a.n_bands / SPS;
  const int cls = band / nbpc, i0 = (band - cls * nbpc) * kS4R;
  const int cnt = (a.NT - cls + SPS - 1) / SPS;   // grid rows of the class
  if (i0 >= cnt) return;                          // (workgroup-uniform)
  const int a0 = a.t0 + cls + SPS * i0;           // abs_time of the tile's first grid row
  const int c0 = ct * kS4TW;
  const float* wf = reinterpret_cast<const float*>(a.wf) + (int64_t)slot * a.T * a.F;
  const bool vec = (a.F & 3) == 0 && (reinterpret_cast<uintptr_t>(a.wf) & 15) == 0;

  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int af = c0 + 2 * lane;
  const int nb = a.num_blocks;
  const int rows = min(kS4R, cnt - i0);
  f32x2 score[kS4Rows];
  int n[kS4Rows];
#pragma unroll
  for (int u = 0; u < kS4Rows; ++u) {
    score[u] = f32x2{0.0f, 0.0f};
    n[u] = 0;
  }

  float4 v[G::kIter];
  const S4Stage<BPT, SPS> stg = s4_stage<BPT, SPS>(a.F, a0, c0);
  if (vec) s4_load<BPT, SPS>(wf, a.T, a.F, stg, 0, v);
  auto stage_band = [&](int m) {
    if (m > 0) __syncthreads();  // every wave has scored band m - 1
    if (vec) {
#pragma unroll
      for (int it = 0; it < G::kIter; ++it) {
        const int idx = (int)threadIdx.x + it * kS4Threads;
        if (idx < G::H * G::Q) reinterpret_cast<float4*>(tile)[idx] = v[it];
      }
      if (m < 3) s4_load<BPT, SPS>(wf, a.T, a.F, stg, m + 1, v);  // in flight while band m is scored
    } else {
      for (int i = threadIdx.x; i < G::kFloats; i += kS4Threads) {
        const int rr = i / P, cc = i - rr * P;
        const int row = a0 + ft4::kSyncStride * m * SPS + SPS * rr, col = c0 + cc;
        float x = 0.0f;
        if (row >= 0 && row < a.T && col < a.F) x = wf[(int64_t)row * a.F + col];
        tile[i] = x;
      }
    }
    __syncthreads();
  };
  const int lo0 = floordiv(a0, SPS);
  // the four bands differ in their tones, so each is its own straight-line code
  stage_band(0);
#pragma unroll
  for (int u = 0; u < kS4Rows; ++u) {
    const int j = w + u * kS4Waves;        // wave-uniform
    if (j < rows) s4_band<BPT, P, 0>(tile + j * P + 2 * lane, lo0 + j, nb, score[u], n[u]);
  }
  stage_band(1);
#pragma unroll
  for (int u = 0; u < kS4Rows; ++u) {
    const int j = w + u * kS4Waves;
    if (j < rows) s4_band<BPT, P, 1>(tile + j * P + 2 * lane, lo0 + j + ft4::kSyncStride, nb, score[u], n[u]);
  }
  stage_band(2);
#pragma unroll
  for (int u = 0; u < kS4Rows; ++u) {
    const int j = w + u * kS4Waves;
    if (j < rows) s4_band<BPT, P, 2>(tile + j * P + 2 * lane, lo0 + j + 2 * ft4::kSyncStride, nb, score[u], n[u]);
  }
  stage_band(3);
#pragma unroll
  for (int u = 0; u < kS4Rows; ++u) {
    const int j = w + u * kS4Waves;
    if (j < rows) s4_band<BPT, P, 3>(tile + j * P + 2 * lane, lo0 + j + 3 * ft4::kSyncStride, nb, score[u], n[u]);
  }

  float* out = reinterpret_cast<float*>(a.scores) + (COMPACT ? 0 : (int64_t)slot * a.NT * a.NF);
  RowSummary* rs = a.rowsum + (int64_t)slot * a.NT * a.nseg;
#pragma unroll
  for (int u = 0; u < kS4Rows; ++u) {
    const int j = w + u * kS4Waves;
    if (j >= rows) continue;
    float res[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const float sc = score[u][c];
      res[c] = (n[u] == 0 || isnan(sc) || isinf(sc)) ? -INFINITY : sc / (float)n[u];
    }
    const int ti = a0 + SPS * j - a.t0;
    const bool v0 = af < a.NF, v1 = af + 1 < a.NF;
    const bool p0 = v0 && passes(res[0], a.min_score, a.cmp_f64);
    const bool p1 = v1 && passes(res[1], a.min_score, a.cmp_f64);
    const uint64_t b0 = __ballot(p0), b1 = __ballot(p1);
    const int64_t seg = ((int64_t)slot * a.NT + ti) * a.nseg + ct;
    if (COMPACT) {
      // the passing scores of the segment, in column order, packed at its start (k_score2's layout)
      const uint64_t below = (1ull << lane) - 1ull;
      const int r0 = __popcll(b0 & below) + __popcll(b1 & below);
      float* sv = out + seg * kSegCols;
      if (p0) sv[r0] = res[0];
      if (p1) sv[r0 + (p0 ? 1 : 0)] = res[1];
    } else {
      float* orow = out + (int64_t)ti * a.NF;
      if (v0) orow[af] = res[0];
      if (v1) orow[af + 1] = res[1];
    }
    if (lane == 0) *reinterpret_cast<ulonglong2*>(a.smask + 2 * seg) = make_ulonglong2(b0, b1);
    // the (row, segment) summary: this wave is the segment's only writer, so a plain store
    const unsigned pc = (unsigned)(__popcll(b0) + __popcll(b1));
    unsigned long long key = 0ull;
    if (pc) {
      float mx = p0 ? res[0] : -INFINITY;
      if (p1) mx = fmaxf(mx, res[1]);
      mx = wave_max(mx);
      key = order_key((double)mx);
    }
    if (lane == 0) {
      RowSummary e;
      e.count = pc;
      e.pad = 0;
      e.maxkey = key;
      rs[seg - (int64_t)slot * a.NT * a.nseg] = e;
    }
  }
}

template <int BPT, int SPS, bool COMPACT>
hipError_t launch_score4_tiled(const SyncLaunch& L, const Score4Args& a0, hipStream_t s) {
  using G = S4Geom<BPT, SPS>;
  Score4Args a = a0;
  // SPS residue classes of the grid rows, each cut into 22-row tiles (a tile past its class's rows exits
  // at once)
  a.n_bands = SPS * ((((L.NT + SPS - 1) / SPS) + kS4R - 1) / kS4R);
  a.n_ctiles = (L.NF + kS4TW - 1) / kS4TW;
  const size_t lds = sizeof(float) * G::kFloats;
  static_assert(sizeof(float) * S4Geom<4, 4>::kFloats <= 64 * 1024, "one band fits the default LDS limit");
  const int groups = (L.n_slots + 7) / 8;
  const int64_t blocks = (int64_t)groups * 8 * a.n_bands * a.n_ctiles;
  return lds_launch(k_score4<BPT, SPS, COMPACT>, dim3((unsigned)blocks), dim3(kS4Threads), lds, s, a);
}
template <int B>
hipError_t launch_score4_any(const SyncLaunch& L, const Score4Args& a, hipStream_t s) {
  return score_compact(L) ? launch_score4_tiled<B, B, true>(L, a, s) : launch_score4_tiled<B, B, false>(L, a, s);
}

template <typename T, int TW>
hipError_t launch_score4_t(const SyncLaunch& L, hipStream_t s) {
  Score4Args a{};
  a.wf = L.wf;
  a.T = L.T;
  a.F = L.F;
  a.sps = L.sps;
  a.bpt = L.bpt;
  a.num_blocks = L.T / L.sps;
  a.t0 = L.t0;
  a.NT = L.NT;
  a.NF = L.NF;
  a.scores = L.scores;
  a.smask = L.smask;
  a.nseg = n_segments(L.NF);
  a.rowsum = L.rowsum;
  a.min_score = L.min_score;
  a.cmp_f64 = L.min_score_f64;
  a.n_slots = L.n_slots;
  if constexpr (sizeof(T) == 4) {
    if (score4_path(L)) {
      switch (L.bpt) {
        case 1: return launch_score4_any<1>(L, a, s);
        case 2: return launch_score4_any<2>(L, a, s);
        case 3: return launch_score4_any<3>(L, a, s);
        case 4: return launch_score4_any<4>(L, a, s);
        default: break;
      }
    }
  }
  // k_score4g sets the mask bits and the (row, segment) summaries of its passing grid points one by one
  hipError_t e = hipMemsetAsync(L.smask, 0, sizeof(uint64_t) * 2 * (size_t)L.n_slots * L.NT * a.nseg, s);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(L.rowsum, 0, sizeof(RowSummary) * (size_t)L.n_slots * L.NT * a.nseg, s);
  if (e != hipSuccess) return e;
  // rows the grid touches: [0, num_blocks * sps) at most, clipped to what the grid's frames reach
  a.rlo = max(0, L.t0);
  const int rhi = min(L.T - 1, L.t0 + L.NT - 1 + (ft4::kSymbols - 1) * L.sps);
  a.nrows = rhi - a.rlo + 1;
  const int ncols = TW + 3 * L.bpt;
  const size_t lds = (size_t)a.nrows * ncols * sizeof(T);
  dim3 grid((L.NF + TW - 1) / TW, L.n_slots);
  if (lds <= kScoreLdsBudget)
    hipLaunchKernelGGL((k_score4g<T, true, TW>), grid, dim3(kScoreThreads), lds, s, a);
  else
    hipLaunchKernelGGL((k_score4g<T, false, TW>), grid, dim3(kScoreThreads), 0, s, a);
  return hipGetLastError();
}

// ---- k_llr4 ------------------------------------------------------------------------------------------
struct Llr4Args {
  const void* wf;
  int T, F, sps, bpt, num_blocks;
  const int32_t* cand;         // mode 0: [n_slots][N][2] + cand_count; mode 1: [n][3] (slot, t, f)
  const int32_t* cand_count;
  int N, n_items, mode, n_slots;
  int normalize;
  double* llr_out;             // [n_items][174]
};
constexpr int kL4Rounds = 6;                       // 16 symbols per round
constexpr int kL4Stage = 16 * kL4Rounds * 4;       // staged powers per candidate
static_assert(16 * kL4Rounds >= ft4::kDataSymbols && 2 * ft4::kDataSymbols == FT8_LDPC_N, "87 symbols, 174 bits");

// modes: 0 per-slot candidate lists (4 consecutive ranks of one slot per wave; ranks >= the slot's count
// skipped), 1 explicit (slot, t, f) list.  A bin outside [0, F) reads as 0 (grid candidates have none).
template <typename T>
__global__ __launch_bounds__(kWave) void k_llr4(Llr4Args a) {
  __shared__ double c[kLlrCpw][kLlrRow];
  __shared__ double part[kLlrCpw][16];
  __shared__ double bc[kLlrCpw];
  // the gather stage and the squared deviations share one buffer: a barrier separates the two uses
  constexpr size_t kScratch = sizeof(T) * kLlrCpw * kL4Stage > sizeof(double) * kLlrCpw * kLlrRow
                                  ? sizeof(T) * kLlrCpw * kL4Stage : sizeof(double) * kLlrCpw * kLlrRow;
  __shared__ __attribute__((aligned(16))) unsigned char scratch[kScratch];
  double (*sq)[kLlrRow] = reinterpret_cast<double (*)[kLlrRow]>(scratch);
  T (*stage)[kL4Stage] = reinterpret_cast<T (*)[kL4Stage]>(scratch);
  const int lane = threadIdx.x;
  const int id = blockIdx.x;
  int item0, n_on;
  int slot[kLlrCpw] = {0, 0, 0, 0}, at[kLlrCpw] = {0, 0, 0, 0}, af[kLlrCpw] = {0, 0, 0, 0};
  static_assert(kLlrCpw == 4, "four candidates per wave");
  if (a.mode == 0) {
    // workgroup id -> (slot, group of 4 ranks) with slot % 8 == id % 8: a slot's candidates on one XCD
    const int groups = (a.N + kLlrCpw - 1) / kLlrCpw;
    const int q = id >> 3;
    const int s0 = (q / groups) * 8 + (id & 7);
    const int c0 = (q % groups) * kLlrCpw;
    if (s0 >= a.n_slots) return;
    n_on = min(kLlrCpw, min(a.N, a.cand_count[s0]) - c0);
    item0 = s0 * a.N + c0;
#pragma unroll
    for (int u = 0; u < kLlrCpw; ++u) {
      slot[u] = s0;
      if (u < n_on) {
        at[u] = a.cand[((int64_t)item0 + u) * 2];
        af[u] = a.cand[((int64_t)item0 + u) * 2 + 1];
      }
    }
  } else {
    item0 = id * kLlrCpw;
    n_on = min(kLlrCpw, a.n_items - item0);
#pragma unroll
    for (int u = 0; u < kLlrCpw; ++u) {
      if (u < n_on) {
        slot[u] = a.cand[((int64_t)item0 + u) * 3];
        at[u] = a.cand[((int64_t)item0 + u) * 3 + 1];
        af[u] = a.cand[((int64_t)item0 + u) * 3 + 2];
      }
    }
  }
  if (n_on <= 0) return;  // wave-uniform

  {  // the gathers: lane 4 g + i fetches tone i of data symbol 16 r + g
    const int i = lane & 3, g = lane >> 2;
    const T* wf0 = reinterpret_cast<const T*>(a.wf);
    T v[kLlrCpw][kL4Rounds];
#pragma unroll
    for (int u = 0; u < kLlrCpw; ++u) {
      const int base = floordiv(at[u], a.sps);
      const T* wf = wf0 + (int64_t)slot[u] * a.T * a.F;
      const int col = af[u] + i * a.bpt;
#pragma unroll
      for (int r = 0; r < kL4Rounds; ++r) {
        const int k = 16 * r + g;
        const int sym = ft4::data_symbol(k);
        const int block = base + sym;
        v[u][r] = (T)0;
        if (u < n_on && k < ft4::kDataSymbols && block >= 0 && block < a.num_blocks && (unsigned)col < (unsigned)a.F)
          v[u][r] = wf[(int64_t)(at[u] + sym * a.sps) * a.F + col];
      }
    }
#pragma unroll
    for (int u = 0; u < kLlrCpw; ++u)
#pragma unroll
      for (int r = 0; r < kL4Rounds; ++r) stage[u][4 * (16 * r + g) + i] = v[u][r];
  }
  __syncthreads();
  for (int k = lane; k < ft4::kDataSymbols; k += kWave) {
    const int sym = ft4::data_symbol(k);
#pragma unroll
    for (int u = 0; u < kLlrCpw; ++u) {
      if (u >= n_on) break;
      const int block = floordiv(at[u], a.sps) + sym;
      double l0 = 0.0, l1 = 0.0;
      if (block >= 0 && block < a.num_blocks) {
        double s[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] = (double)stage[u][4 * k + ft4::gray(j)];
        l0 = pymax2(s[2], s[3]) - pymax2(s[0], s[1]);
        l1 = pymax2(s[1], s[3]) - pymax2(s[0], s[2]);
      }
      c[u][2 * k] = l0;
      c[u][2 * k + 1] = l1;
    }
  }
  __syncthreads();
  if (a.normalize) {  // ftx_normalize_logl, the wave's candidates side by side (k_llr's sequence)
    const double mean = pairwise174x4(c, part, lane) / 174.0;
    if ((lane & 15) == 0) bc[lane >> 4] = mean;
    __syncthreads();
    for (int e = lane; e < n_on * FT8_LDPC_N; e += kWave) {
      const int u = e / FT8_LDPC_N, n = e - u * FT8_LDPC_N;
      const double d = c[u][n] - bc[u];
      sq[u][n] = d * d;
    }
    __syncthreads();
    const double var = pairwise174x4(sq, part, lane) / 174.0;
    if ((lane & 15) == 0) bc[lane >> 4] = sqrt_rn(24.0 / var);
    __syncthreads();
    for (int e = lane; e < n_on * FT8_LDPC_N; e += kWave) {
      const int u = e / FT8_LDPC_N, n = e - u * FT8_LDPC_N;
      a.llr_out[(int64_t)(item0 + u) * FT8_LDPC_N + n] = c[u][n] * bc[u];
    }
    return;
  }
  for (int e = lane; e < n_on * FT8_LDPC_N; e += kWave) {
    const int u = e / FT8_LDPC_N, n = e - u * FT8_LDPC_N;
    a.llr_out[(int64_t)(item0 + u) * FT8_LDPC_N + n] = c[u][n];
  }
}

// ---- descrambler, encoder, synthesis -------------------------------------------------------------------
__global__ void k_ft4_unscramble(ft8_result* res, int n, const int32_t* counts, int cap) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (counts && i % cap >= counts[i / cap]) return;   // a row past its slot's count
#pragma unroll
  for (int b = 0; b < 10; ++b) res[i].payload[b] ^= ft4::kRvecD[b];   // byte 9 of rvec ends in three 0 bits
}

__global__ void k_ft4_encode(const uint8_t* msg, int n, uint8_t* a91, uint8_t* cw, uint8_t* tones) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  ft4::encode(msg + (int64_t)i * 10, a91 ? a91 + (int64_t)i * 12 : nullptr, cw ? cw + (int64_t)i * 22 : nullptr,
              tones ? tones + (int64_t)i * ft4::kSymbols : nullptr);
}

constexpr int kSynThreads = 256;
constexpr int kSynPer = 8;
constexpr int kSynTile = kSynThreads * kSynPer;

// first index in [0, n) whose slot is >= s (signals sorted by slot)
__device__ int lower_slot(const ft8_tx_signal* sig, int n, int s) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (sig[mid].slot < s) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// k_synth's shape: one workgroup per (slot, tile of kSynTile samples), every overlapping signal of the
// slot evaluated sample-parallel and added to the output once, in array order
template <bool CPLX, typename OT, typename AT>
__global__ __launch_bounds__(kSynThreads) void k_ft4_synth(SynthLaunch a) {
  FT8_RACE_PROLOGUE();
  __shared__ int s_E[ft4::kSymbols];
  __shared__ int s_PS[ft4::kSymbols + 1];
  __shared__ int s_range[2];
  const int slot = blockIdx.y;
  const int64_t t0 = (int64_t)blockIdx.x * kSynTile;
  if (threadIdx.x == 0) {
    s_range[0] = lower_slot(a.sig, a.n_sig, slot);
    s_range[1] = lower_slot(a.sig, a.n_sig, slot + 1);
  }
  __syncthreads();
  const int lo = s_range[0], hi = s_range[1];
  const int nsps = a.nsps, L = ft4::kWaveSymbols * nsps;
  const double spacing = a.fs / (double)nsps;
  AT re[kSynPer], im[kSynPer];
#pragma unroll
  for (int k = 0; k < kSynPer; ++k) re[k] = im[k] = (AT)0;
  for (int i = lo; i < hi; ++i) {
    const ft8_tx_signal sg = a.sig[i];
    const int64_t w0 = sg.start - nsps;   // the ramp-up symbol comes before symbol 0
    if (w0 >= t0 + kSynTile || w0 + L <= t0) continue;  // uniform
    __syncthreads();
    const uint8_t* tn = a.tones + (int64_t)i * ft4::kSymbols;
    if (threadIdx.x < ft4::kSymbols) s_E[threadIdx.x] = tn[threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0) {
      int acc = 0;
      for (int k = 0; k <= ft4::kSymbols; ++k) {
        s_PS[k] = acc;
        if (k < ft4::kSymbols) acc += s_E[k];
      }
    }
    __syncthreads();
    const double inv_fs = 1.0 / a.fs;
#pragma unroll
    for (int k = 0; k < kSynPer; ++k) {
      const int64_t nabs = t0 + threadIdx.x + (int64_t)k * kSynThreads;
      const int64_t n64 = nabs - w0;
      if (n64 < 0 || n64 >= L || nabs >= a.n_samples) continue;
      const int n = (int)n64;
      const double G = ft4::gfsk_G(s_E, s_PS, a.P, nsps, n);
      const double cyc = (sg.f0 * (double)n + spacing * G) * inv_fs;
      const double fr = cyc - floor(cyc);
      const AT r = ft4::ramp<AT>(n, L, nsps) * (AT)sg.amplitude;
      const AT psi = (AT)(2.0 * M_PI) * (AT)fr + (AT)sg.phase;
      AT sn, cs;
      if constexpr (sizeof(AT) == 8) sincos(psi, &sn, &cs);
      else sincosf(psi, &sn, &cs);
      re[k] += r * sn;
      if constexpr (CPLX) im[k] -= r * cs;
    }
  }
  OT* out = (OT*)a.out;
#pragma unroll
  for (int k = 0; k < kSynPer; ++k) {
    const int64_t nabs = t0 + threadIdx.x + (int64_t)k * kSynThreads;
    if (nabs >= a.n_samples) continue;
    const int64_t o = (int64_t)slot * a.slot_stride + nabs;
    if constexpr (CPLX) {
      out[2 * o] = (OT)((AT)out[2 * o] + re[k]);
      out[2 * o + 1] = (OT)((AT)out[2 * o + 1] + im[k]);
    } else {
      out[o] = (OT)((AT)out[o] + re[k]);
    }
  }
}

}  // namespace

// the tiled kernel: float32, bpt = sps in 1..4, a slot waterfall its 32-bit element offsets reach
bool score4_path(const SyncLaunch& L) {
  return !L.wf_f64 && L.bpt == L.sps && L.bpt >= 1 && L.bpt <= 4 && (int64_t)L.T * L.F < (1ll << 31);
}

hipError_t launch_score4(const SyncLaunch& L, hipStream_t s) {
  if (L.NT <= 0 || L.NF <= 0 || L.n_slots <= 0) return hipSuccess;
  if (L.wf_f64) return launch_score4_t<double, 32>(L, s);
  return launch_score4_t<float, 64>(L, s);
}

hipError_t launch_llr4(const BpLaunch& L, hipStream_t s) {
  if (L.n_items <= 0) return hipSuccess;
  if (L.mode != 0 && L.mode != 1) return hipErrorInvalidValue;
  Llr4Args a{};
  a.wf = L.wf;
  a.T = L.T;
  a.F = L.F;
  a.sps = L.sps;
  a.bpt = L.bpt;
  a.num_blocks = L.sps > 0 ? L.T / L.sps : 0;
  a.cand = L.cand;
  a.cand_count = L.cand_count;
  a.N = L.N;
  a.n_items = L.n_items;
  a.mode = L.mode;
  a.n_slots = L.n_slots;
  a.normalize = L.normalize;
  a.llr_out = L.llr_out;
  const int64_t grid = L.mode == 0 ? (int64_t)((L.n_slots + 7) / 8) * 8 * ((L.N + kLlrCpw - 1) / kLlrCpw)
                                   : ((int64_t)L.n_items + kLlrCpw - 1) / kLlrCpw;
  if (L.wf_f64)
    hipLaunchKernelGGL(k_llr4<double>, dim3((unsigned)grid), dim3(kWave), 0, s, a);
  else
    hipLaunchKernelGGL(k_llr4<float>, dim3((unsigned)grid), dim3(kWave), 0, s, a);
  hipError_t e = hipGetLastError();
  // the deferred order of equal scores k_llr replays beside its own workgroups
  if (e == hipSuccess && L.mode == 0 && L.tie)
    e = launch_tie_order(TieArgs{L.n_slots, L.N, L.cand_count, L.warn, L.tie, L.cand_score}, s);
  return e;
}

hipError_t launch_ft4_unscramble(ft8_result* res, int n, const int32_t* counts, int cap, hipStream_t s) {
  if (n <= 0 || (counts && cap <= 0)) return hipSuccess;
  hipLaunchKernelGGL(k_ft4_unscramble, dim3((n + 255) / 256), dim3(256), 0, s, res, n, counts, cap);
  return hipGetLastError();
}

hipError_t launch_ft4_encode(const uint8_t* msg, int n, uint8_t* a91, uint8_t* cw, uint8_t* tones, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_ft4_encode, dim3((n + 127) / 128), dim3(128), 0, s, msg, n, a91, cw, tones);
  return hipGetLastError();
}

hipError_t launch_ft4_synth(const SynthLaunch& a, hipStream_t s) {
  if (a.n_slots <= 0 || a.n_samples <= 0) return hipSuccess;
  dim3 grid((unsigned)((a.n_samples + kSynTile - 1) / kSynTile), (unsigned)a.n_slots);
  switch (a.dtype) {
    case FT8_F32: hipLaunchKernelGGL((k_ft4_synth<false, float, float>), grid, dim3(kSynThreads), 0, s, a); break;
    case FT8_F64: hipLaunchKernelGGL((k_ft4_synth<false, double, double>), grid, dim3(kSynThreads), 0, s, a); break;
    case FT8_C64: hipLaunchKernelGGL((k_ft4_synth<true, float, float>), grid, dim3(kSynThreads), 0, s, a); break;
    case FT8_C128: hipLaunchKernelGGL((k_ft4_synth<true, double, double>), grid, dim3(kSynThreads), 0, s, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace ft8
