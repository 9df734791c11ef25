// ft8_internal.h -- shared device helpers and the internal launch interface between the
// kernel translation units (stft.hip, sync.hip, bp.hip) and the C-ABI (capi.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <stdint.h>
#include <utility>

#include "../../include/ft8hip.h"
#include "ft8_ldpc_tables.h"

namespace ft8 {

constexpr int kWave = 64;

// ---- barrier-race check build (-DFT8_RACE_CHECK; tools/build_race.sh, never the shipped library) --
// FT8_RACE_PROLOGUE() opens every kernel whose workgroup has more than one wave and uses LDS: the
// whole LDS allocation of the workgroup (static + dynamic: the dispatch packet's
// group_segment_size) is filled with 0xffffffff (a NaN / -1 sentinel), a barrier, then one wave of
// the workgroup (rotating with the workgroup id) sleeps ~64 k cycles before it starts.  A read of
// another wave's LDS staging that no barrier orders after the write then sees the sentinel instead
// of a late value, deterministically, and the GPU tests fail.
// tools/probe/race_control.hip is the positive control: a kernel with a deliberately missing
// barrier that must read the sentinel under this prologue (tests/test_gpu_race_control.py).
#ifdef FT8_RACE_CHECK
}  // namespace ft8
#include <hsa/hsa.h>
namespace ft8 {
static_assert(offsetof(hsa_kernel_dispatch_packet_t, group_segment_size) == 28, "dispatch packet layout");
__device__ __forceinline__ void race_prologue() {
  const auto* pkt = (const hsa_kernel_dispatch_packet_t*)__builtin_amdgcn_dispatch_ptr();
  const uint32_t bytes = pkt->group_segment_size;  // static + dynamic LDS of this workgroup
  const uint32_t nt = blockDim.x * blockDim.y * blockDim.z;
  const uint32_t t = threadIdx.x + blockDim.x * (threadIdx.y + blockDim.y * threadIdx.z);
  for (uint32_t off = 4 * t; off + 4 <= bytes; off += 4 * nt)
    asm volatile("ds_write_b32 %0, %1" ::"v"(off), "v"(0xffffffffu) : "memory");
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __syncthreads();
  const uint32_t nw = (nt + kWave - 1) / kWave;
  // the test must be wave-uniform in an SGPR: s_sleep is a scalar instruction that the EXEC mask
  // does not gate, so under a per-lane condition (an exec-masked block the compiler does not branch
  // around) every wave slept and none was late -- the positive control caught it
  const uint32_t w = __builtin_amdgcn_readfirstlane(t / kWave);
  if (nw > 1 && w == blockIdx.x % nw)
    for (int i = 0; i < 8; ++i) __builtin_amdgcn_s_sleep(127);
  // a compiler barrier: s_sleep carries no memory semantics, so the kernel's first LDS accesses
  // must not be scheduled above it
  asm volatile("" ::: "memory");
}
#define FT8_RACE_PROLOGUE() ::ft8::race_prologue()
#else
#define FT8_RACE_PROLOGUE() \
  do {                      \
  } while (0)
#endif
constexpr int kMaxCandidates = 4096;   // LDS-resident selection (k_select)
// LDS FFT limits (one (P + P/16 + 1)-point buffer per frame, 256 threads holding P / 256 values each
// per stage): float32 P <= 10240 (87 KB), float64 P <= 8192 (139 KB).  Larger or non-2/3/5/7 lengths
// take the chirp-z transform (its power-of-two convolution on the same LDS FFT), or the direct DFT
// where that convolution would not fit.
constexpr int kMaxFftReal = 20480;     // float32 nfft of the real-input path (half-length FFT <= 10240)
constexpr int kMaxFftComplex = 10240;  // float32 nfft of the complex-input path
constexpr int kMaxFftP64 = 8192;       // float64: FFT points P (real nfft <= 16384, complex <= 8192)
constexpr int kMaxDft = 1 << 18;       // nfft of the direct-DFT fallback (any factorisation)
constexpr int kMaxDftLds = 150 * 1024; // its windowed frame is staged in LDS

__host__ __device__ inline int floordiv(int a, int b) {
  int q = a / b;
  if ((a % b) != 0 && ((a < 0) != (b < 0))) q--;
  return q;
}

template <typename T>
struct cplx {
  T x, y;
};

// ---- LDS opt-in (defined in capi.hip) --------------------------------------------------------
// A launch whose static + dynamic LDS exceeds the default 64 KB needs the kernel's
// MaxDynamicSharedMemorySize attribute raised first.  lds_opt_in returns at once, with no runtime
// call, when `kernel`'s static LDS (queried once) plus dyn_bytes fits the default or when that
// kernel already holds a grant of at least dyn_bytes on the current device; else it raises the
// attribute and records the grant.  The state is keyed by (kernel address, device): kernels of one
// pointer type (the six subtraction kernels are all void(*)(SubLaunch)) never share a grant.
hipError_t lds_opt_in(const void* kernel, size_t dyn_bytes);
// opt in, launch, report
template <typename... P, typename... A>
hipError_t lds_launch(void (*kern)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t s, A&&... args) {
  const hipError_t e = lds_opt_in(reinterpret_cast<const void*>(kern), lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, grid, block, lds, s, std::forward<A>(args)...);
  return hipGetLastError();
}

// ---- STFT plan (host-built tables, device-resident) ----------------------------------------
struct FftPlan {
  int P;              // transform length (nfft/2 for real input, nfft for complex input; nfft if dft;
                      // the convolution length M if blue)
  int dft;            // 1: direct DFT (tw = W_nfft^m): lengths neither the Stockham plans nor the
                      // chirp-z path take (nperseg above its LDS limit)
  int blue;           // 1: chirp-z (Bluestein) transform, for an nfft with a prime factor above 7 or an
                      // odd real nfft: every nfft-point DFT of a frame is a length-P (power of two)
                      // circular convolution, run on the LDS Stockham FFT (stft.hip k_stft_blue)
  int nstages;
  int radix[16];
  const void* tw;     // W_P^m, m in [0, P): cplx<float> or cplx<double>
  const void* post;   // real path: W_N^k, k in [0, P]  (N = 2P)
  // chirp-z (blue): the output bins of a frame are computed in blocks of B = P - nperseg + 1
  int L, B, nblk;     // nperseg the plan is built for, bins per block, blocks covering [0, nfft)
  const void* chirp;  // exp(-i pi k^2 / nfft), k in [0, nfft)
  const void* hspec;  // [nblk][P]: FFT_P of block b's chirp filter conj(chirp(b B + m - (L - 1)))
};
constexpr int kMaxBlueP64 = 8192;       // chirp-z convolution length limits (the LDS FFT's)
constexpr int kMaxBlueP32 = 8192;

struct StftLaunch {
  const void* samples;
  int dtype;               // ft8_dtype
  int64_t n_samples, slot_stride;
  int n_slots;
  int nperseg, hop, nfft;
  int t_lo, t_hi, f_lo, f_hi;
  const void* window;      // float or double [nperseg]
  double scale;            // 1 / (sum w)^2
  void* out;               // float or double [n_slots][t_hi-t_lo][f_hi-f_lo]
  int32_t* argmax;         // non-null: write per-frame argmax over the kept bins instead of `out`
                           // (a direct-DFT plan then writes the dB rows to `out` first)
  int32_t* screen_list;    // non-null (complex128 argmax, 3840-point geometry): float32 screening
  int32_t* screen_count;   // with the uncertain frames listed here and redone in float64
  const void* screen_tw;     // the screening pass's float32 twiddles (W_3840^m) and window
  const void* screen_window;
  FftPlan plan;
};
hipError_t launch_stft(const StftLaunch& a, hipStream_t s);
// complex input in the beacon receiver's geometry (nfft 3840, nperseg 1920, hop 240 M): k_stftc3840
// (stft.hip); a complex128 argmax request in it is screened in float32 first
bool stftc3840_eligible(const StftLaunch& a);
// the production geometry (real float32 / int16 input, nfft 3840, nperseg 1920, hop 960) with packed
// float32 complex arithmetic (stft3840.hip)
bool stft3840_eligible(const StftLaunch& a);
hipError_t launch_stft3840(const StftLaunch& a, hipStream_t s);
bool stftpk_eligible(const StftLaunch& a);        // stft3840.hip: the packed generic real-input plans
hipError_t launch_stftpk(const StftLaunch& a, hipStream_t s);
// the static plans k_stft_sp (stft.hip) and k_stft_pk (stft3840.hip) are built for, {P, radices...}:
// the reference's other real-input geometries (20 kHz, 12 kHz at bpt 10, 6 kHz)
struct StaticPlan {
  int P, n, r[4];
};
constexpr StaticPlan kStaticPlans[] = {{3200, 4, {16, 8, 5, 5}}, {9600, 4, {16, 8, 15, 5}}, {960, 3, {16, 4, 15}}};
// index of the static plan with this factorisation, or -1
inline int static_plan_of(int P, int nstages, const int* radix) {
  for (int q = 0; q < 3; ++q) {
    const StaticPlan& p = kStaticPlans[q];
    bool ok = P == p.P && nstages == p.n;
    for (int i = 0; ok && i < p.n; ++i) ok = radix[i] == p.r[i];
    if (ok) return q;
  }
  return -1;
}

// ---- sync score + selection ----------------------------------------------------------------
// Per (slot, time row) summary written by k_score for k_select: how many grid points of the row
// pass the min_score test, and the largest passing score as an order-preserving key (0 = none).
struct RowSummary {
  unsigned count;
  unsigned pad;
  unsigned long long maxkey;
};
static_assert(sizeof(RowSummary) == 16 && offsetof(RowSummary, maxkey) == 8, "k_select reads it as one uint4");
__host__ __device__ inline unsigned long long order_key(double v) {
  union { double d; unsigned long long u; } x{v};
  return (x.u >> 63) ? ~x.u : (x.u | 0x8000000000000000ull);
}
__host__ __device__ inline double key_value(unsigned long long k) {
  union { double d; unsigned long long u; } x;
  x.u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return x.d;
}

// ft8_find_candidates' admission test (ft8_decode.py:127): not -inf and not below min_score, the
// comparison done in the score's dtype unless min_score is a float64 scalar
template <typename T>
__device__ __forceinline__ bool passes(T s, double ms, int cmp_f64) {
  if (s == (T)-INFINITY) return false;
  if (cmp_f64) return !((double)s < ms);
  return !(s < (T)ms);
}

struct SyncLaunch {
  int protocol = FT8_PROTO_FT8;  // FT8_PROTO_FT4: the FT4 score kernels (ft4.hip) on the FT4 grid
  const void* wf;          // [n_slots][T][F]
  int wf_f64;
  int n_slots, T, F;
  int sps, bpt;
  int t0, NT, NF;          // abs_time grid = [t0, t0+NT), abs_freq grid = [0, NF)
  void* scores;            // full grid [n_slots][NT][NF] in wf dtype, or (compact) the passing
                           // scores of every segment packed at its start [n_slots][NT][nseg][128]
  uint64_t* smask;         // [n_slots][NT][nseg][2]: passing columns of each 128-column segment
                           // (word 0: even columns 2l -> bit l, word 1: odd columns 2l + 1)
  int compact = 0;         // request the compact score layout (honoured by the k_score2 path)
  int N;                   // max candidates
  double min_score;
  int min_score_f64;
  int32_t* cand;           // [n_slots][N][2]
  double* cand_score;      // [n_slots][N]
  int32_t* cand_count;     // [n_slots]
  int32_t* warn;           // scratch [n_slots] (bit 0: tie reached a heap comparison,
                           //                    bit 2: equal scores in the selected set,
                           //                    bit 3: their order deferred to the LLR kernel)
  RowSummary* rowsum;      // scratch [n_slots][NT][n_segments(NF)]: passing count + max passing score
                           // per (time row, 128-column segment)
  int32_t* tie = nullptr;  // nullable scratch [n_slots][tie_stride(N)]: defer the order of equal
                           // scores to the LLR kernel (warn bit 3); k_compact applies it
  int topk = 0;            // FT8_FLAG_TOPK: k_topk instead of the reference heap selection
};

// deferred tie order, per slot: push order [N] | select order [N] | final order [N] |
// scratch [4N] | last record [1] | its score [1] (float bits) | scores in push order [N]
// (heap_replay.h)
inline __host__ __device__ int64_t tie_stride(int N) { return 8 * (int64_t)N + 2; }
struct TieArgs {
  int n_slots, N;
  const int32_t* cand_count;
  int32_t* warn;           // bit 3 set by k_select: replay this slot's heap; bit 0 set on a tie
  int32_t* tie;            // [n_slots][tie_stride(N)]
  const double* cand_score;  // [n_slots][N] selected scores in select order (float32 values)
};
// the deferred order applied to a candidate list ([n_slots][N][2] + [n_slots][N])
hipError_t launch_tie_apply(const TieArgs& a, int32_t* cand, double* cand_score, hipStream_t s);
hipError_t launch_score(const SyncLaunch& a, hipStream_t s);
// score segments: 128 grid columns of one row; the compact layout holds only passing scores
constexpr int kSegCols = 128;
inline __host__ __device__ int n_segments(int NF) { return (NF + kSegCols - 1) / kSegCols; }
// whether launch_score writes the compact layout for this launch (else the full grid)
bool score_compact(const SyncLaunch& a);
hipError_t launch_select(const SyncLaunch& a, hipStream_t s);
// FT4 (ft4.hip): launch_score's work for protocol FT8_PROTO_FT4 -- the same promises to launch_select (the
// full grid or the compact segments, the masks, the summaries); score4_path: whether the tiled kernel
// k_score4 takes the launch (the only one that writes the compact layout), else k_score4g
bool score4_path(const SyncLaunch& a);
hipError_t launch_score4(const SyncLaunch& a, hipStream_t s);
// ft8_sync_score for arbitrary candidates [n][2] = (abs_time, abs_freq); err[i] = 1: IndexError
hipError_t launch_score_list(const void* wf, int wf_f64, int T, int F, int sps, int bpt, const int32_t* cand,
                             int n, void* out, int32_t* err, hipStream_t s);

// ---- LLR + BP + CRC ------------------------------------------------------------------------
// k_bp's work / clock counters: kStatRows rows of kStatStride u64 (one 128-B line each); wave w adds
// to row w % kStatRows and the host sums the rows.  One row for all 4 096 waves put every retiring
// wave's atomics on the same L2 addresses, where they serialise at the launch's tail.
constexpr int kStatRows = 256;
constexpr int kStatStride = 16;   // [0..3] work counters, [4..7] clock (BpLaunch.stats / .clock)
struct BpLaunch {
  // LLR source: either a waterfall + candidate list, or precomputed LLRs
  const void* wf;          // [n_slots][T][F] or null
  int wf_f64, T, F, sps, bpt;
  const int32_t* cand;     // mode A: [n_slots][N][2] + cand_count; mode B: [n][3] (slot, t, f)
  const double* cand_score;
  const int32_t* cand_count;
  int N;                   // per-slot capacity (mode A)
  int n_slots;
  int n_items;             // mode B item count, or n_slots*N in mode A
  int mode;                // 0: waterfall+per-slot candidates, 1: waterfall+explicit list,
                           // 2: LLR input (k_llr: normalise only; k_bp: no candidate metadata)
  const double* llr_in;    // k_bp: always; k_llr: mode 2
  int normalize;           // k_llr only
  int max_iterations;
  double* llr_out;         // k_llr output [n_items][174]
  uint8_t* plain_out;      // nullable [n_items][174]
  ft8_result* res;         // nullable [n_items]
  // k_bp claim counter: 64-bit, never reset.  Launch j claims tickets [base_j, base_j + n_items +
  // waves): every item once, then one ticket >= n_items per wave, so the host advances the base
  // (*work_base, host memory, one per counter) by n_items + waves at each launch -- no reset, no
  // retire counter, nothing a launch cut short could leave behind for the next one to skip over
  unsigned long long* work;
  unsigned long long* work_base;
  unsigned long long* stats = nullptr;  // [candidates, iterations entered, message passes, converged]
  unsigned long long* clock = nullptr;  // timed launches: [wave cycles, wave wall ticks, max wave cycles, waves]
  int slot0 = 0;           // batch index of slot 0 (records carry slot0 + local slot)
  int grid_waves = 4;      // k_bp persistent grid: resident waves per SIMD (clamped to 4)
  int f32 = 0;             // 1: the float32 decoder k_bp32 (bp32.hip) runs this launch (run_bp)
  // mode 0, nullable: slots whose order of equal scores k_select deferred (warn bit 3) get it
  // replayed by k_llr's first workgroups
  int32_t* tie = nullptr;  // [n_slots][tie_stride(N)]
  int32_t* warn = nullptr; // [n_slots]
};
hipError_t launch_llr(const BpLaunch& a, hipStream_t s);  // k_llr: waterfall -> LLRs
hipError_t launch_bp(const BpLaunch& a, hipStream_t s);   // k_bp: LLRs -> BP + CRC
// k_bp32 (bp32.hip): launch_bp's modes 0 and 2 in IEEE binary32, two candidates per wave.  The same host
// protocol on the same counters, but a claim takes two tickets: the launch advances *work_base by
// 2 (ceil(n_items / 2) + waves).
hipError_t launch_bp32(const BpLaunch& a, hipStream_t s);
// the kernel the launch names (BpLaunch.f32)
inline hipError_t run_bp(const BpLaunch& a, hipStream_t s) { return a.f32 ? launch_bp32(a, s) : launch_bp(a, s); }
// FT4 (ft4.hip): k_llr4, launch_llr's modes 0 and 1 with the FT4 symbol layout.  It does not run the
// deferred tie order of mode 0 beside its workgroups: launch_tie_order (bp.hip, one wave per slot) does.
hipError_t launch_llr4(const BpLaunch& a, hipStream_t s);
hipError_t launch_tie_order(const TieArgs& a, hipStream_t s);
// FT4: rvec XORed onto the 77 payload bits of n records in place; with counts, res is [n / cap][cap] and
// only the rows below min(counts[slot], cap) are touched
hipError_t launch_ft4_unscramble(ft8_result* res, int n, const int32_t* counts, int cap, hipStream_t s);

struct CompactLaunch {
  const ft8_result* res;   // [n_slots][N]
  const int32_t* cand_count;
  int n_slots, N;
  ft8_result* out;         // [n_slots][cap]
  int32_t* counts;
  int cap;
  const int32_t* warn = nullptr;  // with tie: slots with warn bit 3 are read in the final order
  const int32_t* tie = nullptr;
};
hipError_t launch_compact(const CompactLaunch& a, hipStream_t s);

// ---- the samples and geometry k_sub_est and k_coherent mix down from (baseband.h; capi.hip baseband_setup)
struct Baseband {
  const void* x;               // samples [n_slots][slot_stride], F32 or I16
  int dtype;
  int64_t n_samples, slot_stride;
  int n_slots;
  double fs;
  int nsps, hop, nfft, t_lo, f_lo;
  int Q;                       // decimated samples per symbol (nsps % Q == 0)
};

// ---- retry pass: the failed candidates of a chunk, tried again (ap.hip, coherent.hip, osd.hip) -----
// The four retries of ft8_decode_batch (coherent, a-priori on the coherent LLRs, a-priori, OSD, in that
// order) take the records plain BP left with ok == 0.  launch_retry_list lists them per slot in candidate
// order; the coherent and the AP pass build new LLRs for the list positions and launch_bp runs in mode 0
// over the compacted lists (cand / score / count as its candidate lists); the stage on the coherent LLRs
// lists attempts on that pass's positions (CohApLaunch) and decodes them the same way; OSD decodes the
// listed records' own LLRs in k_osd.  Every pass accepts an attempt through retry_accept and nowhere else.
struct RetryLists {
  ft8_result* res;             // in / out [n_slots][N]: the records plain BP wrote
  const int32_t* cand_count;   // [n_slots], null: every slot holds N records
  const int32_t* cand_in;      // nullable [n_slots][N][2] and [n_slots][N]: the candidates' positions and
  const double* score_in;      // scores (copied to the compacted lists; zeros without them)
  const double* gate;          // nullable [n_slots][N]: only candidates with gate != 0 are listed
  int n_slots, N, M;           // M <= N: list positions per slot
  int32_t* list;               // [n_slots][M] original indices of the listed candidates
  int32_t* count;              // [n_slots] their number
  int32_t* cand;               // compacted [n_slots][M][2]
  double* score;               // compacted [n_slots][M]
};
__device__ inline int slot_count(const RetryLists& r, int slot) {
  return r.cand_count ? min(r.N, r.cand_count[slot]) : r.N;
}
// k_retry_list, one wave per slot: the first M candidates c < slot_count with !res.ok (and gate != 0),
// in candidate order; count = min(found, M)
hipError_t launch_retry_list(const RetryLists& r, hipStream_t s);
// an accepted attempt `got` rewrites the record it retried; pass_bits: (h + 1) << 4 for AP hypothesis
// h, 2 for the coherent pass (6 at a drift rate other than 0, and 8 more from a multi-symbol set), both
// for hypothesis h on the coherent LLRs, 0xF0 for OSD
__device__ inline void retry_accept(ft8_result* rec, const ft8_result& got, int pass_bits) {
  ft8_result w = *rec;
  w.ok = 1;
  for (int i = 0; i < 10; ++i) w.payload[i] = got.payload[i];
  w.crc_extracted = got.crc_extracted;
  w.crc_calculated = got.crc_calculated;
  w.ldpc_errors = got.ldpc_errors;
  w.pass_index = (uint8_t)(w.pass_index | pass_bits);
  *rec = w;
}

// ---- a-priori decoding (ap.hip) ----------------------------------------------------------------
// The AP retry (ft8hip.h, "a-priori decoding"): k_ap_amax once (amax is the lists' gate), then per
// hypothesis the list, k_ap_clamp -> llr_h, launch_bp -> plain and res_h, k_ap_merge.
struct ApLaunch {
  RetryLists r;                // M == N: k_ap_clamp and k_ap_merge index the lists with the records' stride
                               // (launch_ap_clamp / launch_ap_merge: hipErrorInvalidValue otherwise)
  const double* llr;           // [n_slots][N][174] the LLRs plain BP consumed
  ft8_ap_hyp hyp;              // the hypothesis of this attempt, by value
  int h, max_hard;
  double* amax;                // [n_slots][N] a = 1.01 max |L| of a candidate, 0 where it is not to be retried
  double* llr_h;               // compacted, clamped LLRs
  const uint8_t* plain;        // launch_bp's hard decisions of the compacted lists
  const ft8_result* res_h;     // launch_bp's records of them
  int16_t* hard;               // nullable [n_slots * N], by original index: hard_h of an accepted attempt
};
hipError_t launch_ap_amax(const ApLaunch& a, hipStream_t s);
hipError_t launch_ap_clamp(const ApLaunch& a, hipStream_t s);
hipError_t launch_ap_merge(const ApLaunch& a, hipStream_t s);

// ---- coherent re-demodulation (coherent.hip) ---------------------------------------------------
// k_coherent over a candidate list (ft8hip.h, "coherent re-demodulation"): either an explicit list
// (slot_of non-null: n candidates, workgroup = list position) or per-slot lists [n_slots][M] with
// count[n_slots] entries each (a slot's positions on one XCD).
struct CohLaunch {
  Baseband b;
  const int32_t* cand;         // [positions][2] = (abs_time, abs_freq)
  const int32_t* slot_of;      // explicit list: [n]; null: per-slot lists
  const int32_t* count;        // per-slot lists: [n_slots]
  int n, M;
  double* llr;                 // [positions][174]
  ft8_coh_fit* fit;            // [positions]
};
// the drift search (ft8hip.h, step 1b): on when n_rates > 1 and max_rate > 0.  Its kernels are
// instantiations of their own and take this as a second argument; k_coherent's argument stays CohLaunch.
struct CohDrift {
  float max_rate;              // Hz/s
  int n_rates;                 // odd, <= 33
  ft8_coh_drift* out;          // nullable [positions]
};
inline bool coherent_drift_on(const CohDrift& g) { return g.n_rates > 1 && g.max_rate > 0.f; }
// the multi-symbol sets (ft8hip.h, step 4b): on when nsym > 1.  Like the drift search, instantiations of
// their own with this as a further argument: set s (0-based) of position pos is written at
// llr + pos * pos_stride + s * set_stride (in doubles), so the stage call's [n][S][174] and the pass's
// one [positions][174] per set are both reached.
struct CohMulti {
  int nsym;                    // S: sets per position, 2 or 3
  int64_t pos_stride, set_stride;
  uint8_t* valid;              // nullable [positions]: bit s for a valid set s
};
inline bool coherent_multi_on(const CohMulti& m) { return m.nsym > 1; }
size_t coherent_lds_bytes(int nsps, int Q, bool multi);   // k_coherent's dynamic LDS
hipError_t launch_coherent(const CohLaunch& a, const CohDrift& g, const CohMulti& m, hipStream_t s);
// valid[i] = fit[i].status == 0: the validity bytes where only set 1 exists
hipError_t launch_coh_valid1(const ft8_coh_fit* fit, uint8_t* valid, int n, hipStream_t s);
// The coherent retry inside ft8_decode_batch: the list (M = the per-slot cap), k_coherent -> fit and
// the LLRs, then per set launch_bp -> res_c and k_coh_merge.
struct CohPass {
  RetryLists r;
  const ft8_coh_fit* fit;      // k_coherent's fits of the lists
  const ft8_result* res_c;     // launch_bp's records of them
  const ft8_coh_drift* drift;  // null without the drift search: the winning rates of the lists
  const uint8_t* valid;        // null with one set: k_coherent's validity bytes of the lists
  int set;                     // the set (0-based) res_c was decoded from
};
hipError_t launch_coh_merge(const CohPass& a, hipStream_t s);

// ---- a-priori retries on the coherent LLRs (ap.hip; ft8hip.h, "coherent_ap") -------------------
// The stage after the coherent pass's last merge, on the list that pass built: positions [n_slots][M],
// S LLR sets per position (set n of position pos at llr + pos * pos_stride + n * set_stride, in
// doubles), H hypotheses.  Attempt (j, h, n) of a slot has the index (j * H + h) * S + n, which is the
// contract's order within a position; a slot's usable attempts are compacted in that order into lists
// of stride A = M * H * S, which k_bp decodes in one launch (mode 0, `att` as its candidate lists).
struct CohApLaunch {
  ft8_result* res;             // in / out [n_slots][N]: the records as the coherent pass left them
  int n_slots, N, M, H, S;
  const int32_t* list;         // [n_slots][M] original indices of the positions; null: position j is record j
  const int32_t* count;        // [n_slots] positions per slot; null: M
  const int32_t* cand;         // nullable, compacted [n_slots][M][2] and [n_slots][M]: the positions'
  const double* score;         // candidates and scores (copied to the attempts; zeros without them)
  const ft8_coh_fit* fit;      // nullable [n_slots][M]: only positions with status 0 are tried
  const ft8_coh_drift* drift;  // nullable [n_slots][M]: a rate other than 0 sets bit 2
  const uint8_t* valid;        // nullable [n_slots][M]: set n is tried only where bit n is set
  const double* llr;           // the coherent LLRs
  int64_t pos_stride, set_stride;
  ft8_ap_hyp hyp[FT8_AP_MAX_HYP];
  int max_hard;
  double* amax;                // [n_slots][M][S] a_n = 1.01 max |L_n|, 0 where (position, set) is not tried
  RetryLists att;              // the attempts: N = M = A; list holds the attempt index; res is unused
  int32_t* where;              // [n_slots][A] attempt index -> its place in the slot's list, -1: not listed
  double* llr_a;               // [n_slots][A][174] clamped LLRs of the listed attempts
  const uint8_t* plain;        // launch_bp's hard decisions of them
  const ft8_result* res_a;     // launch_bp's records of them
  int16_t* hard;               // nullable [n_slots * N], by original index: hard errors of an accepted attempt
};
hipError_t launch_cohap_amax(const CohApLaunch& a, hipStream_t s);
hipError_t launch_cohap_list(const CohApLaunch& a, hipStream_t s);
hipError_t launch_cohap_clamp(const CohApLaunch& a, hipStream_t s);
hipError_t launch_cohap_merge(const CohApLaunch& a, hipStream_t s);

// ---- ordered-statistics decoding (osd.hip; ft8hip.h, "ordered-statistics decoding") ------------
// k_osd, one workgroup per list position: positions [n_slots][M] over records [n_slots][N].  The stage
// call has one list of every record (list and count null: position j is record j, and a record that is
// ok already gets status 3); the pass inside ft8_decode_batch gives launch_retry_list's lists.
struct OsdLaunch {
  ft8_result* res;             // in / out [n_slots][N]
  const double* llr;           // [n_slots][N][174] the LLRs plain BP consumed
  int n_slots, N, M;
  const int32_t* list;         // [n_slots][M] original indices of the positions; null: position j is record j
  const int32_t* count;        // [n_slots] positions per slot; null: M
  int order, max_hard;
  ft8_osd_rec* info;           // nullable [n_slots * N], by original index
  uint8_t* codeword;           // nullable [n_slots * N][22], by original index
};
hipError_t launch_osd(const OsdLaunch& a, hipStream_t s);

// ft8_pack_decodes (bp.hip): one workgroup packs a batch's decodes for the all-gather
inline __host__ __device__ int64_t pack_header_bytes(int n_slots) { return 8 + ((4 * (int64_t)n_slots + 7) & ~7ll); }
hipError_t launch_pack(const ft8_result* rec, const int32_t* counts, int n_slots, int cap, int capacity,
                       int slot_offset, uint8_t* send, ft8_result* overflow, hipStream_t s);

// ft8_unpack77 (msg.hip): records [n_slots][cap] -> text records, one workgroup per slot
hipError_t launch_unpack77(const ft8_result* rec, const int32_t* counts, int n_slots, int cap, ft8_text* out,
                           hipStream_t s);

// ---- signal report (snr.hip) -------------------------------------------------------------------
// k_noise_floor: colmean[n_slots][F] = the time mean of every column's linear power; k_noise_rank:
// floor_out[n_slots] = its element of rank `rank` sorted ascending (NaNs last), one workgroup per slot
hipError_t launch_noise_floor(const void* wf, int wf_f64, int n_slots, int T, int F, int rank, double* floor_out,
                              double* colmean, hipStream_t s);
// k_snr: records [n_slots][cap] -> reports, one wave per record; bw_db = 10 log10(enbw_hz / 2500)
hipError_t launch_snr(const void* wf, int wf_f64, int n_slots, int T, int F, int sps, int bpt, const ft8_result* rec,
                      const int32_t* counts, int cap, const double* floor_in, int radius, double bw_db,
                      ft8_snr_rec* out, hipStream_t s);

// ---- transmit chain + subtraction (tx.hip, subtract.hip) -------------------------------------
struct SynthLaunch {
  const uint8_t* tones;        // [n_sig][79]
  const ft8_tx_signal* sig;    // [n_sig], sorted by slot
  int n_sig;
  int nsps, style;
  double fs;
  const double* P;             // cumulative GFSK pulse [3 nsps + 1]
  void* out;                   // [n_slots][slot_stride] of dtype (complex: pairs)
  int dtype;
  int64_t n_samples, slot_stride;
  int n_slots;
};
hipError_t launch_encode(const uint8_t* msg, int msg_bytes, int n, uint8_t* a91, uint8_t* cw, uint8_t* tones,
                         hipStream_t s);
hipError_t launch_synth(const SynthLaunch& a, hipStream_t s);
// FT4 (ft4.hip, ft4_device.h): payloads [n][10] -> a91 / codeword / tones [n][103]; the waveforms of
// SynthLaunch with tones [n_sig][103], P the BT = 1.0 pulse table and style unused
hipError_t launch_ft4_encode(const uint8_t* msg, int n, uint8_t* a91, uint8_t* cw, uint8_t* tones, hipStream_t s);
hipError_t launch_ft4_synth(const SynthLaunch& a, hipStream_t s);

struct SubLaunch {
  Baseband b;
  float* residual;             // [n_slots][slot_stride]
  const ft8_result* res;       // [n_slots][cap] decoded records
  const int32_t* counts;       // [n_slots]
  int cap;
  const double* P;             // cumulative GFSK pulse [3 nsps + 1] (double)
  const float* Pf;             // the same in float
  void* est;                   // scratch [n_slots * cap] SubEst records
  int32_t* list;               // scratch [n_slots][cap + 1]: the records to fit (ok, first of their
                               // payload in the slot), in record order, then their count
  const int32_t* first;        // null, or the slot's first row at first[slot * first_stride]: the rows
  int first_stride;            // before it are neither fitted nor seen (an accumulated list's earlier passes)
};
size_t sub_est_bytes();        // sizeof one SubEst record
hipError_t launch_sub_est(const SubLaunch& a, hipStream_t s);    // fits of the records (k_sub_est)
hipError_t launch_sub_apply(const SubLaunch& a, hipStream_t s);  // residual = x - fitted signals

// out[slot] = the accumulated records out1[slot][0 .. counts1) followed by this pass's records
// out2[slot][0 .. counts2) whose payload no accumulated record carries (pass_index |= 1); counts
// uncapped.  out == out1 (cap == cap1, counts == counts1) appends in place.  pass_counts (nullable)
// [n_slots][n_passes]: column pass - 2 receives counts1, column pass - 1 the new count.
hipError_t launch_merge_pass(ft8_result* out, int32_t* counts, int cap, const ft8_result* out1,
                             const int32_t* counts1, int cap1, const ft8_result* out2, const int32_t* counts2,
                             int cap2, int n_slots, int32_t* pass_counts, int n_passes, int pass, hipStream_t s);

// ---- frequency-drift correction (drift.hip) ---------------------------------------------------
struct DriftFitLaunch {
  const int32_t* idx;          // [n_slots][T] per-frame argmax (kept-bin index)
  int n_slots, T, F;
  ft8_drift_params p;
  ft8_drift_result* res;       // [n_slots]
  double* metric;              // [n_slots][T - window + 1] or null
  int32_t* segments;           // [n_slots][max_segments][2] or null
  int max_segments;
  const double* tmpl;          // stage 2: three_sync_correlation_seq [n_tmpl]
  int n_tmpl;
};
constexpr int kDriftMaxT = 16384;   // frames per signal held in LDS by the fit kernels
hipError_t launch_drift_fit(int stage, const DriftFitLaunch& a, hipStream_t s);

struct DerotateLaunch {
  const void* x;               // stage 1: input samples (dtype), row stride slot_stride
  int dtype;
  int64_t slot_stride;
  double* out;                 // complex128 [n_slots][n_samples] (interleaved re, im)
  int64_t n_samples;
  int n_slots;
  const ft8_drift_result* res;
  double fs, inv_fs, inv_2fs2; // fs, fl(1/fs), fl(1/(2 fs^2)) (NumPy divides complex by real via 1/d)
};
// stage 1: out = x * exp(-2 pi i rate1 n^2 / (2 fs^2))  (x itself for FT8_DRIFT_NO_SEGMENT)
hipError_t launch_derotate1(const DerotateLaunch& a, hipStream_t s);
// stage 2: out *= the polynomial carrier of degree deg (1 or 2) where the status is FT8_DRIFT_FULL
hipError_t launch_derotate2(const DerotateLaunch& a, int deg, hipStream_t s);
int drift_max_template();      // LDS capacity of k_drift_fit2: template length, regression points
int drift_max_points();
constexpr int kDriftMaxWindow = 64;  // continuity window (exact int64 sums)

hipError_t launch_crc14(const uint8_t* msg, const int32_t* nbits, int n, uint16_t* crc, hipStream_t s);
hipError_t launch_ldpc_check(const uint8_t* bits, int n, int32_t* err, hipStream_t s);

}  // namespace ft8
