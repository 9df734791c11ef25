// capi.hip -- host side of libft8hip.so: context, STFT plans, scratch, launches, C-ABI.
//
// See include/ft8hip.h for the contract.  Everything below runs on the host; all numerical work is
// in the kernels of stft.hip / sync.hip / bp.hip.  No path here computes a decode on the CPU.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "ft8_internal.h"

#ifndef FT8_BUILD_ID
#define FT8_BUILD_ID "unversioned"
#endif
#ifndef FT8_BUILD_FLAGS
#define FT8_BUILD_FLAGS ""
#endif

using namespace ft8;

namespace {

// a device allocation and its owner: move-only, freed with its holder (a context's are freed under
// the context's DeviceGuard, ft8_destroy)
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) {
    o.p = nullptr;
    o.cap = 0;
  }
  DevBuf& operator=(DevBuf&& o) noexcept {
    std::swap(p, o.p);
    std::swap(cap, o.cap);
    return *this;
  }
  ~DevBuf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  template <typename T>
  T* as() const { return static_cast<T*>(p); }
};

struct PlanEntry {
  int nfft;
  bool cplx;   // complex-input path (P = nfft) vs real-input half-length path (P = nfft/2)
  bool f64;
  int L = 0;   // nperseg (chirp-z plans are built for one)
  FftPlan plan;  // its table pointers are views into the buffers below
  DevBuf tw, post, chirp, hspec;
};

struct WinEntry {
  int L;
  bool f64;
  DevBuf w;
  double scale;
};

// per-stage timing slots (ft8_get_timing, ft8_replay_stage), in the order of the binding's STAGE_NAMES
enum Stage {
  kStft, kScore, kSelect, kBp, kCompact, kDecodeBatch, kLlr, kSubEst, kDriftStftArgmax, kDriftFit, kDriftDerotate,
  kSubApply, kNStages
};
static_assert(kNStages == FT8_N_STAGES, "the stage ids are the public timing slots");

struct TimedLaunch {
  int stage;
  hipEvent_t a, b;
};

}  // namespace

// ---- LDS opt-in (ft8_internal.h) -----------------------------------------------------------------
namespace ft8 {
hipError_t lds_opt_in(const void* kernel, size_t dyn_bytes) {
  constexpr size_t kDefaultLds = 64 * 1024;
  struct KernelLds {
    size_t static_lds = 0;          // a property of the code object (one architecture): queried once
    std::map<int, size_t> granted;  // device -> dynamic bytes granted there
  };
  static std::mutex mu;
  static std::map<const void*, KernelLds> kernels;
  std::lock_guard<std::mutex> lk(mu);
  auto it = kernels.find(kernel);
  if (it == kernels.end()) {
    hipFuncAttributes fa{};
    const bool ok = hipFuncGetAttributes(&fa, kernel) == hipSuccess;
    if (!ok) (void)hipGetLastError();
    it = kernels.emplace(kernel, KernelLds{ok ? fa.sharedSizeBytes : 0, {}}).first;
  }
  if (it->second.static_lds + dyn_bytes <= kDefaultLds) return hipSuccess;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  size_t& granted = it->second.granted[dev];
  if (dyn_bytes <= granted) return hipSuccess;
  e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn_bytes);
  if (e == hipSuccess) granted = dyn_bytes;
  return e;
}
}  // namespace ft8

namespace {
int ensure(ft8_ctx* c, DevBuf& b, size_t bytes);  // grow-only scratch, below
int fail(ft8_ctx* c, int code, const std::string& msg);
}
// ---- the retry passes' settings and scratch (ft8_internal.h, "retry pass") -------------------------
// Each pass of ft8_decode_batch owns one struct below: its settings (ft8_set_*), its scratch, `ensure`
// (the scratch for n_slots lists; ft8hip.h states the sizes) and `at` (every pointer of the chunk that
// starts at slot `slot0`, offset there and nowhere else, so the chunks of a pipelined batch share none).
//
// What the passes have in common (RetryLists): the lists and, per list position, `sets` LLR vectors and
// records for k_bp, set-major (the coherent pass's multi-symbol sets; 0: the pass decodes without k_bp).
// at: `in` is the chunk's records and candidates (everything but M and the list arrays).
struct RetryView {
  RetryLists lists;
  double* llr;
  ft8_result* res;
};
struct RetryScratch {
  DevBuf list, count, cand, score, llr, res;
  int M = 0;
  size_t n_all = 0;  // list positions of all chunks: the distance between two sets' LLRs and records
  int ensure(ft8_ctx* c, size_t n_slots, int M_, int sets = 1) {
    const size_t n = n_slots * (size_t)M_;
    M = M_;
    n_all = n;
    int rc;
    if ((rc = ::ensure(c, list, sizeof(int32_t) * n))) return rc;
    if ((rc = ::ensure(c, count, sizeof(int32_t) * n_slots))) return rc;
    if ((rc = ::ensure(c, cand, sizeof(int32_t) * 2 * n))) return rc;
    if ((rc = ::ensure(c, score, sizeof(double) * n)) || sets == 0) return rc;
    if ((rc = ::ensure(c, llr, sizeof(double) * FT8_LDPC_N * n * sets))) return rc;
    return ::ensure(c, res, sizeof(ft8_result) * n * sets);
  }
  RetryView at(RetryLists in, int slot0) const {
    const size_t r0 = (size_t)slot0 * M;
    in.M = M;
    in.list = list.as<int32_t>() + r0;
    in.count = count.as<int32_t>() + slot0;
    in.cand = cand.as<int32_t>() + 2 * r0;
    in.score = score.as<double>() + r0;
    return {in, llr.p ? llr.as<double>() + (size_t)FT8_LDPC_N * r0 : nullptr, res.p ? res.as<ft8_result>() + r0 : nullptr};
  }
};

// a-priori decoding (ft8_set_ap): the hypotheses and the hard-error limit; lists of M = N, amax per
// record, plain per list position
struct ApRetry {
  std::vector<ft8_ap_hyp> hyps;
  int max_hard = FT8_LDPC_N;
  RetryScratch lists;
  DevBuf amax, plain;
  struct View : RetryView { double* amax; uint8_t* plain; };
  int ensure(ft8_ctx* c, size_t n_slots, int N) {
    int rc = lists.ensure(c, n_slots, N);
    if (!rc) rc = ::ensure(c, amax, sizeof(double) * n_slots * N);
    if (!rc) rc = ::ensure(c, plain, (size_t)FT8_LDPC_N * n_slots * N);
    return rc;
  }
  View at(const RetryLists& in, int slot0) const {
    const size_t r0 = (size_t)slot0 * lists.M;
    return {lists.at(in, slot0), amax.as<double>() + r0, plain.as<uint8_t>() + (size_t)FT8_LDPC_N * r0};
  }
};

// coherent re-demodulation (ft8_set_coherent, _drift, _nsym): the per-slot cap (0: every failed
// candidate), the drift search (off: 0, 1) and the set count (off: 1); lists of the cap with nsym sets,
// and per list position a fit, the winning rate (drift search only) and the validity byte (nsym > 1 only)
struct CoherentRetry {
  int max = 0, drift_n = 1, nsym = 1;
  float drift_rate = 0.f;
  RetryScratch lists;
  DevBuf fit, drift, valid;
  struct View : RetryView {  // llr / res: set 0; set n is n * set_stride doubles / n * n_all records further
    ft8_coh_fit* fit;
    ft8_coh_drift* drift;  // null without the drift search
    uint8_t* valid;        // null with one set
    int nsym;
    size_t n_all;
    int64_t set_stride;
  };
  bool drift_on() const { return coherent_drift_on(CohDrift{drift_rate, drift_n, nullptr}); }
  int cap(int N) const { return max > 0 ? std::min(max, N) : N; }  // listed candidates per slot
  int ensure(ft8_ctx* c, size_t n_slots, int N) {
    const int M = cap(N);
    int rc = lists.ensure(c, n_slots, M, nsym);
    if (!rc) rc = ::ensure(c, fit, sizeof(ft8_coh_fit) * n_slots * M);
    if (!rc && nsym > 1) rc = ::ensure(c, valid, n_slots * M);
    if (!rc && drift_on()) rc = ::ensure(c, drift, sizeof(ft8_coh_drift) * n_slots * M);
    return rc;
  }
  View at(const RetryLists& in, int slot0) const {
    const size_t r0 = (size_t)slot0 * lists.M;
    return {lists.at(in, slot0), fit.as<ft8_coh_fit>() + r0, drift_on() ? drift.as<ft8_coh_drift>() + r0 : nullptr,
            nsym > 1 ? valid.as<uint8_t>() + r0 : nullptr, nsym, lists.n_all, (int64_t)(FT8_LDPC_N * lists.n_all)};
  }
};

// a-priori retries on the coherent LLRs (ft8_set_coherent_ap; off: 0): lists of A = M * H * S attempts
// per slot; a per (position, set), the place of every attempt, plain per attempt
struct CoherentApRetry {
  int on = 0;
  RetryScratch lists;
  DevBuf amax, where, plain;
  struct View : RetryView { double* amax; int32_t* where; uint8_t* plain; };
  // FT8_E_RANGE where the attempts do not fit k_bp's 32-bit item count
  int ensure(ft8_ctx* c, size_t n_slots, int M, int H, int S) {
    const uint64_t A = (uint64_t)M * (uint64_t)H * (uint64_t)S;
    if (A * n_slots > (uint64_t)INT32_MAX)
      return fail(c, FT8_E_RANGE, "coherent a-priori retries: more than 2^31 - 1 attempts");
    int rc = lists.ensure(c, n_slots, (int)A);
    if (!rc) rc = ::ensure(c, amax, sizeof(double) * n_slots * M * S);
    if (!rc) rc = ::ensure(c, where, sizeof(int32_t) * n_slots * A);
    if (!rc) rc = ::ensure(c, plain, (size_t)FT8_LDPC_N * n_slots * A);
    return rc;
  }
  // the attempts of n_slots lists of M positions with S sets
  View at(int n_slots, int M, int S, int slot0) const {
    RetryLists in{};
    in.n_slots = n_slots;
    in.N = lists.M;
    const size_t a0 = (size_t)slot0 * lists.M;
    return {lists.at(in, slot0), amax.as<double>() + (size_t)slot0 * M * S, where.as<int32_t>() + a0,
            plain.as<uint8_t>() + (size_t)FT8_LDPC_N * a0};
  }
};

// ordered-statistics decoding (ft8_set_osd): the order, the per-slot cap (0: every failed candidate) and
// the hard-error limit; lists of the cap, no LLRs or records of its own
struct OsdRetry {
  int order = 2, max = 0, max_hard = 36;
  RetryScratch lists;
  int cap(int N) const { return max > 0 ? std::min(max, N) : N; }
  int ensure(ft8_ctx* c, size_t n_slots, int N) { return lists.ensure(c, n_slots, cap(N), 0); }
  RetryLists at(const RetryLists& in, int slot0) const { return lists.at(in, slot0).lists; }
};

struct ft8_ctx {
  int device = 0;
  std::string err;
  std::vector<PlanEntry> plans;
  std::vector<WinEntry> wins;
  DevBuf wf, scores, smask, cand, cand_score, cand_count, warn, rowsum, res_all, work, stats, llr, tie;
  // first ticket of the next k_bp launch per claim counter in `work` (8 B each, indexed by
  // bp_counter); reset with the buffer, which is zeroed whenever it is (re)allocated
  std::vector<unsigned long long> work_base;
  // FT8_FLAG_SUBTRACT: residual samples, per-record fits, the accumulated records (pass 1's, then what
  // every pass but the last appended) / the current pass's records
  DevBuf residual, sub_est, sub_list, out1, counts1, out2, counts2;
  // ft8_set_subtract: passes of an FT8_FLAG_SUBTRACT batch and whether each runs the AP / coherent retries
  int sub_passes = 2, sub_retry = 0;
  // ft8_subtract_counts: [n_slots][n_passes] row counts after each pass of the last FT8_FLAG_SUBTRACT batch,
  // and that batch's shape (-1: the last batch was none, or had nothing to search)
  DevBuf sub_pass_counts;
  int subc_slots = -1, subc_passes = -1;
  DevBuf screen;  // complex128 argmax STFT: [count][frames] uncertain-frame list (stft.hip)
  int64_t screen_frames = 0;  // frames of the last screened call (0: the last call was not screened)
  int sub_slots = 0, sub_cap = 0;  // shape of the fits in sub_est (ft8_subtract_fits)
  // cumulative GFSK pulse of the transmit chain for one nsps (double and float)
  int gfsk_nsps = 0;
  double gfsk_bt = 0.0;  // with gfsk_nsps the key of the tables below (FT8: 2.0, FT4: 1.0)
  DevBuf gfsk_P, gfsk_Pf;
  // frequency-drift correction: per-frame argmax, three-Costas correlation template (cached per
  // steps_per_symbol / nsync / ndata)
  DevBuf drift_idx, drift_tmpl;
  int tmpl_key[3] = {0, 0, 0};
  int tmpl_len = 0;
  bool timing = false;
  uint32_t stage_mask = 0xFFFFFFFFu;  // stages that record events while timing is on
  std::vector<TimedLaunch> pending;
  std::vector<hipEvent_t> pool;
  double ms[FT8_N_STAGES] = {0};
  int64_t launches[FT8_N_STAGES] = {0};
  // decode_batch pipeline: slot chunks spread over internal streams (0 = one chain on the caller's
  // stream); BP grid residency in waves per SIMD
  int chunk_slots = 0, n_streams = 0, bp_waves = 4;
  std::vector<hipStream_t> streams;
  hipEvent_t fork = nullptr;
  std::vector<hipEvent_t> joins;
  // the kernels of the last single-chain ft8_decode_batch, for ft8_replay_stage (benchmarking):
  // valid until the next entry point that may reallocate the context's scratch
  bool replay_ok = false;
  // ft8_snr_last: the last ft8_decode_batch left its whole waterfall in `wf` (chunked or not) and
  // snr_batch describes it; cleared wherever replay_ok is.  A and N0 of the report go to snr_A / snr_N0
  bool snr_ok = false;
  struct {
    int n_slots, T, F, cap;
    bool f64, subtract;
    double bw_db;  // 10 log10(enbw_hz / 2500) of the batch's geometry
    int sps, bpt;
    bool ft4;      // an FT4 batch: the report's symbol layout is FT8's, so ft8_snr_last refuses
  } snr_batch{};
  DevBuf snr_A, snr_N0;
  // the retry passes of ft8_decode_batch and their stage calls, each sized for one call
  ApRetry ap;
  CoherentRetry coh;
  CoherentApRetry cohap;
  OsdRetry osd;
  // the stream of the last entry point that enqueued work, and an event recorded on it after that
  // work (StreamOrder): a call on another stream first waits for it
  hipStream_t last_stream = nullptr;
  hipEvent_t last_done = nullptr;
  bool have_last = false;
  StftLaunch last_stft{};
  SyncLaunch last_sync{};
  BpLaunch last_bp{};
  CompactLaunch last_compact{};
};

namespace {

int fail(ft8_ctx* c, int code, const std::string& msg) {
  if (c) c->err = msg;
  return code;
}

int hipfail(ft8_ctx* c, hipError_t e, const char* where) {
  return fail(c, FT8_E_HIP, std::string(where) + ": " + hipGetErrorString(e));
}

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) (void)hipSetDevice(dev);
  }
  ~DeviceGuard() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};

// grow-only scratch: at least `bytes` (a quarter more when it has to grow), old contents dropped
int ensure(ft8_ctx* c, DevBuf& b, size_t bytes) {
  if (bytes == 0) bytes = 16;
  if (b.cap >= bytes) return FT8_OK;
  b.release();
  size_t want = bytes + bytes / 4;
  hipError_t e = hipMalloc(&b.p, want);
  if (e != hipSuccess) {
    b.p = nullptr;
    (void)hipGetLastError();
    return fail(c, FT8_E_NOMEM, std::string("hipMalloc failed for ") + std::to_string(want) + " bytes");
  }
  b.cap = want;
  return FT8_OK;
}

// ensure() for a buffer that must read as zeros when (re)allocated: the k_bp work counters, which
// every k_bp launch leaves at 0 again (bp.hip), so they are cleared only here
// *reallocated (optional) reports whether the buffer was (re)allocated and zeroed; a grown buffer
// can come back at the old address, so the test is the capacity as well as the pointer
int ensure_zeroed(ft8_ctx* c, DevBuf& b, size_t bytes, hipStream_t s, bool* reallocated = nullptr) {
  void* old = b.p;
  const size_t old_cap = b.cap;
  if (reallocated) *reallocated = false;
  int rc = ensure(c, b, bytes);
  if (rc || (b.p == old && b.cap == old_cap)) return rc;
  if (reallocated) *reallocated = true;
  hipError_t e = hipMemsetAsync(b.p, 0, b.cap, s);
  return e == hipSuccess ? FT8_OK : hipfail(c, e, "memset");
}

// the k_bp claim counters (8 B each) and their host-side ticket bases: whenever the counters are
// (re)allocated they read 0, so every base restarts at 0 and the vector covers the new capacity
int ensure_work(ft8_ctx* c, int n_counters, hipStream_t s) {
  bool fresh = false;
  int rc = ensure_zeroed(c, c->work, sizeof(unsigned long long) * (size_t)n_counters, s, &fresh);
  if (rc) return rc;
  if (fresh) c->work_base.assign(c->work.cap / sizeof(unsigned long long), 0ull);
  return FT8_OK;
}

// Claim counter indices: [0] belongs to ft8_bp / ft8_ap_decode (a caller stream, in order); a batch of
// n_chunks chunks then holds one per chunk for plain BP, for the a-priori pass and for the coherent
// pass, in that order, and last for the a-priori retries on the coherent LLRs, so that chunks on
// different streams never share one.
enum BpUser { kCallerBp = -1, kChunkBp = 0, kChunkAp = 1, kChunkCoherent = 2, kChunkCoherentAp = 3 };
int bp_counter(BpUser u, int k, int n_chunks) { return u == kCallerBp ? 0 : 1 + (int)u * n_chunks + k; }
// counters of a batch: through its last user's
int bp_counters(bool ap, bool coh, bool coh_ap, int n_chunks) {
  return bp_counter(coh_ap ? kChunkCoherentAp : coh ? kChunkCoherent : ap ? kChunkAp : kChunkBp, n_chunks - 1,
                    n_chunks) + 1;
}

hipEvent_t get_event(ft8_ctx* c) {
  if (!c->pool.empty()) {
    hipEvent_t e = c->pool.back();
    c->pool.pop_back();
    return e;
  }
  hipEvent_t e;
  (void)hipEventCreate(&e);
  return e;
}

struct StageTimer {
  ft8_ctx* c;
  Stage stage;
  hipStream_t s;
  hipEvent_t a = nullptr;
  StageTimer(ft8_ctx* c_, Stage st, hipStream_t s_) : c(c_), stage(st), s(s_) {
    if (c->timing && ((c->stage_mask >> st) & 1u)) {
      a = get_event(c);
      (void)hipEventRecord(a, s);
    }
  }
  void done() {
    if (c->timing && a) {
      hipEvent_t b = get_event(c);
      (void)hipEventRecord(b, s);
      c->pending.push_back({stage, a, b});
      a = nullptr;
    }
  }
};

// one timed launch: `launch()` enqueues on s and returns its hipError_t; a failure is the context's
// error "<what>: <hip error>"
template <typename F>
int timed_launch(ft8_ctx* c, Stage stage, hipStream_t s, const char* what, F&& launch) {
  StageTimer t(c, stage, s);
  const hipError_t e = launch();
  t.done();
  return e == hipSuccess ? FT8_OK : hipfail(c, e, what);
}

// Stream order of a context's work.  The scratch buffers, the k_bp claim counters and their
// host-side ticket bases assume that a context's launches run one after another; an entry point
// that uses them, called on a stream other than the previous such call's, first waits (device side,
// no host sync) for an event recorded after that call's work.  (Entry points that touch no context
// state -- ft8_sync_score, ft8_llr, ft8_normalize, ft8_encode, ft8_pack_decodes, ft8_crc14,
// ft8_ldpc_check -- take no part, so they never serialise two contexts' streams.)  Without it, two streams sharing one context (e.g. one
// host thread alternating torch streams) would run two calls' kernels concurrently on the same
// scratch and interleave the tickets of two k_bp launches.
struct StreamOrder {
  ft8_ctx* c;
  hipStream_t s;
  StreamOrder(ft8_ctx* c_, hipStream_t s_) : c(c_), s(s_) {
    if (!c) return;
    if (c->have_last && c->last_stream != s) (void)hipStreamWaitEvent(s, c->last_done, 0);
  }
  ~StreamOrder() {
    if (!c) return;
    DeviceGuard dg(c->device);  // the event lives on the context's device
    if (!c->last_done && hipEventCreateWithFlags(&c->last_done, hipEventDisableTiming) != hipSuccess) {
      c->last_done = nullptr;
      return;
    }
    if (hipEventRecord(c->last_done, s) == hipSuccess) {
      c->last_stream = s;
      c->have_last = true;
    }
  }
};

// NumPy pairwise summation of a complex64 array with zero imaginary parts (real part returned),
// CFLOAT_pairwise_sum with n counted in floats (loops_utils.h.src)
float cfloat_pairwise_re(const float* re, long n_floats) {
  if (n_floats < 8) {
    float rr = -0.0f;
    for (long i = 0; i < n_floats; i += 2) rr += re[i / 2];
    return rr;
  } else if (n_floats <= 128) {
    float r[4];
    for (int j = 0; j < 4; ++j) r[j] = re[j];
    long i;
    for (i = 8; i < n_floats - (n_floats % 8); i += 8)
      for (int j = 0; j < 4; ++j) r[j] += re[i / 2 + j];
    float rr = (r[0] + r[1]) + (r[2] + r[3]);
    for (; i < n_floats; i += 2) rr += re[i / 2];
    return rr;
  } else {
    long n2 = n_floats / 2;
    n2 -= n2 % 8;
    return cfloat_pairwise_re(re, n2) + cfloat_pairwise_re(re + n2 / 2, n_floats - n2);
  }
}

double double_pairwise(const double* a, long n) {
  if (n < 8) {
    double r = -0.0;
    for (long i = 0; i < n; ++i) r += a[i];
    return r;
  } else if (n <= 128) {
    double r[8];
    for (int j = 0; j < 8; ++j) r[j] = a[j];
    long i;
    for (i = 8; i < n - (n % 8); i += 8)
      for (int j = 0; j < 8; ++j) r[j] += a[i + j];
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += a[i];
    return res;
  } else {
    long n2 = n / 2;
    n2 -= n2 % 8;
    return double_pairwise(a, n2) + double_pairwise(a + n2, n - n2);
  }
}

// periodic Hann window exactly as scipy.signal.get_window('hann', L) builds it:
// general_cosine(L + 1, [0.5, 0.5]) truncated, fac = linspace(-pi, pi, L + 1)
std::vector<double> hann(int L) {
  std::vector<double> w(L);
  const double start = -M_PI, stop = M_PI;
  const double step = (stop - start) / (double)L;
  for (int i = 0; i < L; ++i) {
    const double fac = (double)i * step + start;
    w[i] = (0.0 + 0.5 * 1.0) + 0.5 * std::cos(fac);
  }
  if (L == 1) w[0] = 1.0;
  return w;
}

// n host values of T in a fresh device buffer of exactly that size
template <typename T>
hipError_t upload(DevBuf& b, const std::vector<T>& host) {
  b.release();
  const size_t bytes = sizeof(T) * host.size();
  hipError_t e = hipMalloc(&b.p, bytes);
  if (e != hipSuccess) {
    b.p = nullptr;
    return e;
  }
  b.cap = bytes;
  return hipMemcpy(b.p, host.data(), bytes, hipMemcpyHostToDevice);
}

// a complex table of n entries, gen(i, &re, &im) in long double, rounded to the plan's type
// (cplx<double> or cplx<float>)
template <typename Gen>
hipError_t upload_table(DevBuf& b, bool f64, size_t n, Gen&& gen) {
  auto build = [&](auto zero) {
    using CT = decltype(zero);
    std::vector<cplx<CT>> host(n);
    for (size_t i = 0; i < n; ++i) {
      long double re, im;
      gen(i, &re, &im);
      host[i] = {(CT)re, (CT)im};
    }
    return upload(b, host);
  };
  return f64 ? build(0.0) : build(0.0f);
}

int get_window(ft8_ctx* c, int L, bool f64, WinEntry** out) {
  for (auto& w : c->wins)
    if (w.L == L && w.f64 == f64) { *out = &w; return FT8_OK; }
  std::vector<double> w = hann(L);
  WinEntry e;
  e.L = L;
  e.f64 = f64;
  hipError_t he;
  if (f64) {
    double s = 0.0 + double_pairwise(w.data(), L);
    e.scale = 1.0 / (s * s);
    he = upload(e.w, w);
  } else {
    std::vector<float> w32(L);
    for (int i = 0; i < L; ++i) w32[i] = (float)w[i];
    float s = 0.0f + cfloat_pairwise_re(w32.data(), 2L * L);
    float sq = s * s;
    e.scale = (double)(1.0f / sq);
    he = upload(e.w, w32);
  }
  if (he != hipSuccess) return hipfail(c, he, "window upload");
  c->wins.push_back(std::move(e));
  *out = &c->wins.back();
  return FT8_OK;
}

bool factor(int P, FftPlan& pl) {
  pl.nstages = 0;
  int r = P;
  auto take = [&](int f) {
    while (r % f == 0 && pl.nstages < 16) {
      pl.radix[pl.nstages++] = f;
      r /= f;
    }
  };
  // few, large register-resident stages: every stage is one LDS round trip
  take(16);
  take(8);
  take(4);
  take(2);
  take(15);
  take(5);
  take(3);
  take(7);
  return r == 1 && pl.nstages > 0;
}

// in-place radix-2 FFT (long double, host) of a power-of-two length: the chirp-z filter spectra
void host_fft_pow2(std::vector<long double>& re, std::vector<long double>& im) {
  const size_t n = re.size();
  for (size_t i = 1, j = 0; i < n; ++i) {
    size_t bit = n >> 1;
    for (; j & bit; bit >>= 1) j ^= bit;
    j ^= bit;
    if (i < j) {
      std::swap(re[i], re[j]);
      std::swap(im[i], im[j]);
    }
  }
  for (size_t len = 2; len <= n; len <<= 1) {
    for (size_t k = 0; k < len / 2; ++k) {
      const long double ang = -2.0L * M_PIl * (long double)k / (long double)len;
      const long double wr = cosl(ang), wi = sinl(ang);
      for (size_t i = k; i < n; i += len) {
        const size_t j = i + len / 2;
        const long double xr = re[j] * wr - im[j] * wi, xi = re[j] * wi + im[j] * wr;
        re[j] = re[i] - xr;
        im[j] = im[i] - xi;
        re[i] += xr;
        im[i] += xi;
      }
    }
  }
}

// exp(-i pi j^2 / N) from the exact residue j^2 mod 2N
void chirp_of(int64_t j, int N, long double* cr, long double* ci) {
  const int64_t r = (j * j) % (2 * (int64_t)N);
  const long double ang = -M_PIl * (long double)r / (long double)N;
  *cr = cosl(ang);
  *ci = sinl(ang);
}

// the chirp-z tables of a plan (P = the convolution length, a power of two): chirp c(k), k < nfft,
// and the spectra of the nblk block filters h_b[m] = conj(c(b B + m - (L - 1))), m < P
int blue_tables(ft8_ctx* c, PlanEntry& e, int nfft, int L, int P, bool f64) {
  const int B = P - L + 1;
  const int nblk = (nfft + B - 1) / B;
  std::vector<long double> hre((size_t)nblk * P), him((size_t)nblk * P), re(P), im(P);
  for (int b = 0; b < nblk; ++b) {
    for (int m = 0; m < P; ++m) {
      long double cr, ci;
      chirp_of((int64_t)b * B + m - (L - 1), nfft, &cr, &ci);
      re[m] = cr;
      im[m] = -ci;
    }
    host_fft_pow2(re, im);
    std::copy(re.begin(), re.end(), hre.begin() + (size_t)b * P);
    std::copy(im.begin(), im.end(), him.begin() + (size_t)b * P);
  }
  // both straight from long double to the plan's type
  hipError_t he = upload_table(e.chirp, f64, nfft, [&](size_t k, long double* cr, long double* ci) {
    chirp_of((int64_t)k, nfft, cr, ci);
  });
  if (he == hipSuccess)
    he = upload_table(e.hspec, f64, hre.size(), [&](size_t i, long double* xr, long double* xi) {
      *xr = hre[i];
      *xi = him[i];
    });
  if (he != hipSuccess) return hipfail(c, he, "chirp-z plan upload");
  e.plan.L = L;
  e.plan.B = B;
  e.plan.nblk = nblk;
  e.plan.chirp = e.chirp.p;
  e.plan.hspec = e.hspec.p;
  return FT8_OK;
}

int get_plan(ft8_ctx* c, int nfft, bool cplx, bool f64, int nperseg, FftPlan* out) {
  for (auto& p : c->plans)
    // a fallback plan (chirp-z or direct DFT) was chosen for one nperseg: the choice between the
    // two depends on it, so such a plan is reused only for that nperseg
    if (p.nfft == nfft && p.cplx == cplx && p.f64 == f64 && (!(p.plan.blue || p.plan.dft) || p.L == nperseg)) {
      *out = p.plan;
      return FT8_OK;
    }
  PlanEntry e;
  e.nfft = nfft;
  e.cplx = cplx;
  e.f64 = f64;
  int P = cplx ? nfft : nfft / 2;
  e.plan.dft = 0;
  e.plan.blue = 0;
  // lengths the LDS Stockham FFT cannot take (a prime factor above 7, odd real nfft, above the
  // compiled limit) take the chirp-z transform when its convolution fits the LDS FFT and is the
  // cheaper one, else the direct DFT kernel (P = nfft, tw = W_nfft^m)
  const int max_p = f64 ? kMaxFftP64 : (cplx ? kMaxFftComplex : kMaxFftReal / 2);
  if ((!cplx && (nfft % 2)) || P > max_p || !factor(P, e.plan)) {
    if (nfft > kMaxDft) return fail(c, FT8_E_RANGE, "nfft " + std::to_string(nfft) + " exceeds the compiled DFT limit");
    // chirp-z: P a power of two >= L + (bins needed) - 1, capped at the LDS FFT limit; cost per frame
    // ~ blocks x 2 x 5 P log2 P against the direct DFT's 8 L per kept bin
    const int need = cplx ? nfft : (nfft + 1) / 2;
    const int pmax = f64 ? kMaxBlueP64 : kMaxBlueP32;
    int M = 1;
    while (M < nperseg + need - 1 && M < pmax) M <<= 1;
    int lg = 0;
    while ((1 << lg) < M) ++lg;
    const double blocks = M > nperseg ? std::ceil((double)need / (double)(M - nperseg + 1)) : 0.0;
    const bool blue = M > nperseg && blocks * 10.0 * M * lg < 8.0 * nperseg * need;
    if (blue && factor(M, e.plan)) {
      P = M;
      e.plan.blue = 1;
      e.L = nperseg;
      int rc = blue_tables(c, e, nfft, nperseg, M, f64);
      if (rc) return rc;
    } else {
      P = nfft;
      e.plan.dft = 1;
      e.plan.nstages = 0;
      e.L = nperseg;
    }
  }
  e.plan.P = P;
  // twiddles W_P^m and post-processing W_N^k (N = 2P), from long double angles, rounded to double
  // and from there to the plan's type
  auto root_of_unity = [](size_t k, int n, long double* cr, long double* ci) {
    const long double ang = -2.0L * M_PIl * (long double)k / (long double)n;
    *cr = (double)cosl(ang);
    *ci = (double)sinl(ang);
  };
  hipError_t he = upload_table(e.tw, f64, P, [&](size_t m, long double* cr, long double* ci) {
    root_of_unity(m, P, cr, ci);
  });
  if (he == hipSuccess)
    he = upload_table(e.post, f64, (size_t)P + 1, [&](size_t k, long double* cr, long double* ci) {
      root_of_unity(k, 2 * P, cr, ci);
    });
  if (he != hipSuccess) return hipfail(c, he, "fft plan upload");
  e.plan.tw = e.tw.p;
  e.plan.post = e.post.p;
  *out = e.plan;
  c->plans.push_back(std::move(e));
  return FT8_OK;
}

struct Geo {
  int nperseg, hop, noverlap, nfft, frames;
};

// the sample rate a parameter block names: the exact Hz when given (ABI 2), else the integral field
double rate_of(const ft8_params* p) { return p->sample_rate_hz > 0.0 ? p->sample_rate_hz : (double)p->sample_rate; }

// fs in double: the reference computes both lengths on the float it was given (a float fs such as
// 10e3 or 12006.3 is legal there), so int(0.16 * 12006.3) = 1921, not int(0.16 * 12006) = 1920
int geometry(double fs, int bpt, int sps, int64_t n, Geo* g, std::string* why) {
  if (!(fs > 0.0) || !(fs < 2e9) || bpt <= 0 || sps <= 0) { *why = "sample_rate, bins_per_tone and steps_per_symbol must be positive"; return FT8_E_ARG; }
  g->nperseg = (int)(0.16 * fs);                         // spectrogram_analyse.py:32
  g->noverlap = g->nperseg - g->nperseg / sps;           // :33
  g->nfft = (int)(fs / 6.25 * (double)bpt);              // :34
  if (g->noverlap >= g->nperseg) g->noverlap = g->nperseg - 1;  // :42-43
  g->hop = g->nperseg - g->noverlap;
  if (g->nperseg < 1) { *why = "nperseg must be a positive integer"; return FT8_E_ARG; }
  if (g->nfft < g->nperseg) { *why = "nfft must be greater than or equal to nperseg."; return FT8_E_ARG; }
  g->frames = (n < g->nperseg) ? 0 : (int)((n - g->noverlap) / g->hop);
  return FT8_OK;
}

// FT4's scrambling vector on the host (ft4_device.h holds the device's copy)
constexpr uint8_t kFt4Rvec[10] = {0x4a, 0x5e, 0x89, 0xb4, 0xb0, 0x8a, 0x79, 0x55, 0xbe, 0x28};

// FT4's samples per symbol, fs * 6 / 125 (T = 0.048 s), or 0 where that is no whole number >= 8
int ft4_nsps(double fs) {
  const double v = fs * 6.0 / 125.0;
  return (v >= 8.0 && v < 1e9 && v == std::floor(v)) ? (int)v : 0;
}

// the geometry of a protocol (ft8hip.h, "FT4": nperseg = nsps, the reference's noverlap rule, nfft = nsps bpt)
int geometry(int protocol, double fs, int bpt, int sps, int64_t n, Geo* g, std::string* why) {
  if (protocol == FT8_PROTO_FT8) return geometry(fs, bpt, sps, n, g, why);
  if (protocol != FT8_PROTO_FT4) { *why = "unknown ft8_params.protocol"; return FT8_E_ARG; }
  if (!(fs > 0.0) || !(fs < 2e9) || bpt <= 0 || sps <= 0) { *why = "sample_rate, bins_per_tone and steps_per_symbol must be positive"; return FT8_E_ARG; }
  const int nsps = ft4_nsps(fs);
  if (nsps == 0) { *why = "FT4 needs a sample rate whose 0.048-s symbol is a whole number of samples (>= 8)"; return FT8_E_UNSUPPORTED; }
  if ((int64_t)nsps * bpt > INT32_MAX) { *why = "nfft out of range"; return FT8_E_ARG; }
  g->nperseg = nsps;
  g->noverlap = nsps - nsps / sps;
  if (g->noverlap >= g->nperseg) g->noverlap = g->nperseg - 1;
  g->hop = g->nperseg - g->noverlap;
  g->nfft = nsps * bpt;
  g->frames = (n < g->nperseg) ? 0 : (int)((n - g->noverlap) / g->hop);
  return FT8_OK;
}
int geometry(const ft8_params* p, int64_t n, Geo* g, std::string* why) {
  return geometry(p->protocol, rate_of(p), p->bins_per_tone, p->steps_per_symbol, n, g, why);
}

// the entry points that take an ft8_params but no FT4: FT8_E_ARG for an unknown protocol, FT8_E_UNSUPPORTED
// for FT4
int ft8_only(ft8_ctx* c, const ft8_params* p, const char* who) {
  if (p->protocol == FT8_PROTO_FT8) return FT8_OK;
  if (p->protocol != FT8_PROTO_FT4) return fail(c, FT8_E_ARG, "unknown ft8_params.protocol");
  return fail(c, FT8_E_UNSUPPORTED, std::string(who) + " does not take FT4");
}

bool is_f64_dtype(int dt) { return dt == FT8_F64 || dt == FT8_C128; }
bool is_cplx_dtype(int dt) { return dt == FT8_C64 || dt == FT8_C128; }

// what an StftLaunch is built for: dB rows (an empty bin range is an empty result), the per-frame
// argmax (an empty bin range has none: an error), or only the choice of kernel (ft8_stft_method: no
// ranges, no window)
enum class StftUse { Rows, Argmax, Method };

// The one place that validates an STFT request and fills its launch block: geometry, dtype, frame
// and bin ranges, plan, the direct DFT's LDS limit, window.  *launch = false: valid, nothing to
// compute.  samples / out / argmax / screen_* stay with the caller.
int make_stft_launch(ft8_ctx* c, const ft8_params* p, int dtype, int64_t n_samples, int n_slots, int64_t stride,
                     StftUse use, StftLaunch* L, bool* launch) {
  Geo g;
  std::string why;
  int rc = geometry(p, n_samples, &g, &why);
  if (rc) return fail(c, rc, why);
  if (dtype < FT8_F32 || dtype > FT8_I16) return fail(c, FT8_E_ARG, "unknown sample dtype");
  *launch = false;
  if (use != StftUse::Method) {
    if (p->t_lo < 0 || p->t_hi > g.frames || p->t_lo > p->t_hi)
      return fail(c, FT8_E_ARG, "frame range [t_lo, t_hi) outside [0, " + std::to_string(g.frames) + ")");
    if (use == StftUse::Argmax) {
      if (p->f_lo < 0 || p->f_hi > g.nfft || p->f_lo >= p->f_hi) return fail(c, FT8_E_ARG, "bin range [f_lo, f_hi) empty or outside [0, nfft)");
    } else if (p->f_lo < 0 || p->f_hi > g.nfft || p->f_lo > p->f_hi) {
      return fail(c, FT8_E_ARG, "bin range [f_lo, f_hi) outside [0, nfft)");
    }
    if (p->t_hi == p->t_lo || p->f_hi == p->f_lo || n_slots == 0) return FT8_OK;
  }
  const bool f64 = is_f64_dtype(dtype);
  *L = StftLaunch{};
  L->dtype = dtype;
  L->n_samples = n_samples;
  L->slot_stride = stride;
  L->n_slots = n_slots;
  L->nperseg = g.nperseg;
  L->hop = g.hop;
  L->nfft = g.nfft;
  L->t_lo = p->t_lo;
  L->t_hi = p->t_hi;
  L->f_lo = p->f_lo;
  L->f_hi = p->f_hi;
  if ((rc = get_plan(c, g.nfft, is_cplx_dtype(dtype), f64, g.nperseg, &L->plan))) return rc;
  *launch = true;
  if (use == StftUse::Method) return FT8_OK;
  if (L->plan.dft && (size_t)g.nperseg * (f64 ? 16 : 8) > (size_t)kMaxDftLds)
    return fail(c, FT8_E_RANGE, "nperseg " + std::to_string(g.nperseg) + " exceeds the direct-DFT limit");
  WinEntry* w = nullptr;
  if ((rc = get_window(c, g.nperseg, f64, &w))) return rc;
  L->window = w->w.p;
  L->scale = w->scale;
  return FT8_OK;
}

int do_stft(ft8_ctx* c, const void* samples, int dtype, int64_t n_samples, int n_slots, int64_t slot_stride,
            const ft8_params* p, void* d_wf, hipStream_t s) {
  StftLaunch L;
  bool launch;
  int rc = make_stft_launch(c, p, dtype, n_samples, n_slots, slot_stride, StftUse::Rows, &L, &launch);
  if (rc || !launch) return rc;
  L.samples = samples;
  L.out = d_wf;
  c->last_stft = L;
  return timed_launch(c, kStft, s, "stft launch", [&] { return launch_stft(L, s); });
}

struct Grid {
  int t0, NT, NF;
};
Grid grid_of(int T, int F, int sps, int bpt, int protocol) {
  // ft8_find_candidates ranges (ft8_decode.py:108-109): a frame may start 10 symbols early and end 20
  // late.  FT4: 103 symbols of 4 tones (ft8hip.h, "FT4") for FT8's 79 of 8.
  const bool ft4 = protocol == FT8_PROTO_FT4;
  Grid g;
  const int nb = T / sps;
  g.t0 = -10 * sps;
  const int t_end = nb * sps - sps * (ft4 ? FT8_FT4_SYMBOLS - 20 : 59);
  g.NT = t_end > g.t0 ? t_end - g.t0 : 0;
  const int tones = ft4 ? 3 : 7;
  g.NF = F - tones * bpt > 0 ? F - tones * bpt : 0;
  return g;
}
Grid grid_of(int T, int F, const ft8_params* p) {
  return grid_of(T, F, p->steps_per_symbol, p->bins_per_tone, p->protocol);
}
// score scratch per slot: elements (the full grid NT x NF, or the compact layout NT x nseg x 128)
// and segment-mask words
size_t score_elems(const Grid& g) { return (size_t)g.NT * n_segments(g.NF) * kSegCols; }
size_t smask_words(const Grid& g) { return (size_t)g.NT * n_segments(g.NF) * 2; }

// the score/select scratch of a run of slots: scores [n][score_elems] in the waterfall's type, smask
// [n][smask_words], warn [n], rowsum [n][NT][nseg], tie [n][tie_stride(N)] (float32 scores only)
struct SelScratch {
  void* scores;
  uint64_t* smask;
  int32_t* warn;
  RowSummary* rowsum;
  int32_t* tie;
};

// sizes the context's score/select scratch for n_slots slots (own_scores = false: the caller brings
// the score grid)
int ensure_sel_scratch(ft8_ctx* c, int n_slots, const Grid& g, int N, bool f64, bool own_scores = true) {
  const size_t n = (size_t)n_slots;
  int rc;
  if (own_scores && (rc = ensure(c, c->scores, (f64 ? 8 : 4) * n * score_elems(g)))) return rc;
  if ((rc = ensure(c, c->smask, sizeof(uint64_t) * n * smask_words(g)))) return rc;
  if ((rc = ensure(c, c->warn, sizeof(int32_t) * n))) return rc;
  if ((rc = ensure(c, c->rowsum, sizeof(RowSummary) * n * g.NT * n_segments(g.NF)))) return rc;
  if (!f64 && (rc = ensure(c, c->tie, sizeof(int32_t) * n * tie_stride(N)))) return rc;
  return FT8_OK;
}

// the part of that scratch that starts at slot `slot0`
SelScratch sel_scratch_at(const ft8_ctx* c, int slot0, const Grid& g, int N, bool f64) {
  const size_t k = (size_t)slot0;
  return {c->scores.as<char>() + (f64 ? 8 : 4) * k * score_elems(g), c->smask.as<uint64_t>() + k * smask_words(g),
          c->warn.as<int32_t>() + k, c->rowsum.as<RowSummary>() + k * g.NT * n_segments(g.NF),
          f64 ? nullptr : c->tie.as<int32_t>() + k * tie_stride(N)};
}

// the search parameters ft8_sync_select and ft8_decode_batch share.  The two entry points have
// always reported a call that breaks two rules differently: ft8_decode_batch names the candidate
// limit first, ft8_sync_select the flags (limit_first).
int check_search_params(ft8_ctx* c, const ft8_params* p, bool limit_first) {
  if (p->steps_per_symbol <= 0 || p->bins_per_tone <= 0) return fail(c, FT8_E_ARG, "bad oversampling factors");
  if (p->protocol != FT8_PROTO_FT8 && p->protocol != FT8_PROTO_FT4) return fail(c, FT8_E_ARG, "unknown ft8_params.protocol");
  const bool over = p->max_candidates > kMaxCandidates;
  if ((p->flags & ~(FT8_FLAG_TOPK | FT8_FLAG_SUBTRACT | FT8_FLAG_AP | FT8_FLAG_COHERENT | FT8_FLAG_OSD | FT8_FLAG_BP_F32)) && !(limit_first && over))
    return fail(c, FT8_E_ARG, "unknown bits in ft8_params.flags");
  if (over) return fail(c, FT8_E_RANGE, "max_candidates > " + std::to_string(kMaxCandidates) + " is not supported");
  return FT8_OK;
}

int decode_pass(ft8_ctx* c, const void* d_samples, int dtype, int64_t n_samples, int32_t n_slots,
                int64_t slot_stride, const ft8_params* p, ft8_result* d_out, int32_t* d_counts, int32_t cap,
                hipStream_t s);
int subtract_core(ft8_ctx* c, const void* x, int dtype, float* resid, int64_t n_samples, int n_slots,
                  int64_t x_stride, int64_t r_stride, const ft8_params* p, const ft8_result* res,
                  const int32_t* counts, int cap, hipStream_t s, const int32_t* first = nullptr, int first_stride = 0);
int gfsk_tables(ft8_ctx* c, int nsps, double bt = 2.0);

// the counter half of a k_bp launch: claim counter `counter` (ensure_work) and its host ticket base,
// the work counters, the clock counters while timing is on (ft8_set_timing allocates them), and the
// persistent grid's resident waves per SIMD (kernel maximum 4)
void wire_bp_counters(ft8_ctx* c, BpLaunch& B, int counter, int grid_waves) {
  B.work = c->work.as<unsigned long long>() + counter;
  B.work_base = &c->work_base[counter];
  B.stats = c->stats.as<unsigned long long>();
  B.clock = c->timing && c->stats.p ? B.stats + 4 : nullptr;
  B.grid_waves = grid_waves;
}

// k_bp (f32: k_bp32, an FT8_FLAG_BP_F32 batch) in mode 0 over a retry pass's compacted lists: llr_in /
// plain_out (nullable) / res_out per list position
hipError_t bp_over_lists(ft8_ctx* c, const RetryLists& l, const double* llr_in, uint8_t* plain_out,
                         ft8_result* res_out, int max_iterations, int counter, hipStream_t s, bool f32) {
  BpLaunch B{};
  B.cand = l.cand;
  B.cand_score = l.score;
  B.cand_count = l.count;
  B.N = l.M;
  B.n_slots = l.n_slots;
  B.n_items = l.n_slots * l.M;
  B.mode = 0;
  B.max_iterations = max_iterations;
  B.llr_in = llr_in;
  B.plain_out = plain_out;
  B.res = res_out;
  B.f32 = f32 ? 1 : 0;
  wire_bp_counters(c, B, counter, c->bp_waves);
  return run_bp(B, s);
}

// score + select on the scratch `sc`; compact: the score kernel may write only the passing scores
// (k_score2 path, reference selection), else the full grid
int sync_select_core(ft8_ctx* c, const void* d_wf, int wf_f64, int n_slots, int T, int F, const ft8_params* p,
                     int32_t* cand, double* cand_score, int32_t* cand_count, const SelScratch& sc, int compact,
                     hipStream_t s) {
  Grid g = grid_of(T, F, p);
  SyncLaunch L{};
  L.protocol = p->protocol;
  L.wf = d_wf;
  L.wf_f64 = wf_f64;
  L.n_slots = n_slots;
  L.T = T;
  L.F = F;
  L.sps = p->steps_per_symbol;
  L.bpt = p->bins_per_tone;
  L.t0 = g.t0;
  L.NT = g.NT;
  L.NF = g.NF;
  L.scores = sc.scores;
  L.smask = sc.smask;
  L.compact = compact;
  L.N = p->max_candidates;
  L.min_score = p->min_score;
  L.min_score_f64 = p->min_score_f64;
  L.cand = cand;
  L.cand_score = cand_score;
  L.cand_count = cand_count;
  L.warn = sc.warn;
  L.rowsum = sc.rowsum;
  L.tie = sc.tie;
  L.topk = (p->flags & FT8_FLAG_TOPK) ? 1 : 0;
  c->last_sync = L;
  int rc = timed_launch(c, kScore, s, "score launch", [&] { return launch_score(L, s); });
  if (rc) return rc;
  return timed_launch(c, kSelect, s, "select launch", [&] { return launch_select(L, s); });
}

int do_sync_select(ft8_ctx* c, const void* d_wf, int wf_f64, int n_slots, int T, int F, const ft8_params* p,
                   int32_t* cand, double* cand_score, int32_t* cand_count, void* d_scores, hipStream_t s) {
  int rc = check_search_params(c, p, false);
  if (rc) return rc;
  const int N = p->max_candidates;
  Grid g = grid_of(T, F, p);
  if (N <= 0 || g.NT == 0 || g.NF == 0 || n_slots == 0) {
    hipError_t e = hipMemsetAsync(cand_count, 0, sizeof(int32_t) * (size_t)(n_slots > 0 ? n_slots : 0), s);
    return e == hipSuccess ? FT8_OK : hipfail(c, e, "memset");
  }
  // without a caller grid the scores stay in the compact layout (only passing scores written)
  if ((rc = ensure_sel_scratch(c, n_slots, g, N, wf_f64, d_scores == nullptr))) return rc;
  SelScratch sc = sel_scratch_at(c, 0, g, N, wf_f64);
  if (d_scores) sc.scores = d_scores;
  if ((rc = sync_select_core(c, d_wf, wf_f64, n_slots, T, F, p, cand, cand_score, cand_count, sc,
                             d_scores == nullptr, s)))
    return rc;
  // float32 scores: k_select leaves equal scores in scan order and k_tie_apply replays the
  // reference heap for the slots that have them (the same code k_llr runs inside decode_batch)
  if (sc.tie) {
    const TieArgs ta{n_slots, N, cand_count, sc.warn, sc.tie, cand_score};
    hipError_t e = launch_tie_apply(ta, cand, cand_score, s);
    if (e != hipSuccess) return hipfail(c, e, "tie launch");
  }
  return FT8_OK;
}

// ---- a-priori decoding ---------------------------------------------------------------------------
// The AP pass over the records `failed` describes (everything but M, gate and the list arrays) and
// llr[n_slots][N][174], the context's hypotheses one after another (ap.hip), on the scratch of the chunk
// that starts at slot `slot0`; `counter` is the k_bp claim counter the pass's launches draw their
// tickets from.
int ap_pass(ft8_ctx* c, const RetryLists& failed, const double* llr, int slot0, int max_iterations, int16_t* hard,
            int counter, hipStream_t s, int protocol = FT8_PROTO_FT8, bool f32 = false) {
  const ApRetry::View v = c->ap.at(failed, slot0);
  ApLaunch A{v.lists, llr, {}, 0, c->ap.max_hard, v.amax, v.llr, v.plain, v.res, hard};
  A.r.gate = A.amax;
  hipError_t e = launch_ap_amax(A, s);
  if (e != hipSuccess) return hipfail(c, e, "ap launch");
  for (size_t h = 0; h < c->ap.hyps.size(); ++h) {
    A.hyp = c->ap.hyps[h];
    // FT4: the LLRs and the decoded payload are in scrambled bits, the context's hypotheses in message
    // bits, so the launch's copy takes rvec on its value; clamp and acceptance then agree
    if (protocol == FT8_PROTO_FT4)
      for (int i = 0; i < 10; ++i) A.hyp.value[i] ^= kFt4Rvec[i];
    A.h = (int)h;
    if ((e = launch_retry_list(A.r, s)) != hipSuccess) return hipfail(c, e, "ap launch");
    if ((e = launch_ap_clamp(A, s)) != hipSuccess) return hipfail(c, e, "ap launch");
    if ((e = bp_over_lists(c, A.r, v.llr, v.plain, v.res, max_iterations, counter, s, f32)) != hipSuccess)
      return hipfail(c, e, "ap bp launch");
    if ((e = launch_ap_merge(A, s)) != hipSuccess) return hipfail(c, e, "ap launch");
  }
  return FT8_OK;
}

// ---- the baseband front end of the subtraction and the coherent pass (baseband.h) ---------------
// decimated samples per symbol: 32 when nsps allows, else the largest divisor of nsps in [8, 32]
int sub_q(int nsps) {
  for (int q = 32; q >= 8; --q)
    if (nsps % q == 0) return q;
  return 0;
}

// the geometry and dtype checks both share (`who` opens their messages); fills the launch's samples
// and geometry
int baseband_setup(ft8_ctx* c, const void* x, int dtype, int64_t n_samples, int n_slots, int64_t slot_stride,
                   const ft8_params* p, const char* who, Baseband* B) {
  Geo g;
  std::string why;
  int rc = ft8_only(c, p, who);
  if (rc) return rc;
  rc = geometry(rate_of(p), p->bins_per_tone, p->steps_per_symbol, n_samples, &g, &why);
  if (rc) return fail(c, rc, why);
  if (dtype != FT8_F32 && dtype != FT8_I16)
    return fail(c, FT8_E_UNSUPPORTED, std::string(who) + " needs float32 or int16 samples");
  const int Q = sub_q(g.nperseg);
  if (Q == 0 || g.hop <= 0 || g.nperseg % g.hop != 0)
    return fail(c, FT8_E_UNSUPPORTED, std::string(who) + " needs nsps with a divisor in [8, 32] and hop | nsps");
  *B = Baseband{x, dtype, n_samples, slot_stride, n_slots, rate_of(p), g.nperseg, g.hop, g.nfft, p->t_lo, p->f_lo, Q};
  return FT8_OK;
}

// ---- coherent re-demodulation -------------------------------------------------------------------
// the checks ft8_coherent_llr and FT8_FLAG_COHERENT share; fills the launch's baseband
int coherent_setup(ft8_ctx* c, const void* x, int dtype, int64_t n_samples, int n_slots, int64_t slot_stride,
                   const ft8_params* p, bool multi, CohLaunch* L) {
  *L = CohLaunch{};
  const int rc = baseband_setup(c, x, dtype, n_samples, n_slots, slot_stride, p, "coherent re-demodulation", &L->b);
  if (rc) return rc;
  if (coherent_lds_bytes(L->b.nsps, L->b.Q, multi) > 64 * 1024)
    return fail(c, FT8_E_RANGE, "coherent re-demodulation: the decimation's twiddle table does not fit 64 KB of LDS");
  return FT8_OK;
}

// the drift search's settings, as ft8_coherent_drift_llr and ft8_set_coherent_drift take them
int check_coherent_drift(ft8_ctx* c, float max_rate, int n_rates) {
  if (n_rates < 1 || n_rates > 33 || n_rates % 2 == 0)
    return fail(c, FT8_E_ARG, "coherent drift: n_rates must be odd and in [1, 33]");
  if (!(max_rate >= 0.f && max_rate <= 4.f))
    return fail(c, FT8_E_ARG, "coherent drift: max_rate must be in [0, 4] Hz/s");
  return FT8_OK;
}

// the set count, as ft8_coherent_nsym_llr and ft8_set_coherent_nsym take it
int check_coherent_nsym(ft8_ctx* c, int max_nsym) {
  if (max_nsym < 1 || max_nsym > 3) return fail(c, FT8_E_ARG, "coherent nsym: max_nsym must be in [1, 3]");
  return FT8_OK;
}

// The coherent pass over one chunk, v = c->coh.at(the chunk's failed records, its first slot) (coherent.hip):
// list, k_coherent, then per set k_bp over the lists and the merge, on one claim counter as ap_pass's
// hypotheses.  L: coherent_setup's launch for the chunk's samples.
int coherent_pass(ft8_ctx* c, CohLaunch L, const CoherentRetry::View& v, int max_iterations, int counter,
                  hipStream_t s, bool f32 = false) {
  const RetryLists& l = v.lists;
  hipError_t e = launch_retry_list(l, s);
  if (e != hipSuccess) return hipfail(c, e, "coherent launch");
  L.cand = l.cand;
  L.slot_of = nullptr;
  L.count = l.count;
  L.n = l.n_slots * l.M;
  L.M = l.M;
  L.llr = v.llr;
  L.fit = v.fit;
  const CohDrift G{c->coh.drift_rate, c->coh.drift_n, v.drift};
  const CohMulti Ms{v.nsym, FT8_LDPC_N, v.set_stride, v.valid};
  if ((e = launch_coherent(L, G, Ms, s)) != hipSuccess) return hipfail(c, e, "coherent launch");
  for (int n = 0; n < v.nsym; ++n) {
    const double* llr_n = v.llr + (size_t)n * v.set_stride;
    ft8_result* res_n = v.res + (size_t)n * v.n_all;
    if ((e = bp_over_lists(c, l, llr_n, nullptr, res_n, max_iterations, counter, s, f32)) != hipSuccess)
      return hipfail(c, e, "coherent bp launch");
    const CohPass A{l, v.fit, res_n, v.drift, v.valid, n};
    if ((e = launch_coh_merge(A, s)) != hipSuccess) return hipfail(c, e, "coherent launch");
  }
  return FT8_OK;
}

// ---- a-priori retries on the coherent LLRs ------------------------------------------------------
// whether a batch with these flags runs the stage (ft8_set_coherent_ap)
bool coherent_ap_on(const ft8_ctx* c, int flags) {
  return c->cohap.on && (flags & FT8_FLAG_AP) && (flags & FT8_FLAG_COHERENT);
}

// the stage's input inside ft8_decode_batch: what the coherent pass listed in the chunk of v and left failed
CohApLaunch coherent_ap_input(const CoherentRetry::View& v) {
  const RetryLists& l = v.lists;  // CohApLaunch's members through set_stride, in order; H is the pass's
  return CohApLaunch{l.res,  l.n_slots, l.N,     l.M,     0,       v.nsym,  l.list,      l.count,
                     l.cand, l.score,   v.fit,   v.drift, v.valid, v.llr, FT8_LDPC_N,  v.set_stride};
}

// The stage over one chunk (ap.hip): A.res / n_slots / N / M / S and the coherent list, fits, validity
// bytes, drift records and LLRs are the caller's; the hypotheses, the limit and the scratch of the chunk
// that starts at slot `slot0` are filled in here.  Five launches.
int coherent_ap_pass(ft8_ctx* c, CohApLaunch A, int slot0, int max_iterations, int counter, hipStream_t s,
                     bool f32 = false) {
  A.H = (int)c->ap.hyps.size();
  for (int h = 0; h < A.H; ++h) A.hyp[h] = c->ap.hyps[h];
  A.max_hard = c->ap.max_hard;
  const CoherentApRetry::View v = c->cohap.at(A.n_slots, A.M, A.S, slot0);
  A.amax = v.amax;
  A.att = v.lists;
  A.where = v.where;
  A.llr_a = v.llr;
  A.plain = v.plain;
  A.res_a = v.res;
  hipError_t e = launch_cohap_amax(A, s);
  if (e == hipSuccess) e = launch_cohap_list(A, s);
  if (e == hipSuccess) e = launch_cohap_clamp(A, s);
  if (e != hipSuccess) return hipfail(c, e, "coherent ap launch");
  if ((e = bp_over_lists(c, A.att, v.llr, v.plain, v.res, max_iterations, counter, s, f32)) != hipSuccess)
    return hipfail(c, e, "coherent ap bp launch");
  if ((e = launch_cohap_merge(A, s)) != hipSuccess) return hipfail(c, e, "coherent ap launch");
  return FT8_OK;
}

// ---- ordered-statistics decoding ----------------------------------------------------------------
// The OSD pass over the records `failed` describes, one chunk's (osd.hip): the list of the first M records
// still failed, on the scratch of the chunk that starts at slot `slot0`, then k_osd on llr[n_slots][N][174].
int osd_pass(ft8_ctx* c, const RetryLists& failed, const double* llr, int slot0, hipStream_t s) {
  const RetryLists l = c->osd.at(failed, slot0);
  hipError_t e = launch_retry_list(l, s);
  if (e != hipSuccess) return hipfail(c, e, "osd launch");
  const OsdLaunch A{l.res, llr, l.n_slots, l.N, l.M, l.list, l.count, c->osd.order, c->osd.max_hard};  // no info
  if ((e = launch_osd(A, s)) != hipSuccess) return hipfail(c, e, "osd launch");
  return FT8_OK;
}

// ---- the retries of ft8_decode_batch ------------------------------------------------------------
// What the retry flags need before anything is searched.  Under FT8_FLAG_SUBTRACT without the setting that
// lets the retries run (ft8_set_subtract) the first of AP, coherent, OSD is refused; then AP needs
// hypotheses and the coherent pass samples it can take.
int check_retry_flags(ft8_ctx* c, const void* d_samples, int dtype, int64_t n_samples, int n_slots,
                      int64_t slot_stride, const ft8_params* p) {
  const int f = p->flags;
  if (p->protocol == FT8_PROTO_FT4 && (f & FT8_FLAG_SUBTRACT))
    return fail(c, FT8_E_UNSUPPORTED, "FT8_FLAG_SUBTRACT does not take FT4");
  const char* refused = !(f & FT8_FLAG_SUBTRACT) || c->sub_retry ? nullptr
                        : (f & FT8_FLAG_AP)                      ? "FT8_FLAG_AP"
                        : (f & FT8_FLAG_COHERENT)                ? "FT8_FLAG_COHERENT"
                        : (f & FT8_FLAG_OSD)                     ? "FT8_FLAG_OSD"
                                                                 : nullptr;
  if (refused) return fail(c, FT8_E_UNSUPPORTED, std::string(refused) + " with FT8_FLAG_SUBTRACT is not supported");
  if ((f & FT8_FLAG_AP) && c->ap.hyps.empty()) return fail(c, FT8_E_ARG, "FT8_FLAG_AP without hypotheses (ft8_set_ap)");
  if (!(f & FT8_FLAG_COHERENT)) return FT8_OK;
  CohLaunch probe;
  return coherent_setup(c, d_samples, dtype, n_samples, n_slots, slot_stride, p, c->coh.nsym > 1, &probe);
}

// the scratch of every retry the flags ask for, for n_slots slots of N candidates
int ensure_retry_scratch(ft8_ctx* c, int flags, size_t n_slots, int N) {
  int rc = FT8_OK;
  if (flags & FT8_FLAG_AP) rc = c->ap.ensure(c, n_slots, N);
  if (!rc && (flags & FT8_FLAG_COHERENT)) rc = c->coh.ensure(c, n_slots, N);
  if (!rc && coherent_ap_on(c, flags))
    rc = c->cohap.ensure(c, n_slots, c->coh.cap(N), (int)c->ap.hyps.size(), c->coh.nsym);
  if (!rc && (flags & FT8_FLAG_OSD)) rc = c->osd.ensure(c, n_slots, N);
  return rc;
}

// The retries of chunk k of n_chunks over the records `failed` describes, in order: the coherent pass on
// the chunk's samples xs, the known bits on its LLRs of what it listed and left failed, then on the STFT
// LLRs `llr` (the coherent pass leaves them alone) the AP pass and last, over what every other retry left
// failed, OSD.  Each k_bp user draws its tickets from a claim counter of its own.
int retry_passes(ft8_ctx* c, const RetryLists& failed, const double* llr, const void* xs, int dtype, int64_t n_samples,
                 int64_t slot_stride, const ft8_params* p, int slot0, int k, int n_chunks, hipStream_t s) {
  int rc;
  const bool f32 = (p->flags & FT8_FLAG_BP_F32) != 0;  // every BP launch of the batch runs k_bp32
  if (p->flags & FT8_FLAG_COHERENT) {
    CohLaunch L;
    if ((rc = coherent_setup(c, xs, dtype, n_samples, failed.n_slots, slot_stride, p, c->coh.nsym > 1, &L))) return rc;
    const CoherentRetry::View v = c->coh.at(failed, slot0);
    if ((rc = coherent_pass(c, L, v, p->max_iterations, bp_counter(kChunkCoherent, k, n_chunks), s, f32))) return rc;
    if (coherent_ap_on(c, p->flags) &&
        (rc = coherent_ap_pass(c, coherent_ap_input(v), slot0, p->max_iterations,
                               bp_counter(kChunkCoherentAp, k, n_chunks), s, f32)))
      return rc;
  }
  if ((p->flags & FT8_FLAG_AP) &&
      (rc = ap_pass(c, failed, llr, slot0, p->max_iterations, nullptr, bp_counter(kChunkAp, k, n_chunks), s,
                    p->protocol, f32)))
    return rc;
  if ((p->flags & FT8_FLAG_OSD) && (rc = osd_pass(c, failed, llr, slot0, s))) return rc;
  return FT8_OK;
}

// ft8_ap_decode and ft8_coherent_ap_decode: records without slot structure, one list of n, retried with the
// context's hypotheses on n_sets LLR sets each.  The checks, the caller's claim counter, the stage's
// scratch (`scratch`), hard = -1 throughout, then `pass`.
template <typename Scratch, typename Pass>
int ap_stage_call(ft8_ctx* c, const double* d_llr, int n_sets, ft8_result* d_res, int n, int16_t* d_hard, hipStream_t s,
                  Scratch&& scratch, Pass&& pass) {
  if (!c || n < 0 || (n > 0 && (!d_llr || !d_res))) return fail(c, FT8_E_ARG, "bad argument");
  if (n_sets < 1 || n_sets > 3) return fail(c, FT8_E_ARG, "coherent ap: n_sets must be in [1, 3]");
  if (c->ap.hyps.empty()) return fail(c, FT8_E_ARG, "no hypotheses set (ft8_set_ap)");
  if (n == 0) return FT8_OK;
  DeviceGuard dg(c->device);
  int rc;
  if ((rc = ensure_work(c, 1, s))) return rc;
  if ((rc = scratch())) return rc;
  if (d_hard) {
    const hipError_t e = hipMemsetAsync(d_hard, 0xFF, sizeof(int16_t) * (size_t)n, s);  // -1 throughout
    if (e != hipSuccess) return hipfail(c, e, "memset");
  }
  return pass();
}

int decode_pass(ft8_ctx* c, const void* d_samples, int dtype, int64_t n_samples, int32_t n_slots,
                int64_t slot_stride, const ft8_params* p, ft8_result* d_out, int32_t* d_counts, int32_t cap,
                hipStream_t s) {
  const int T = p->t_hi - p->t_lo, F = p->f_hi - p->f_lo;
  const bool f64 = is_f64_dtype(dtype);
  const size_t esz = f64 ? 8 : 4;
  const int N = p->max_candidates;
  Grid gr = grid_of(T, F, p);
  int rc;

  // slot chunks, each an independent STFT -> score/select -> LLR -> BP -> compact chain; chunks
  // alternate over the internal streams so one chunk's BP (FP64 VALU) overlaps the next chunk's
  // STFT / score (LDS, HBM)
  const int csz = (c->n_streams > 0 && c->chunk_slots > 0) ? c->chunk_slots : n_slots;
  const int n_chunks = (n_slots + csz - 1) / csz;
  const int n_str = (c->n_streams > 0 && n_chunks > 1) ? std::min(c->n_streams, n_chunks) : 0;
  const int f = p->flags;
  if ((rc = ensure_work(c, bp_counters(f & FT8_FLAG_AP, f & FT8_FLAG_COHERENT, coherent_ap_on(c, f), n_chunks), s)))
    return rc;
  hipError_t e = hipSuccess;
  if (n_str > 0) {
    while ((int)c->streams.size() < n_str) {
      hipStream_t st;
      if ((e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking)) != hipSuccess) return hipfail(c, e, "stream");
      c->streams.push_back(st);
      hipEvent_t ev;
      if ((e = hipEventCreateWithFlags(&ev, hipEventDisableTiming)) != hipSuccess) return hipfail(c, e, "event");
      c->joins.push_back(ev);
    }
    if (!c->fork && (e = hipEventCreateWithFlags(&c->fork, hipEventDisableTiming)) != hipSuccess)
      return hipfail(c, e, "event");
    if ((e = hipEventRecord(c->fork, s)) != hipSuccess) return hipfail(c, e, "fork");
    for (int i = 0; i < n_str; ++i)
      if ((e = hipStreamWaitEvent(c->streams[i], c->fork, 0)) != hipSuccess) return hipfail(c, e, "fork wait");
  }
  const size_t in_esz = dtype == FT8_I16 ? 2 : dtype == FT8_F32 ? 4 : (dtype == FT8_F64 || dtype == FT8_C64) ? 8 : 16;
  for (int k = 0; k < n_chunks; ++k) {
    const int c0 = k * csz, ns = std::min(csz, n_slots - c0);
    hipStream_t cs = n_str > 0 ? c->streams[k % n_str] : s;
    char* wf = c->wf.as<char>() + esz * (size_t)c0 * T * F;
    const char* xs = (const char*)d_samples + in_esz * (size_t)c0 * slot_stride;
    if ((rc = do_stft(c, xs, dtype, n_samples, ns, slot_stride, p, wf, cs))) return rc;
    int32_t* cand = c->cand.as<int32_t>() + 2 * (size_t)c0 * N;
    double* cand_score = c->cand_score.as<double>() + (size_t)c0 * N;
    int32_t* cand_count = c->cand_count.as<int32_t>() + c0;
    // float32 scores (sc.tie): equal scores keep the select order through LLR/BP and are reordered
    // by k_compact after k_llr's first workgroups replayed the reference heap
    const SelScratch sc = sel_scratch_at(c, c0, gr, N, f64);
    if ((rc = sync_select_core(c, wf, f64, ns, T, F, p, cand, cand_score, cand_count, sc, 1, cs))) return rc;
    BpLaunch B{};
    B.wf = wf;
    B.wf_f64 = f64;
    B.T = T;
    B.F = F;
    B.sps = p->steps_per_symbol;
    B.bpt = p->bins_per_tone;
    B.cand = cand;
    B.cand_score = cand_score;
    B.cand_count = cand_count;
    B.N = N;
    B.n_slots = ns;
    B.slot0 = c0;
    B.n_items = ns * N;
    B.mode = 0;
    B.normalize = 1;
    B.max_iterations = p->max_iterations;
    B.llr_out = c->llr.as<double>() + (size_t)FT8_LDPC_N * c0 * N;
    B.llr_in = B.llr_out;
    B.res = c->res_all.as<ft8_result>() + (size_t)c0 * N;
    B.f32 = (f & FT8_FLAG_BP_F32) ? 1 : 0;
    wire_bp_counters(c, B, bp_counter(kChunkBp, k, n_chunks), c->bp_waves);
    B.tie = sc.tie;
    B.warn = sc.warn;
    const bool ft4 = p->protocol == FT8_PROTO_FT4;
    if ((rc = timed_launch(c, kLlr, cs, "llr launch", [&] { return ft4 ? launch_llr4(B, cs) : launch_llr(B, cs); })))
      return rc;
    if ((rc = timed_launch(c, kBp, cs, "bp launch", [&] { return run_bp(B, cs); }))) return rc;
    // the tie order k_compact applies permutes positions, not records, so the coherent and AP passes
    // work on res_all as it is; the coherent pass leaves c->llr alone, so AP sees the STFT LLRs
    RetryLists failed{};
    failed.res = B.res;
    failed.cand_count = cand_count;
    failed.cand_in = cand;
    failed.score_in = cand_score;
    failed.n_slots = ns;
    failed.N = N;
    if ((rc = retry_passes(c, failed, B.llr_in, xs, dtype, n_samples, slot_stride, p, c0, k, n_chunks, cs))) return rc;
    CompactLaunch C{};
    C.res = B.res;
    C.cand_count = cand_count;
    C.n_slots = ns;
    C.N = N;
    C.out = d_out ? d_out + (size_t)c0 * cap : nullptr;
    C.counts = d_counts + c0;
    C.cap = cap;
    C.warn = sc.warn;
    C.tie = sc.tie;
    c->last_bp = B;
    c->last_compact = C;
    if ((rc = timed_launch(c, kCompact, cs, "compact launch", [&] { return launch_compact(C, cs); }))) return rc;
    // FT4: BP, the retries and the tail worked on scrambled bits; the rows handed out carry the message
    if (ft4 && C.out && (e = launch_ft4_unscramble(C.out, ns * cap, C.counts, cap, cs)) != hipSuccess)
      return hipfail(c, e, "unscramble launch");
  }
  for (int i = 0; i < n_str; ++i) {
    if ((e = hipEventRecord(c->joins[i], c->streams[i])) != hipSuccess) return hipfail(c, e, "join");
    if ((e = hipStreamWaitEvent(s, c->joins[i], 0)) != hipSuccess) return hipfail(c, e, "join wait");
  }
  // a replayed k_bp would overwrite the rescued records
  // (and the descramble of an FT4 batch is an involution, not idempotent)
  c->replay_ok = n_chunks == 1 && !(f & (FT8_FLAG_AP | FT8_FLAG_COHERENT | FT8_FLAG_OSD)) && p->protocol == FT8_PROTO_FT8;
  return FT8_OK;
}

// cumulative GFSK frequency pulse P[0 .. 3 nsps] of the transmit chain (tx_device.h), double and
// float, built once per (nsps, BT): p(i) = gauss_window_generator(BT, (i - 1.5 nsps) / nsps)
// (modulator.py:20-25, 33-34; BT = 2.0 for FT8, 1.0 for FT4), P[i + 1] = P[i] + p(i)
int gfsk_tables(ft8_ctx* c, int nsps, double bt) {
  if (c->gfsk_nsps == nsps && c->gfsk_bt == bt && c->gfsk_P.p) return FT8_OK;
  // the tables are rewritten in place: whatever still reads the old ones (a protocol switch on one
  // context) finishes first
  if (c->gfsk_P.p && hipDeviceSynchronize() != hipSuccess) return fail(c, FT8_E_HIP, "gfsk table sync");
  const int n = 3 * nsps + 1;
  int rc;
  if ((rc = ensure(c, c->gfsk_P, sizeof(double) * n))) return rc;
  if ((rc = ensure(c, c->gfsk_Pf, sizeof(float) * n))) return rc;
  std::vector<double> P(n);
  std::vector<float> Pf(n);
  const double k = M_PI * std::sqrt(2.0 / std::log(2.0));
  P[0] = 0.0;
  for (int i = 0; i < 3 * nsps; ++i) {
    const double t = ((double)i - 1.5 * (double)nsps) / (double)nsps;
    const double w = 0.5 * (std::erf(k * bt * (t + 0.5)) - std::erf(k * bt * (t - 0.5)));
    P[i + 1] = P[i] + w;
  }
  for (int i = 0; i < n; ++i) Pf[i] = (float)P[i];
  hipError_t e = hipMemcpy(c->gfsk_P.p, P.data(), sizeof(double) * n, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(c->gfsk_Pf.p, Pf.data(), sizeof(float) * n, hipMemcpyHostToDevice);
  if (e != hipSuccess) return hipfail(c, e, "gfsk table upload");
  c->gfsk_nsps = nsps;
  c->gfsk_bt = bt;
  return FT8_OK;
}

int subtract_core(ft8_ctx* c, const void* x, int dtype, float* resid, int64_t n_samples, int n_slots,
                  int64_t x_stride, int64_t r_stride, const ft8_params* p, const ft8_result* res,
                  const int32_t* counts, int cap, hipStream_t s, const int32_t* first, int first_stride) {
  // FT8_FLAG_SUBTRACT, the one caller whose strides can differ, has passed the geometry and dtype checks
  if (x_stride != r_stride) return fail(c, FT8_E_ARG, "residual and sample strides differ");
  SubLaunch L{};
  int rc = baseband_setup(c, x, dtype, n_samples, n_slots, x_stride, p, "subtraction", &L.b);
  if (rc) return rc;
  c->sub_slots = c->sub_cap = -1;  // no valid fits until this subtraction has been launched
  if ((rc = gfsk_tables(c, L.b.nsps))) return rc;
  if ((rc = ensure(c, c->sub_est, sub_est_bytes() * (size_t)n_slots * (size_t)(cap > 0 ? cap : 1)))) return rc;
  if ((rc = ensure(c, c->sub_list, sizeof(int32_t) * (size_t)n_slots * (size_t)(cap + 1)))) return rc;
  L.residual = resid;
  L.res = res;
  L.counts = counts;
  L.cap = cap;
  L.P = c->gfsk_P.as<const double>();
  L.Pf = c->gfsk_Pf.as<const float>();
  L.est = c->sub_est.p;
  L.list = c->sub_list.as<int32_t>();
  L.first = first;
  L.first_stride = first_stride;
  if ((rc = timed_launch(c, kSubEst, s, "subtract launch", [&] { return launch_sub_est(L, s); }))) return rc;
  if ((rc = timed_launch(c, kSubApply, s, "subtract launch", [&] { return launch_sub_apply(L, s); }))) return rc;
  c->sub_slots = n_slots;
  c->sub_cap = cap;
  return FT8_OK;
}

// ---- frequency-drift correction ----------------------------------------------------------------
// kept f >= 0 bins of a two-sided spectrum after fftshift (frequency_correction.py:198-200)
int drift_bins(int nfft) { return (nfft + 1) / 2; }

int stft_argmax_core(ft8_ctx* c, const void* x, int dtype, int64_t n_samples, int n_slots, int64_t stride,
                     const ft8_params* p, int32_t* idx, hipStream_t s) {
  StftLaunch L;
  bool launch;
  int rc = make_stft_launch(c, p, dtype, n_samples, n_slots, stride, StftUse::Argmax, &L, &launch);
  if (rc || !launch) return rc;
  L.samples = x;
  L.argmax = idx;
  const size_t frames = (size_t)n_slots * (size_t)(p->t_hi - p->t_lo);
  if (L.plan.dft || L.plan.blue) {
    // the direct DFT and the chirp-z path write the dB rows, then reduce each to its argmax: stage
    // them in wf
    if ((rc = ensure(c, c->wf, frames * (p->f_hi - p->f_lo) * (is_f64_dtype(dtype) ? 8 : 4)))) return rc;
    L.out = c->wf.p;
  }
  if (dtype != FT8_C128 || !stftc3840_eligible(L)) {
    c->screen_frames = 0;
  } else {
    if ((rc = ensure(c, c->screen, sizeof(int32_t) * (frames + 1)))) return rc;
    L.screen_count = c->screen.as<int32_t>();
    L.screen_list = L.screen_count + 1;
    // the screening pass transforms in float32: its own twiddles and window
    FftPlan fp;
    if ((rc = get_plan(c, L.nfft, true, false, L.nperseg, &fp))) return rc;
    WinEntry* wf32 = nullptr;
    if ((rc = get_window(c, L.nperseg, false, &wf32))) return rc;
    if (fp.P != 3840 || fp.dft || fp.blue) return fail(c, FT8_E_UNSUPPORTED, "float32 screening plan");
    L.screen_tw = fp.tw;
    L.screen_window = wf32->w.p;
    c->screen_frames = (int64_t)frames;
  }
  return timed_launch(c, kDriftStftArgmax, s, "stft argmax launch", [&] { return launch_stft(L, s); });
}

int check_drift_params(ft8_ctx* c, const ft8_drift_params* p) {
  if (p->bins_per_tone <= 0 || p->steps_per_symbol <= 0) return fail(c, FT8_E_ARG, "bins_per_tone and steps_per_symbol must be positive");
  if (p->sample_rate <= 0 || p->sample_rate != std::floor(p->sample_rate) || p->sample_rate > 2e9)
    return fail(c, FT8_E_UNSUPPORTED, "sample_rate must be a positive integral number of Hz");
  const int w = p->window_size_factor * p->steps_per_symbol;
  if (w < 1) return fail(c, FT8_E_ARG, "window_size_factor * steps_per_symbol must be >= 1");
  if (w > kDriftMaxWindow) return fail(c, FT8_E_RANGE, "continuity window exceeds " + std::to_string(kDriftMaxWindow));
  if (p->nsync_sym < 1 || p->nsync_sym > 7) return fail(c, FT8_E_ARG, "nsync_sym must be in [1, 7] (the Costas array has 7 tones)");
  if (p->ndata_sym < 0) return fail(c, FT8_E_ARG, "ndata_sym must be >= 0");
  if (3 * (p->nsync_sym - 1) * p->steps_per_symbol > drift_max_points())
    return fail(c, FT8_E_RANGE, "sync regression points exceed the compiled limit");
  return FT8_OK;
}

// three_sync_correlation_seq (frequency_correction.py:386-407), NumPy's operation order
int drift_template(ft8_ctx* c, const ft8_drift_params* p) {
  const int tosr = p->steps_per_symbol, ns = p->nsync_sym, nd = p->ndata_sym;
  if (c->tmpl_len > 0 && c->tmpl_key[0] == tosr && c->tmpl_key[1] == ns && c->tmpl_key[2] == nd) return FT8_OK;
  const int sps2 = 2 * tosr;
  static const int costas[7] = {3, 1, 4, 0, 6, 5, 2};
  double seq[7];
  for (int k = 0; k < 7; ++k) seq[k] = (double)(costas[k] + 1) - 4.0;  // - np.mean(...) = 4.0 exactly
  // t = np.linspace(-1, 1, sps2 + 1); gfsk_shape = gfsk_pulse(2.0, t)  (:27-40)
  const double step = 2.0 / (double)sps2;
  const double kk = M_PI * std::sqrt(2.0 / std::log(2.0));
  const double kb = kk * 2.0;
  std::vector<double> shape(sps2 + 1);
  for (int j = 0; j <= sps2; ++j) {
    const double t = j == sps2 ? 1.0 : (double)j * step + -1.0;
    shape[j] = 0.5 * (std::erf(kb * (t + 0.5)) - std::erf(kb * (t - 0.5)));
  }
  const int L1 = (ns - 1) * tosr + sps2 + 1;
  std::vector<double> one(L1, 0.0);
  for (int k = 0; k < ns; ++k)
    for (int j = 0; j <= sps2; ++j) one[k * tosr + j] += shape[j] * seq[k];
  const int L3 = (3 * ns + nd - 1) * tosr + 1 + sps2;
  if (L3 > drift_max_template()) return fail(c, FT8_E_RANGE, "sync template exceeds the compiled limit");
  std::vector<double> three(L3, 0.0);
  for (int i = 0; i < 3; ++i) {
    const int s0 = i * (ns + nd / 2) * tosr;
    if (s0 + L1 > L3) return fail(c, FT8_E_ARG, "sync blocks do not fit the template (the reference raises ValueError)");
    for (int j = 0; j < L1; ++j) three[s0 + j] = one[j];
  }
  int rc = ensure(c, c->drift_tmpl, sizeof(double) * L3);
  if (rc) return rc;
  hipError_t e = hipMemcpy(c->drift_tmpl.p, three.data(), sizeof(double) * L3, hipMemcpyHostToDevice);
  if (e != hipSuccess) return hipfail(c, e, "template upload");
  c->tmpl_key[0] = tosr;
  c->tmpl_key[1] = ns;
  c->tmpl_key[2] = nd;
  c->tmpl_len = L3;
  return FT8_OK;
}

int drift_fit_core(ft8_ctx* c, int stage, const int32_t* idx, int n_slots, int T, int F, const ft8_drift_params* p,
                   ft8_drift_result* res, double* metric, int32_t* segments, int max_segments, hipStream_t s) {
  int rc = check_drift_params(c, p);
  if (rc) return rc;
  if (T > kDriftMaxT) return fail(c, FT8_E_RANGE, "more than " + std::to_string(kDriftMaxT) + " frames per signal");
  if (F < 1 || F > 8192) return fail(c, FT8_E_RANGE, "freq_bins must be in [1, 8192]");
  DriftFitLaunch L{};
  L.idx = idx;
  L.n_slots = n_slots;
  L.T = T;
  L.F = F;
  L.p = *p;
  L.res = res;
  L.metric = metric;
  L.segments = segments;
  L.max_segments = segments ? max_segments : 0;
  if (stage == 2) {
    if ((rc = drift_template(c, p))) return rc;
    L.tmpl = c->drift_tmpl.as<const double>();
    L.n_tmpl = c->tmpl_len;
  }
  return timed_launch(c, kDriftFit, s, "drift fit launch", [&] { return launch_drift_fit(stage, L, s); });
}

// ---- signal report ---------------------------------------------------------------------------------
// 10 log10(enbw_hz / 2500): the equivalent noise bandwidth of the STFT's periodic Hann window with
// scaling='spectrum' is 1.5 fs / nperseg; the report is the SNR in 2500 Hz
double snr_bw_db(double fs, int nperseg) { return 10.0 * std::log10(1.5 * fs / (double)nperseg / 2500.0); }

// ft8_decode_batch succeeded: c->wf holds the batch's waterfall [n_slots][T][F]
void remember_snr_batch(ft8_ctx* c, const ft8_params* p, const Geo& g, int n_slots, int T, int F, int cap, bool f64) {
  c->snr_batch = {n_slots, T, F, cap, f64, (p->flags & FT8_FLAG_SUBTRACT) != 0, snr_bw_db(rate_of(p), g.nperseg),
                  p->steps_per_symbol, p->bins_per_tone, p->protocol == FT8_PROTO_FT4};
  c->snr_ok = true;
}

int check_snr_records(ft8_ctx* c, const ft8_result* d_records, const int32_t* d_counts, int64_t n_slots, int64_t cap,
                      const ft8_snr_rec* d_out) {
  if (!d_records || !d_out) return fail(c, FT8_E_ARG, "null records or output");
  if (n_slots * cap > INT32_MAX) return fail(c, FT8_E_RANGE, "n_slots * cap exceeds 2^31 records");
  if (((uintptr_t)d_records & 7) || ((uintptr_t)d_out & 7) || ((uintptr_t)d_counts & 3))
    return fail(c, FT8_E_ARG, "records and reports must be 8-byte, counts 4-byte aligned");
  return FT8_OK;
}

int noise_floor_rank(double q, int F) { return (int)std::floor(q * (double)(F - 1)); }

}  // namespace

// ============================================================================================
extern "C" {

int ft8_abi_version(void) { return FT8HIP_ABI_VERSION; }

int ft8_limits(int32_t* max_candidates, int32_t* max_fft_real, int32_t* max_fft_complex) {
  if (max_candidates) *max_candidates = kMaxCandidates;
  if (max_fft_real) *max_fft_real = kMaxFftReal;
  if (max_fft_complex) *max_fft_complex = kMaxFftComplex;
  return FT8_OK;
}

int ft8_create(int device, ft8_ctx** out) {
  if (!out) return FT8_E_ARG;
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) return FT8_E_HIP;
  if (device < 0 || device >= n) return FT8_E_ARG;
  ft8_ctx* c = new (std::nothrow) ft8_ctx();
  if (!c) return FT8_E_NOMEM;
  c->device = device;
  *out = c;
  return FT8_OK;
}

int ft8_destroy(ft8_ctx* c) {
  if (!c) return FT8_OK;
  {
    DeviceGuard dg(c->device);
    for (auto& t : c->pending) {
      (void)hipEventDestroy(t.a);
      (void)hipEventDestroy(t.b);
    }
    for (auto ev : c->pool) (void)hipEventDestroy(ev);
    for (auto st : c->streams) (void)hipStreamDestroy(st);
    for (auto ev : c->joins) (void)hipEventDestroy(ev);
    if (c->fork) (void)hipEventDestroy(c->fork);
    if (c->last_done) (void)hipEventDestroy(c->last_done);
    delete c;  // every DevBuf of the context (scratch, plans, windows) is freed here, on its device
  }
  return FT8_OK;
}

const char* ft8_last_error(const ft8_ctx* c) { return c ? c->err.c_str() : "null context"; }

int ft8_geometry(int32_t fs, int32_t bpt, int32_t sps, int64_t n, int32_t* nperseg, int32_t* hop, int32_t* nfft,
                 int32_t* frames) {
  return ft8_geometry_hz((double)fs, bpt, sps, n, nperseg, hop, nfft, frames);
}

int ft8_geometry_hz(double fs, int32_t bpt, int32_t sps, int64_t n, int32_t* nperseg, int32_t* hop, int32_t* nfft,
                    int32_t* frames) {
  Geo g;
  std::string why;
  int rc = geometry(fs, bpt, sps, n, &g, &why);
  if (rc) return rc;
  if (nperseg) *nperseg = g.nperseg;
  if (hop) *hop = g.hop;
  if (nfft) *nfft = g.nfft;
  if (frames) *frames = g.frames;
  return FT8_OK;
}

int ft8_stft(ft8_ctx* c, const void* d_samples, int dtype, int64_t n_samples, int32_t n_slots, int64_t slot_stride,
             const ft8_params* p, void* d_wf, void* stream) {
  StreamOrder order_(c, (hipStream_t)stream);
  if (c) c->replay_ok = c->snr_ok = false;
  if (!c || !p || (!d_samples && n_slots > 0) || (!d_wf && n_slots > 0)) return fail(c, FT8_E_ARG, "null argument");
  DeviceGuard dg(c->device);
  return do_stft(c, d_samples, dtype, n_samples, n_slots, slot_stride, p, d_wf, (hipStream_t)stream);
}

int ft8_stft_screen_stats(ft8_ctx* c, int64_t* frames_redone, int64_t* frames) {
  if (!c || !frames_redone || !frames) return fail(c, FT8_E_ARG, "null argument");
  *frames_redone = 0;
  *frames = c->screen_frames;
  if (c->screen_frames == 0) return FT8_OK;
  DeviceGuard dg(c->device);
  int32_t n = 0;
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(&n, c->screen.p, sizeof(int32_t), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return hipfail(c, e, "screen count");
  *frames_redone = n;
  return FT8_OK;
}

int ft8_stft_method(ft8_ctx* c, int32_t fs, int32_t bpt, int32_t sps, int64_t n, int dtype) {
  if (!c) return FT8_E_ARG;
  if (dtype < FT8_F32 || dtype > FT8_I16) return fail(c, FT8_E_ARG, "unknown sample dtype");
  ft8_params p{};
  p.sample_rate = fs;
  p.bins_per_tone = bpt;
  p.steps_per_symbol = sps;
  DeviceGuard dg(c->device);
  StftLaunch L;
  bool launch;
  // stride 2: the packed kernel's only stride condition (even) is the caller's
  int rc = make_stft_launch(c, &p, dtype, n, 1, 2, StftUse::Method, &L, &launch);
  if (rc) return rc;
  if (L.plan.blue) return FT8_STFT_CHIRPZ;
  if (L.plan.dft) return FT8_STFT_DFT;
  return stft3840_eligible(L) ? FT8_STFT_PACKED3840 : FT8_STFT_STOCKHAM;
}

int ft8_sync_select(ft8_ctx* c, const void* d_wf, int wf_f64, int32_t n_slots, int32_t T, int32_t F,
                    const ft8_params* p, int32_t* d_cand, double* d_cand_score, int32_t* d_cand_count,
                    void* d_scores, void* stream) {
  StreamOrder order_(c, (hipStream_t)stream);
  if (c) c->replay_ok = c->snr_ok = false;
  if (!c || !p || !d_cand_count) return fail(c, FT8_E_ARG, "null argument");
  if (T < 0 || F < 0 || n_slots < 0) return fail(c, FT8_E_ARG, "negative size");
  DeviceGuard dg(c->device);
  return do_sync_select(c, d_wf, wf_f64, n_slots, T, F, p, d_cand, d_cand_score, d_cand_count, d_scores,
                        (hipStream_t)stream);
}

int ft8_sync_score(ft8_ctx* c, const void* d_wf, int wf_f64, int32_t T, int32_t F, int32_t sps, int32_t bpt,
                   const int32_t* d_cand, int32_t n, void* d_out, int32_t* d_err, void* stream) {
  if (c) c->replay_ok = c->snr_ok = false;
  if (!c || n < 0 || (n > 0 && (!d_wf || !d_cand || !d_out || !d_err))) return fail(c, FT8_E_ARG, "bad argument");
  if (T <= 0 || F <= 0 || sps <= 0 || bpt <= 0) return fail(c, FT8_E_ARG, "empty waterfall or bad oversampling");
  DeviceGuard dg(c->device);
  hipError_t e = launch_score_list(d_wf, wf_f64, T, F, sps, bpt, d_cand, n, d_out, d_err, (hipStream_t)stream);
  return e == hipSuccess ? FT8_OK : hipfail(c, e, "score launch");
}

int ft8_llr(ft8_ctx* c, const void* d_wf, int wf_f64, int32_t T, int32_t F, int32_t sps, int32_t bpt,
            const int32_t* d_cand, int32_t n, int normalize, double* d_llr, void* stream) {
  if (c) c->replay_ok = c->snr_ok = false;
  if (!c || !d_llr || (!d_cand && n > 0) || sps <= 0 || bpt <= 0) return fail(c, FT8_E_ARG, "bad argument");
  if (n <= 0) return FT8_OK;
  DeviceGuard dg(c->device);
  BpLaunch L{};
  L.wf = d_wf;
  L.wf_f64 = wf_f64;
  L.T = T;
  L.F = F;
  L.sps = sps;
  L.bpt = bpt;
  L.cand = d_cand;
  L.n_items = n;
  L.mode = 1;
  L.normalize = normalize;
  L.llr_out = d_llr;
  hipStream_t s = (hipStream_t)stream;
  return timed_launch(c, kLlr, s, "llr launch", [&] { return launch_llr(L, s); });
}

int ft8_normalize(ft8_ctx* c, const double* d_in, int32_t n, double* d_out, void* stream) {
  if (c) c->replay_ok = c->snr_ok = false;
  if (!c || (n > 0 && (!d_in || !d_out))) return fail(c, FT8_E_ARG, "bad argument");
  if (n <= 0) return FT8_OK;
  DeviceGuard dg(c->device);
  BpLaunch L{};
  L.mode = 2;
  L.llr_in = d_in;
  L.n_items = n;
  L.normalize = 1;
  L.llr_out = d_out;
  hipStream_t s = (hipStream_t)stream;
  return timed_launch(c, kLlr, s, "normalize launch", [&] { return launch_llr(L, s); });
}

// ft8_bp and ft8_bp_f32: one stage call, the kernel and its grid residency apart
static int bp_stage_call(ft8_ctx* c, const double* d_llr, int32_t n, int32_t max_iterations, uint8_t* d_plain,
                  ft8_result* d_res, void* stream, bool f32) {
  StreamOrder order_(c, (hipStream_t)stream);
  if (c) c->replay_ok = c->snr_ok = false;
  if (!c || (!d_llr && n > 0)) return fail(c, FT8_E_ARG, "bad argument");
  if (n <= 0) return FT8_OK;
  DeviceGuard dg(c->device);
  int rc;
  if ((rc = ensure_work(c, 1, (hipStream_t)stream))) return rc;
  BpLaunch L{};
  L.mode = 2;
  L.llr_in = d_llr;
  L.n_items = n;
  L.normalize = 0;
  L.max_iterations = max_iterations;
  L.plain_out = d_plain;
  L.res = d_res;
  L.f32 = f32 ? 1 : 0;
  // ft8_bp: BpLaunch's default residency, not the pipeline's; ft8_bp_f32: the pipeline's (ft8_set_pipeline)
  wire_bp_counters(c, L, bp_counter(kCallerBp, 0, 0), f32 ? c->bp_waves : L.grid_waves);
  hipStream_t s = (hipStream_t)stream;
  return timed_launch(c, kBp, s, "bp launch", [&] { return run_bp(L, s); });
}

int ft8_bp(ft8_ctx* c, const double* d_llr, int32_t n, int32_t max_iterations, uint8_t* d_plain, ft8_result* d_res,
           void* stream) {
  return bp_stage_call(c, d_llr, n, max_iterations, d_plain, d_res, stream, false);
}

int ft8_bp_f32(ft8_ctx* c, const double* d_llr, int32_t n, int32_t max_iterations, uint8_t* d_plain,
               ft8_result* d_res, void* stream) {
  return bp_stage_call(c, d_llr, n, max_iterations, d_plain, d_res, stream, true);
}

int ft8_set_ap(ft8_ctx* c, const ft8_ap_hyp* hyps, int32_t n, int32_t max_hard_errors) {
  if (!c || n < 0 || (n > 0 && !hyps)) return fail(c, FT8_E_ARG, "bad argument");
  if (n > FT8_AP_MAX_HYP) return fail(c, FT8_E_RANGE, "more than " + std::to_string(FT8_AP_MAX_HYP) + " hypotheses");
  if (max_hard_errors < 0 || max_hard_errors > FT8_LDPC_N) return fail(c, FT8_E_ARG, "max_hard_errors outside [0, 174]");
  for (int i = 0; i < n; ++i)
    if ((hyps[i].mask[9] | hyps[i].value[9]) & 7) return fail(c, FT8_E_ARG, "a hypothesis bit outside the 77 message bits");
  c->ap.hyps.assign(hyps, hyps + n);
  c->ap.max_hard = max_hard_errors;
  return FT8_OK;
}

int ft8_ap_decode(ft8_ctx* c, const double* d_llr, ft8_result* d_res, int32_t n, int32_t max_iterations,
                  int16_t* d_hard, void* stream) {
  StreamOrder order_(c, (hipStream_t)stream);
  if (c) c->replay_ok = c->snr_ok = false;
  hipStream_t s = (hipStream_t)stream;
  return ap_stage_call(
      c, d_llr, 1, d_res, n, d_hard, s, [&] { return c->ap.ensure(c, 1, n); },
      [&] {  // no candidate positions or scores
        RetryLists failed{};
        failed.res = d_res;
        failed.n_slots = 1;
        failed.N = n;
        return ap_pass(c, failed, d_llr, 0, max_iterations, d_hard, bp_counter(kCallerBp, 0, 0), s);
      });
}

int ft8_set_osd(ft8_ctx* c, int32_t order, int32_t max_per_slot, int32_t max_hard_errors) {
  if (!c) return FT8_E_ARG;
  if (order < 0 || order > 2) return fail(c, FT8_E_ARG, "osd: order must be in [0, 2]");
  if (max_per_slot < 0) return fail(c, FT8_E_ARG, "osd: max_per_slot must be >= 0");
  if (max_hard_errors < 0 || max_hard_errors > FT8_LDPC_N) return fail(c, FT8_E_ARG, "osd: max_hard_errors outside [0, 174]");
  c->osd.order = order;
  c->osd.max = max_per_slot;
  c->osd.max_hard = max_hard_errors;
  return FT8_OK;
}

int ft8_osd_decode(ft8_ctx* c, const double* d_llr, ft8_result* d_res, int32_t n, ft8_osd_rec* d_info,
                   uint8_t* d_codeword, void* stream) {
  StreamOrder order_(c, (hipStream_t)stream);
  if (c) c->replay_ok = c->snr_ok = false;
  if (!c || n < 0 || (n > 0 && (!d_llr || !d_res))) return fail(c, FT8_E_ARG, "bad argument");
  if (n == 0) return FT8_OK;
  DeviceGuard dg(c->device);
  // records without slot structure: one list of every record
  OsdLaunch A{};
  A.res = d_res;
  A.llr = d_llr;
  A.n_slots = 1;
  A.N = A.M = n;
  A.order = c->osd.order;
  A.max_hard = c->osd.max_hard;
  A.info = d_info;
  A.codeword = d_codeword;
  const hipError_t e = launch_osd(A, (hipStream_t)stream);
  return e == hipSuccess ? FT8_OK : hipfail(c, e, "osd launch");
}

int ft8_set_coherent(ft8_ctx* c, int32_t max_per_slot) {
  if (!c || max_per_slot < 0) return fail(c, FT8_E_ARG, "bad argument");
  c->coh.max = max_per_slot;
  return FT8_OK;
}

int ft8_set_coherent_drift(ft8_ctx* c, float max_rate_hz_per_s, int32_t n_rates) {
  if (!c) return FT8_E_ARG;
  const int rc = check_coherent_drift(c, max_rate_hz_per_s, n_rates);
  if (rc) return rc;
  c->coh.drift_rate = max_rate_hz_per_s;
  c->coh.drift_n = n_rates;
  return FT8_OK;
}

int ft8_set_coherent_nsym(ft8_ctx* c, int32_t max_nsym) {
  if (!c) return FT8_E_ARG;
  const int rc = check_coherent_nsym(c, max_nsym);
  if (rc) return rc;
  c->coh.nsym = max_nsym;
  return FT8_OK;
}

int ft8_set_coherent_ap(ft8_ctx* c, int32_t on) {
  if (!c) return FT8_E_ARG;
  if (on != 0 && on != 1) return fail(c, FT8_E_ARG, "coherent ap: on must be 0 or 1");
  c->cohap.on = on;
  return FT8_OK;
}

int ft8_coherent_ap_decode(ft8_ctx* c, const double* d_llr, int32_t n_sets, const uint8_t* d_valid, ft8_result* d_res,
                           int32_t n, int32_t max_iterations, int16_t* d_hard, void* stream) {
  StreamOrder order_(c, (hipStream_t)stream);
  if (c) c->replay_ok = c->snr_ok = false;
  hipStream_t s = (hipStream_t)stream;
  return ap_stage_call(
      c, d_llr, n_sets, d_res, n, d_hard, s, [&] { return c->cohap.ensure(c, 1, n, (int)c->ap.hyps.size(), n_sets); },
      [&] {  // position j is record j, every fit valid, no drift
        CohApLaunch A{};
        A.res = d_res;
        A.n_slots = 1;
        A.N = A.M = n;
        A.S = n_sets;
        A.valid = d_valid;
        A.llr = d_llr;
        A.pos_stride = (int64_t)n_sets * FT8_LDPC_N;
        A.set_stride = FT8_LDPC_N;
        A.hard = d_hard;
        return coherent_ap_pass(c, A, 0, max_iterations, bp_counter(kCallerBp, 0, 0), s);
      });
}

int ft8_coherent_llr(ft8_ctx* c, const void* d_samples, int dtype, int64_t n_samples, int32_t n_slots,
                     int64_t slot_stride, const ft8_params* p, const int32_t* d_cand, const int32_t* d_slot_of,
                     int32_t n, double* d_llr_out, ft8_coh_fit* d_fit_out, void* stream) {
  return ft8_coherent_drift_llr(c, d_samples, dtype, n_samples, n_slots, slot_stride, p, d_cand, d_slot_of, n, 0.f, 1,
                                d_llr_out, d_fit_out, nullptr, stream);
}

int ft8_coherent_drift_llr(ft8_ctx* c, const void* d_samples, int dtype, int64_t n_samples, int32_t n_slots,
                           int64_t slot_stride, const ft8_params* p, const int32_t* d_cand,
                           const int32_t* d_slot_of, int32_t n, float max_rate_hz_per_s, int32_t n_rates,
                           double* d_llr_out, ft8_coh_fit* d_fit_out, ft8_coh_drift* d_drift_out, void* stream) {
  return ft8_coherent_nsym_llr(c, d_samples, dtype, n_samples, n_slots, slot_stride, p, d_cand, d_slot_of, n,
                               max_rate_hz_per_s, n_rates, d_llr_out, d_fit_out, d_drift_out, 1, nullptr, stream);
}

int ft8_coherent_nsym_llr(ft8_ctx* c, const void* d_samples, int dtype, int64_t n_samples, int32_t n_slots,
                          int64_t slot_stride, const ft8_params* p, const int32_t* d_cand,
                          const int32_t* d_slot_of, int32_t n, float max_rate_hz_per_s, int32_t n_rates,
                          double* d_llr_out, ft8_coh_fit* d_fit_out, ft8_coh_drift* d_drift_out, int32_t max_nsym,
                          uint8_t* d_valid_out, void* stream) {
  if (c) c->replay_ok = c->snr_ok = false;
  if (!c || !p || n < 0 || n_slots < 0 || n_samples < 0 || slot_stride < n_samples ||
      (n > 0 && (!d_samples || !d_cand || !d_slot_of || !d_llr_out || !d_fit_out)))
    return fail(c, FT8_E_ARG, "bad argument");
  if (p->steps_per_symbol <= 0 || p->bins_per_tone <= 0) return fail(c, FT8_E_ARG, "bad oversampling factors");
  int rc = check_coherent_drift(c, max_rate_hz_per_s, n_rates);
  if (!rc) rc = check_coherent_nsym(c, max_nsym);
  if (rc) return rc;
  DeviceGuard dg(c->device);
  CohLaunch L;
  rc = coherent_setup(c, d_samples, dtype, n_samples, n_slots, slot_stride, p, max_nsym > 1, &L);
  if (rc) return rc;
  if (n == 0) return FT8_OK;
  L.cand = d_cand;
  L.slot_of = d_slot_of;
  L.n = n;
  L.M = 0;
  L.llr = d_llr_out;
  L.fit = d_fit_out;
  hipStream_t s = (hipStream_t)stream;
  const CohDrift G{max_rate_hz_per_s, n_rates, d_drift_out};
  if (!coherent_drift_on(G) && d_drift_out) {  // off: the plain kernel, and zeros in the drift records
    const hipError_t e = hipMemsetAsync(d_drift_out, 0, sizeof(ft8_coh_drift) * (size_t)n, s);
    if (e != hipSuccess) return hipfail(c, e, "memset");
  }
  // [n][max_nsym][174]; one set: the plain or the drift kernel, and the validity bytes from its fits
  const CohMulti Ms{max_nsym, (int64_t)max_nsym * FT8_LDPC_N, FT8_LDPC_N, d_valid_out};
  hipError_t e = launch_coherent(L, G, Ms, s);
  if (e == hipSuccess && max_nsym == 1 && d_valid_out) e = launch_coh_valid1(d_fit_out, d_valid_out, n, s);
  return e == hipSuccess ? FT8_OK : hipfail(c, e, "coherent launch");
}

int ft8_decode_batch(ft8_ctx* c, const void* d_samples, int dtype, int64_t n_samples, int32_t n_slots,
                     int64_t slot_stride, const ft8_params* p, ft8_result* d_out, int32_t* d_counts,
                     int32_t cap, void* stream) {
  StreamOrder order_(c, (hipStream_t)stream);
  if (c) c->replay_ok = c->snr_ok = false;
  if (c) c->subc_slots = c->subc_passes = -1;
  if (!c || !p || !d_counts || (n_slots > 0 && !d_samples) || n_slots < 0 || cap < 0)
    return fail(c, FT8_E_ARG, "bad argument");
  if (cap > 0 && !d_out) return fail(c, FT8_E_ARG, "null output with positive capacity");
  DeviceGuard dg(c->device);
  hipStream_t s = (hipStream_t)stream;
  if (n_slots == 0) return FT8_OK;
  StageTimer whole(c, kDecodeBatch, s);
  Geo g;
  std::string why;
  int rc = geometry(p, n_samples, &g, &why);
  if (rc) return fail(c, rc, why);
  // also where there is nothing to search
  if ((rc = check_retry_flags(c, d_samples, dtype, n_samples, n_slots, slot_stride, p))) return rc;
  const int T = p->t_hi - p->t_lo, F = p->f_hi - p->f_lo;
  const bool f64 = is_f64_dtype(dtype);
  const int N = p->max_candidates;
  Grid gr = grid_of(T > 0 ? T : 0, F > 0 ? F : 0, p);
  if (T <= 0 || F <= 0 || N <= 0 || gr.NT == 0 || gr.NF == 0) {
    // nothing to search: validate the ranges, report zero decodes
    if (p->t_lo < 0 || p->t_hi > g.frames || p->f_lo < 0 || p->f_hi > g.nfft)
      return fail(c, FT8_E_ARG, "frame/bin range outside the spectrogram");
    hipError_t e = hipMemsetAsync(d_counts, 0, sizeof(int32_t) * n_slots, s);
    whole.done();
    return e == hipSuccess ? FT8_OK : hipfail(c, e, "memset");
  }
  if ((rc = check_search_params(c, p, true))) return rc;
  if ((rc = ensure(c, c->wf, (f64 ? 8 : 4) * (size_t)n_slots * T * F))) return rc;
  if ((rc = ensure(c, c->cand, sizeof(int32_t) * 2 * (size_t)n_slots * N))) return rc;
  if ((rc = ensure(c, c->cand_score, sizeof(double) * (size_t)n_slots * N))) return rc;
  if ((rc = ensure(c, c->cand_count, sizeof(int32_t) * (size_t)n_slots))) return rc;
  if ((rc = ensure(c, c->res_all, sizeof(ft8_result) * (size_t)n_slots * N))) return rc;
  if ((rc = ensure(c, c->llr, sizeof(double) * FT8_LDPC_N * (size_t)n_slots * N))) return rc;
  if ((rc = ensure_sel_scratch(c, n_slots, gr, N, f64))) return rc;
  if ((rc = ensure_retry_scratch(c, p->flags, (size_t)n_slots, N))) return rc;
  if (!(p->flags & FT8_FLAG_SUBTRACT)) {
    if ((rc = decode_pass(c, d_samples, dtype, n_samples, n_slots, slot_stride, p, d_out, d_counts, cap, s))) return rc;
    remember_snr_batch(c, p, g, n_slots, T, F, cap, f64);
    whole.done();
    return FT8_OK;
  }
  // ---- FT8_FLAG_SUBTRACT: pass 1 (complete record lists), then per further pass: subtract what the last
  // pass added, decode the residual, append the new payloads (ft8_set_subtract: 2 to 4 passes, each with
  // the retries the flags ask for when the setting allows them)
  if (dtype != FT8_F32 && dtype != FT8_I16)
    return fail(c, FT8_E_UNSUPPORTED, "FT8_FLAG_SUBTRACT needs float32 or int16 samples");
  const int n_passes = c->sub_passes;
  const int acc_cap = (n_passes - 1) * N;  // the accumulated list before the last merge
  if ((rc = ensure(c, c->out1, sizeof(ft8_result) * (size_t)n_slots * acc_cap))) return rc;
  if ((rc = ensure(c, c->out2, sizeof(ft8_result) * (size_t)n_slots * N))) return rc;
  if ((rc = ensure(c, c->counts1, sizeof(int32_t) * (size_t)n_slots))) return rc;
  if ((rc = ensure(c, c->counts2, sizeof(int32_t) * (size_t)n_slots))) return rc;
  if ((rc = ensure(c, c->sub_pass_counts, sizeof(int32_t) * (size_t)n_slots * n_passes))) return rc;
  if ((rc = ensure(c, c->residual, sizeof(float) * (size_t)n_slots * n_samples))) return rc;
  ft8_result* acc = c->out1.as<ft8_result>();
  ft8_result* out2 = c->out2.as<ft8_result>();
  int32_t* acc_counts = c->counts1.as<int32_t>();
  int32_t* counts2 = c->counts2.as<int32_t>();
  int32_t* pass_counts = c->sub_pass_counts.as<int32_t>();
  float* resid = c->residual.as<float>();
  if ((rc = decode_pass(c, d_samples, dtype, n_samples, n_slots, slot_stride, p, acc, acc_counts, acc_cap, s)))
    return rc;
  if ((rc = subtract_core(c, d_samples, dtype, resid, n_samples, n_slots, slot_stride, n_samples, p, acc, acc_counts,
                          acc_cap, s)))
    return rc;
  for (int k = 2; k <= n_passes; ++k) {
    if ((rc = decode_pass(c, resid, FT8_F32, n_samples, n_slots, n_samples, p, out2, counts2, N, s))) return rc;
    const bool last = k == n_passes;
    hipError_t e = launch_merge_pass(last ? d_out : acc, last ? d_counts : acc_counts, last ? cap : acc_cap, acc,
                                     acc_counts, acc_cap, out2, counts2, N, n_slots, pass_counts, n_passes, k, s);
    if (e != hipSuccess) return hipfail(c, e, "merge launch");
    // the rows this merge appended (from pass_counts' column k - 2 on), fitted on and taken out of the residual
    if (!last && (rc = subtract_core(c, resid, FT8_F32, resid, n_samples, n_slots, n_samples, n_samples, p, acc,
                                     acc_counts, acc_cap, s, pass_counts + (k - 2), n_passes)))
      return rc;
  }
  if (n_passes > 2) c->sub_slots = c->sub_cap = -1;  // the fits' scratch was used again: none to report
  c->subc_slots = n_slots;
  c->subc_passes = n_passes;
  c->replay_ok = false;
  remember_snr_batch(c, p, g, n_slots, T, F, cap, false);
  whole.done();
  return FT8_OK;
}

int ft8_encode(ft8_ctx* c, const uint8_t* d_msg, int32_t msg_bytes, int32_t n, uint8_t* d_a91, uint8_t* d_codeword,
               uint8_t* d_tones, void* stream) {
  if (c) c->replay_ok = c->snr_ok = false;
  if (!c || n < 0 || (n > 0 && !d_msg)) return fail(c, FT8_E_ARG, "bad argument");
  if (msg_bytes != 10 && msg_bytes != 12) return fail(c, FT8_E_ARG, "msg_bytes must be 10 (payload) or 12 (a91)");
  if (n == 0) return FT8_OK;
  DeviceGuard dg(c->device);
  hipError_t e = launch_encode(d_msg, msg_bytes, n, d_a91, d_codeword, d_tones, (hipStream_t)stream);
  return e == hipSuccess ? FT8_OK : hipfail(c, e, "encode launch");
}

int ft8_synthesize(ft8_ctx* c, const uint8_t* d_tones, const ft8_tx_signal* d_signals, int32_t n_signals,
                   int32_t sample_rate, int32_t style, void* d_out, int out_dtype, int64_t n_samples, int32_t n_slots,
                   int64_t slot_stride, void* stream) {
  StreamOrder order_(c, (hipStream_t)stream);
  if (c) c->replay_ok = c->snr_ok = false;
  if (!c || n_signals < 0 || n_slots < 0 || n_samples < 0 || sample_rate <= 0) return fail(c, FT8_E_ARG, "bad argument");
  if (style != FT8_TX_PROTOCOL && style != FT8_TX_REFERENCE) return fail(c, FT8_E_ARG, "unknown ft8_tx_style");
  if (out_dtype != FT8_F32 && out_dtype != FT8_F64 && out_dtype != FT8_C64 && out_dtype != FT8_C128)
    return fail(c, FT8_E_ARG, "out_dtype must be FT8_F32, FT8_F64, FT8_C64 or FT8_C128");
  if (n_signals == 0 || n_slots == 0 || n_samples == 0) return FT8_OK;
  if (!d_tones || !d_signals || !d_out) return fail(c, FT8_E_ARG, "null argument");
  if (slot_stride < n_samples && n_slots > 1) return fail(c, FT8_E_ARG, "slot_stride < n_samples");
  const int nsps = (int)(0.16 * (double)sample_rate);  // modulator.py:31 int(FT8_SYMBOL_TIME_S * fs)
  if (nsps < 8) return fail(c, FT8_E_ARG, "sample_rate too low (nsps < 8)");
  DeviceGuard dg(c->device);
  int rc = gfsk_tables(c, nsps);
  if (rc) return rc;
  SynthLaunch L{};
  L.tones = d_tones;
  L.sig = d_signals;
  L.n_sig = n_signals;
  L.nsps = nsps;
  L.style = style;
  L.fs = (double)sample_rate;
  L.P = c->gfsk_P.as<const double>();
  L.out = d_out;
  L.dtype = out_dtype;
  L.n_samples = n_samples;
  L.slot_stride = slot_stride;
  L.n_slots = n_slots;
  hipError_t e = launch_synth(L, (hipStream_t)stream);
  return e == hipSuccess ? FT8_OK : hipfail(c, e, "synthesize launch");
}

// ---- FT4 stage calls (ft4.hip) -----------------------------------------------------------------------
int ft8_geometry_proto(int32_t protocol, double fs, int32_t bpt, int32_t sps, int64_t n, int32_t* nperseg,
                       int32_t* hop, int32_t* nfft, int32_t* frames) {
  Geo g;
  std::string why;
  int rc = geometry(protocol, fs, bpt, sps, n, &g, &why);
  if (rc) return rc;
  if (nperseg) *nperseg = g.nperseg;
  if (hop) *hop = g.hop;
  if (nfft) *nfft = g.nfft;
  if (frames) *frames = g.frames;
  return FT8_OK;
}

int ft8_ft4_llr(ft8_ctx* c, const void* d_wf, int wf_f64, int32_t T, int32_t F, int32_t sps, int32_t bpt,
                const int32_t* d_cand, int32_t n, int normalize, double* d_llr, void* stream) {
  if (c) c->replay_ok = c->snr_ok = false;
  if (!c || !d_llr || (!d_cand && n > 0) || (!d_wf && n > 0) || sps <= 0 || bpt <= 0 || T < 0 || F < 0)
    return fail(c, FT8_E_ARG, "bad argument");
  if (n <= 0) return FT8_OK;
  DeviceGuard dg(c->device);
  BpLaunch L{};
  L.wf = d_wf;
  L.wf_f64 = wf_f64;
  L.T = T;
  L.F = F;
  L.sps = sps;
  L.bpt = bpt;
  L.cand = d_cand;
  L.n_items = n;
  L.mode = 1;
  L.normalize = normalize;
  L.llr_out = d_llr;
  hipStream_t s = (hipStream_t)stream;
  return timed_launch(c, kLlr, s, "llr launch", [&] { return launch_llr4(L, s); });
}

int ft8_ft4_unscramble(ft8_ctx* c, ft8_result* d_res, int32_t n, void* stream) {
  if (c) c->replay_ok = c->snr_ok = false;
  if (!c || n < 0 || (n > 0 && !d_res)) return fail(c, FT8_E_ARG, "bad argument");
  if (n == 0) return FT8_OK;
  DeviceGuard dg(c->device);
  hipError_t e = launch_ft4_unscramble(d_res, n, nullptr, 0, (hipStream_t)stream);
  return e == hipSuccess ? FT8_OK : hipfail(c, e, "unscramble launch");
}

int ft8_ft4_encode(ft8_ctx* c, const uint8_t* d_msg, int32_t n, uint8_t* d_a91, uint8_t* d_codeword, uint8_t* d_tones,
                   void* stream) {
  if (c) c->replay_ok = c->snr_ok = false;
  if (!c || n < 0 || (n > 0 && !d_msg)) return fail(c, FT8_E_ARG, "bad argument");
  if (n == 0) return FT8_OK;
  DeviceGuard dg(c->device);
  hipError_t e = launch_ft4_encode(d_msg, n, d_a91, d_codeword, d_tones, (hipStream_t)stream);
  return e == hipSuccess ? FT8_OK : hipfail(c, e, "encode launch");
}

int ft8_ft4_synthesize(ft8_ctx* c, const uint8_t* d_tones, const ft8_tx_signal* d_signals, int32_t n_signals,
                       int32_t sample_rate, void* d_out, int out_dtype, int64_t n_samples, int32_t n_slots,
                       int64_t slot_stride, void* stream) {
  StreamOrder order_(c, (hipStream_t)stream);
  if (c) c->replay_ok = c->snr_ok = false;
  if (!c || n_signals < 0 || n_slots < 0 || n_samples < 0 || sample_rate <= 0) return fail(c, FT8_E_ARG, "bad argument");
  if (out_dtype != FT8_F32 && out_dtype != FT8_F64 && out_dtype != FT8_C64 && out_dtype != FT8_C128)
    return fail(c, FT8_E_ARG, "out_dtype must be FT8_F32, FT8_F64, FT8_C64 or FT8_C128");
  const int nsps = ft4_nsps((double)sample_rate);
  if (nsps == 0 || (int64_t)nsps * 105 > INT32_MAX)
    return fail(c, FT8_E_UNSUPPORTED, "FT4 needs a sample rate whose 0.048-s symbol is a whole number of samples (>= 8)");
  if (n_signals == 0 || n_slots == 0 || n_samples == 0) return FT8_OK;
  if (!d_tones || !d_signals || !d_out) return fail(c, FT8_E_ARG, "null argument");
  if (slot_stride < n_samples && n_slots > 1) return fail(c, FT8_E_ARG, "slot_stride < n_samples");
  DeviceGuard dg(c->device);
  int rc = gfsk_tables(c, nsps, 1.0);
  if (rc) return rc;
  SynthLaunch L{};
  L.tones = d_tones;
  L.sig = d_signals;
  L.n_sig = n_signals;
  L.nsps = nsps;
  L.fs = (double)sample_rate;
  L.P = c->gfsk_P.as<const double>();
  L.out = d_out;
  L.dtype = out_dtype;
  L.n_samples = n_samples;
  L.slot_stride = slot_stride;
  L.n_slots = n_slots;
  hipError_t e = launch_ft4_synth(L, (hipStream_t)stream);
  return e == hipSuccess ? FT8_OK : hipfail(c, e, "synthesize launch");
}

int ft8_subtract(ft8_ctx* c, const void* d_samples, int dtype, float* d_residual, int64_t n_samples, int32_t n_slots,
                 int64_t slot_stride, const ft8_params* p, const ft8_result* d_res, const int32_t* d_counts, int32_t cap,
                 void* stream) {
  StreamOrder order_(c, (hipStream_t)stream);
  if (c) c->replay_ok = c->snr_ok = false;
  if (!c || !p || n_slots < 0 || cap < 0 || n_samples < 0) return fail(c, FT8_E_ARG, "bad argument");
  if (n_slots == 0 || n_samples == 0) {
    // nothing to fit: an empty subtraction's (zero) fits are valid, a zero-length one's never written
    c->sub_slots = n_slots == 0 ? 0 : -1;
    c->sub_cap = n_slots == 0 ? cap : -1;
    return FT8_OK;
  }
  if (!d_samples || !d_residual || !d_counts || (cap > 0 && !d_res)) return fail(c, FT8_E_ARG, "null argument");
  if (slot_stride < n_samples && n_slots > 1) return fail(c, FT8_E_ARG, "slot_stride < n_samples");
  DeviceGuard dg(c->device);
  return subtract_core(c, d_samples, dtype, d_residual, n_samples, n_slots, slot_stride, slot_stride, p, d_res,
                       d_counts, cap, (hipStream_t)stream);
}

int ft8_set_subtract(ft8_ctx* c, int32_t n_passes, int32_t retry) {
  if (!c) return FT8_E_ARG;
  if (n_passes < 2 || n_passes > FT8_SUBTRACT_MAX_PASSES)
    return fail(c, FT8_E_ARG, "subtract: n_passes must be in [2, " + std::to_string(FT8_SUBTRACT_MAX_PASSES) + "]");
  if (retry != 0 && retry != 1) return fail(c, FT8_E_ARG, "subtract: retry must be 0 or 1");
  c->sub_passes = n_passes;
  c->sub_retry = retry;
  return FT8_OK;
}

int ft8_subtract_counts(ft8_ctx* c, int32_t* d_out, int32_t n_slots, int32_t n_passes, void* stream) {
  StreamOrder order_(c, (hipStream_t)stream);
  if (!c || !d_out) return fail(c, FT8_E_ARG, "bad argument");
  if (c->subc_slots < 0)
    return fail(c, FT8_E_ARG, "the last ft8_decode_batch was no FT8_FLAG_SUBTRACT batch (or had nothing to search)");
  if (n_slots != c->subc_slots || n_passes != c->subc_passes)
    return fail(c, FT8_E_ARG, "n_slots / n_passes differ from the last FT8_FLAG_SUBTRACT batch's (" +
                                  std::to_string(c->subc_slots) + " / " + std::to_string(c->subc_passes) + ")");
  DeviceGuard dg(c->device);
  hipError_t e = hipMemcpyAsync(d_out, c->sub_pass_counts.p, sizeof(int32_t) * (size_t)n_slots * n_passes,
                                hipMemcpyDeviceToDevice, (hipStream_t)stream);
  return e == hipSuccess ? FT8_OK : hipfail(c, e, "counts copy");
}

int ft8_subtract_fits(ft8_ctx* c, ft8_sub_fit* d_out, int32_t n_slots, int32_t cap, void* stream) {
  StreamOrder order_(c, (hipStream_t)stream);
  if (!c || (!d_out && n_slots > 0 && cap > 0)) return fail(c, FT8_E_ARG, "bad argument");
  if (n_slots != c->sub_slots || cap != c->sub_cap)
    return fail(c, FT8_E_ARG, "n_slots / cap differ from the last subtraction's (" + std::to_string(c->sub_slots) +
                                  " / " + std::to_string(c->sub_cap) + ")");
  if (n_slots == 0 || cap == 0) return FT8_OK;
  DeviceGuard dg(c->device);
  static_assert(sizeof(ft8_sub_fit) == 1056, "ft8_sub_fit layout");
  hipError_t e = hipMemcpyAsync(d_out, c->sub_est.p, sizeof(ft8_sub_fit) * (size_t)n_slots * cap,
                                hipMemcpyDeviceToDevice, (hipStream_t)stream);
  return e == hipSuccess ? FT8_OK : hipfail(c, e, "fits copy");
}

int ft8_stft_argmax(ft8_ctx* c, const void* d_samples, int dtype, int64_t n_samples, int32_t n_slots,
                    int64_t slot_stride, const ft8_params* p, int32_t* d_idx, void* stream) {
  StreamOrder order_(c, (hipStream_t)stream);
  if (c) c->replay_ok = c->snr_ok = false;
  if (!c || !p || (n_slots > 0 && (!d_samples || !d_idx))) return fail(c, FT8_E_ARG, "null argument");
  if (n_slots < 0 || n_samples < 0) return fail(c, FT8_E_ARG, "negative size");
  if (n_slots > 1 && slot_stride < n_samples) return fail(c, FT8_E_ARG, "slot_stride < n_samples");
  if (int rc = ft8_only(c, p, "ft8_stft_argmax")) return rc;
  DeviceGuard dg(c->device);
  return stft_argmax_core(c, d_samples, dtype, n_samples, n_slots, slot_stride, p, d_idx, (hipStream_t)stream);
}

int ft8_drift_fit(ft8_ctx* c, int32_t stage, const int32_t* d_idx, int32_t n_slots, int32_t T, int32_t F,
                  const ft8_drift_params* p, ft8_drift_result* d_res, double* d_metric, int32_t* d_segments,
                  int32_t max_segments, void* stream) {
  StreamOrder order_(c, (hipStream_t)stream);
  if (c) c->replay_ok = c->snr_ok = false;
  if (!c || !p) return fail(c, FT8_E_ARG, "null argument");
  if (stage != 1 && stage != 2) return fail(c, FT8_E_ARG, "stage must be 1 or 2");
  if (n_slots < 0 || T < 0 || max_segments < 0) return fail(c, FT8_E_ARG, "negative size");
  if (n_slots == 0) return FT8_OK;
  if (!d_res || (T > 0 && !d_idx)) return fail(c, FT8_E_ARG, "null argument");
  DeviceGuard dg(c->device);
  return drift_fit_core(c, stage, d_idx, n_slots, T, F, p, d_res, d_metric, d_segments, max_segments,
                        (hipStream_t)stream);
}

int ft8_drift_correct(ft8_ctx* c, const void* d_samples, int dtype, int64_t n_samples, int32_t n_slots,
                      int64_t slot_stride, const ft8_drift_params* p, void* d_out, ft8_drift_result* d_res,
                      void* stream) {
  StreamOrder order_(c, (hipStream_t)stream);
  if (c) c->replay_ok = c->snr_ok = false;
  if (!c || !p) return fail(c, FT8_E_ARG, "null argument");
  if (n_slots < 0 || n_samples < 0) return fail(c, FT8_E_ARG, "negative size");
  if (n_slots == 0) return FT8_OK;
  if (!d_samples || !d_out || !d_res) return fail(c, FT8_E_ARG, "null argument");
  if (n_slots > 1 && slot_stride < n_samples) return fail(c, FT8_E_ARG, "slot_stride < n_samples");
  if (dtype != FT8_F32 && dtype != FT8_F64 && dtype != FT8_C64 && dtype != FT8_C128)
    return fail(c, FT8_E_UNSUPPORTED, "drift correction takes float32/float64/complex64/complex128 samples");
  int rc = check_drift_params(c, p);
  if (rc) return rc;
  DeviceGuard dg(c->device);
  hipStream_t s = (hipStream_t)stream;
  Geo g;
  std::string why;
  const int fs = (int)p->sample_rate;
  if ((rc = geometry(fs, p->bins_per_tone, p->steps_per_symbol, n_samples, &g, &why))) return fail(c, rc, why);
  if (g.frames == 0) return fail(c, FT8_E_ARG, "input shorter than one symbol (the reference's argmax of an empty spectrogram raises)");
  if (g.frames > kDriftMaxT) return fail(c, FT8_E_RANGE, "more than " + std::to_string(kDriftMaxT) + " frames per signal");
  const int T = g.frames, F = drift_bins(g.nfft);
  if ((rc = ensure(c, c->drift_idx, sizeof(int32_t) * (size_t)n_slots * T))) return rc;
  int32_t* idx = c->drift_idx.as<int32_t>();
  ft8_params sp{};
  sp.sample_rate = fs;
  sp.bins_per_tone = p->bins_per_tone;
  sp.steps_per_symbol = p->steps_per_symbol;
  sp.f_lo = 0;
  sp.f_hi = F;
  sp.t_lo = 0;
  sp.t_hi = T;
  if ((rc = stft_argmax_core(c, d_samples, dtype, n_samples, n_slots, slot_stride, &sp, idx, s))) return rc;
  if ((rc = drift_fit_core(c, 1, idx, n_slots, T, F, p, d_res, nullptr, nullptr, 0, s))) return rc;
  DerotateLaunch D{};
  D.x = d_samples;
  D.dtype = dtype;
  D.slot_stride = slot_stride;
  D.out = (double*)d_out;
  D.n_samples = n_samples;
  D.n_slots = n_slots;
  D.res = d_res;
  D.fs = p->sample_rate;
  D.inv_fs = 1.0 / p->sample_rate;
  D.inv_2fs2 = 1.0 / (2.0 * p->sample_rate * p->sample_rate);
  if ((rc = timed_launch(c, kDriftDerotate, s, "derotate launch", [&] { return launch_derotate1(D, s); }))) return rc;
  if (!p->precise_sync) return FT8_OK;
  if ((rc = stft_argmax_core(c, d_out, FT8_C128, n_samples, n_slots, n_samples, &sp, idx, s))) return rc;
  if ((rc = drift_fit_core(c, 2, idx, n_slots, T, F, p, d_res, nullptr, nullptr, 0, s))) return rc;
  return timed_launch(c, kDriftDerotate, s, "derotate launch", [&] { return launch_derotate2(D, p->poly_degree, s); });
}

const char* ft8_build_id(void) { return FT8_BUILD_ID; }
const char* ft8_build_flags(void) { return FT8_BUILD_FLAGS; }

int ft8_replay_stage(ft8_ctx* c, int32_t stage, int32_t reps, void* stream) {
  StreamOrder order_(c, (hipStream_t)stream);
  if (!c || reps < 0) return fail(c, FT8_E_ARG, "bad argument");
  if (!c->replay_ok) return fail(c, FT8_E_ARG, "no single-chain ft8_decode_batch to replay");
  c->snr_ok = false;  // a replayed STFT rewrites wf from whatever the caller's sample buffer holds now
  DeviceGuard dg(c->device);
  hipStream_t s = (hipStream_t)stream;
  for (int r = 0; r < reps; ++r) {
    hipError_t e;
    switch (stage) {
      case kStft: e = launch_stft(c->last_stft, s); break;
      case kScore: e = launch_score(c->last_sync, s); break;
      case kSelect: e = launch_select(c->last_sync, s); break;
      case kBp: e = run_bp(c->last_bp, s); break;  // the kernel that ran (BpLaunch.f32)
      case kCompact: e = launch_compact(c->last_compact, s); break;
      case kLlr: e = launch_llr(c->last_bp, s); break;
      default: return fail(c, FT8_E_ARG, "stage " + std::to_string(stage) + " cannot be replayed");
    }
    if (e != hipSuccess) return hipfail(c, e, "replay launch");
  }
  return FT8_OK;
}

int ft8_set_pipeline(ft8_ctx* c, int32_t chunk_slots, int32_t n_streams, int32_t bp_waves_per_simd) {
  if (!c || chunk_slots < 0 || n_streams < 0 || n_streams > 8 || bp_waves_per_simd < 1 || bp_waves_per_simd > 4)
    return fail(c, FT8_E_ARG, "bad pipeline setting");
  c->chunk_slots = chunk_slots;
  c->n_streams = n_streams;
  c->bp_waves = bp_waves_per_simd;
  return FT8_OK;
}

int64_t ft8_pack_bytes(int32_t n_slots, int32_t capacity) {
  if (n_slots < 0 || capacity < 0) return -1;
  return pack_header_bytes(n_slots) + (int64_t)capacity * (int64_t)sizeof(ft8_result);
}

int ft8_pack_decodes(ft8_ctx* c, const ft8_result* d_records, const int32_t* d_counts, int32_t n_slots, int32_t cap,
                     int32_t capacity, int32_t slot_offset, void* d_send, ft8_result* d_overflow, void* stream) {
  if (!c || !d_send || n_slots < 0 || cap < 0 || capacity < 0) return fail(c, FT8_E_ARG, "bad argument");
  if (n_slots > 0 && (!d_counts || (cap > 0 && !d_records))) return fail(c, FT8_E_ARG, "null records or counts");
  if ((int64_t)n_slots * cap > INT32_MAX) return fail(c, FT8_E_RANGE, "n_slots * cap exceeds 2^31 rows");
  if (((uintptr_t)d_send & 7) || ((uintptr_t)d_overflow & 7)) return fail(c, FT8_E_ARG, "buffers must be 8-byte aligned");
  DeviceGuard dg(c->device);
  hipError_t e = launch_pack(d_records, d_counts, n_slots, cap, capacity, slot_offset, (uint8_t*)d_send, d_overflow,
                             (hipStream_t)stream);
  return e == hipSuccess ? FT8_OK : hipfail(c, e, "pack launch");
}

// like ft8_pack_decodes it touches no context state, so it takes no part in the StreamOrder
int ft8_unpack77(ft8_ctx* c, const ft8_result* d_records, const int32_t* d_counts, int32_t n_slots, int32_t cap,
                 ft8_text* d_out, void* stream) {
  if (!c || n_slots < 0 || cap < 0) return fail(c, FT8_E_ARG, "bad argument");
  if (cap > INT16_MAX) return fail(c, FT8_E_RANGE, "cap exceeds 32767 (ft8_text.dup_of is 16 bits)");
  if (n_slots > 0 && cap > 0 && (!d_records || !d_out)) return fail(c, FT8_E_ARG, "null records or output");
  if (((uintptr_t)d_records & 7) || ((uintptr_t)d_out & 3) || ((uintptr_t)d_counts & 3))
    return fail(c, FT8_E_ARG, "records must be 8-byte, text records and counts 4-byte aligned");
  DeviceGuard dg(c->device);
  hipError_t e = launch_unpack77(d_records, d_counts, n_slots, cap, d_out, (hipStream_t)stream);
  return e == hipSuccess ? FT8_OK : hipfail(c, e, "unpack77 launch");
}

// the two stage calls touch no context state, so like ft8_unpack77 they take no part in the StreamOrder
int ft8_noise_floor(ft8_ctx* c, const void* d_wf, int wf_f64, int32_t n_slots, int32_t T, int32_t F, double q,
                    double* d_floor, double* d_colmean, void* stream) {
  if (!c || n_slots < 0) return fail(c, FT8_E_ARG, "bad argument");
  if (!(q >= 0.0 && q <= 1.0)) return fail(c, FT8_E_ARG, "q must lie in [0, 1]");
  if (n_slots == 0) return FT8_OK;
  if (T <= 0 || F <= 0) return fail(c, FT8_E_ARG, "empty waterfall");
  if (!d_wf || !d_floor || !d_colmean) return fail(c, FT8_E_ARG, "null argument");
  if (((uintptr_t)d_wf & (wf_f64 ? 7 : 3)) || ((uintptr_t)d_floor & 7) || ((uintptr_t)d_colmean & 7))
    return fail(c, FT8_E_ARG, "misaligned buffer");
  DeviceGuard dg(c->device);
  hipError_t e = launch_noise_floor(d_wf, wf_f64, n_slots, T, F, noise_floor_rank(q, F), d_floor, d_colmean,
                                    (hipStream_t)stream);
  return e == hipSuccess ? FT8_OK : hipfail(c, e, "noise floor launch");
}

int ft8_snr(ft8_ctx* c, const void* d_wf, int wf_f64, int32_t n_slots, int32_t T, int32_t F, const ft8_params* p,
            int64_t n_samples, const ft8_result* d_records, const int32_t* d_counts, int32_t cap,
            const double* d_floor, int32_t radius, ft8_snr_rec* d_out, void* stream) {
  if (!c || !p || n_slots < 0 || cap < 0) return fail(c, FT8_E_ARG, "bad argument");
  if (radius < 0 || radius > 1) return fail(c, FT8_E_ARG, "radius must be 0 or 1");
  Geo g;
  std::string why;
  int rc = ft8_only(c, p, "ft8_snr");
  if (rc) return rc;
  rc = geometry(rate_of(p), p->bins_per_tone, p->steps_per_symbol, n_samples, &g, &why);
  if (rc) return fail(c, rc, why);
  if (n_slots == 0 || cap == 0) return FT8_OK;
  if (T <= 0 || F <= 0) return fail(c, FT8_E_ARG, "empty waterfall");
  if (!d_wf || !d_floor) return fail(c, FT8_E_ARG, "null argument");
  if (((uintptr_t)d_wf & (wf_f64 ? 7 : 3)) || ((uintptr_t)d_floor & 7)) return fail(c, FT8_E_ARG, "misaligned buffer");
  if ((rc = check_snr_records(c, d_records, d_counts, n_slots, cap, d_out))) return rc;
  DeviceGuard dg(c->device);
  hipError_t e = launch_snr(d_wf, wf_f64, n_slots, T, F, p->steps_per_symbol, p->bins_per_tone, d_records, d_counts,
                            cap, d_floor, radius, snr_bw_db(rate_of(p), g.nperseg), d_out, (hipStream_t)stream);
  return e == hipSuccess ? FT8_OK : hipfail(c, e, "snr launch");
}

int ft8_snr_last(ft8_ctx* c, const ft8_result* d_records, const int32_t* d_counts, int32_t n_slots, int32_t cap,
                 ft8_snr_rec* d_out, void* stream) {
  StreamOrder order_(c, (hipStream_t)stream);
  if (!c || n_slots < 0 || cap < 0) return fail(c, FT8_E_ARG, "bad argument");
  if (n_slots == 0) return FT8_OK;
  if (!c->snr_ok) return fail(c, FT8_E_ARG, "no ft8_decode_batch whose waterfall is still in the context");
  const auto& b = c->snr_batch;
  if (n_slots != b.n_slots || cap != b.cap)
    return fail(c, FT8_E_ARG, "n_slots / cap differ from the last ft8_decode_batch's (" + std::to_string(b.n_slots) +
                                  " / " + std::to_string(b.cap) + ")");
  if (b.ft4) return fail(c, FT8_E_UNSUPPORTED, "the last batch was FT4: ft8_snr_last does not take FT4");
  if (b.subtract)
    return fail(c, FT8_E_UNSUPPORTED,
                "the last batch ran FT8_FLAG_SUBTRACT: the context holds the residual's waterfall, without the pass-1 "
                "signals (use ft8_stft + ft8_noise_floor + ft8_snr)");
  if (cap == 0) return FT8_OK;
  int rc;
  if ((rc = check_snr_records(c, d_records, d_counts, n_slots, cap, d_out))) return rc;
  DeviceGuard dg(c->device);
  hipStream_t s = (hipStream_t)stream;
  if ((rc = ensure(c, c->snr_A, sizeof(double) * (size_t)n_slots * b.F))) return rc;
  if ((rc = ensure(c, c->snr_N0, sizeof(double) * (size_t)n_slots))) return rc;
  hipError_t e = launch_noise_floor(c->wf.p, b.f64, n_slots, b.T, b.F, noise_floor_rank(0.25, b.F),
                                    c->snr_N0.as<double>(), c->snr_A.as<double>(), s);
  if (e != hipSuccess) return hipfail(c, e, "noise floor launch");
  e = launch_snr(c->wf.p, b.f64, n_slots, b.T, b.F, b.sps, b.bpt, d_records, d_counts, cap, c->snr_N0.as<double>(), 1,
                 b.bw_db, d_out, s);
  return e == hipSuccess ? FT8_OK : hipfail(c, e, "snr launch");
}

int ft8_select_warnings(ft8_ctx* c, int32_t* d_out, int32_t n_slots, void* stream) {
  StreamOrder order_(c, (hipStream_t)stream);
  if (!c || !d_out || n_slots < 0) return fail(c, FT8_E_ARG, "bad argument");
  if (n_slots == 0) return FT8_OK;
  if (!c->warn.p || c->warn.cap < sizeof(int32_t) * n_slots) return fail(c, FT8_E_ARG, "no selection has run");
  DeviceGuard dg(c->device);
  hipError_t e = hipMemcpyAsync(d_out, c->warn.p, sizeof(int32_t) * n_slots, hipMemcpyDeviceToDevice,
                                (hipStream_t)stream);
  return e == hipSuccess ? FT8_OK : hipfail(c, e, "copy warnings");
}

int ft8_crc14(ft8_ctx* c, const uint8_t* d_msg, const int32_t* d_nbits, int32_t n, uint16_t* d_crc, void* stream) {
  if (c) c->replay_ok = c->snr_ok = false;
  if (!c || (n > 0 && (!d_msg || !d_nbits || !d_crc))) return fail(c, FT8_E_ARG, "bad argument");
  DeviceGuard dg(c->device);
  hipError_t e = launch_crc14(d_msg, d_nbits, n, d_crc, (hipStream_t)stream);
  return e == hipSuccess ? FT8_OK : hipfail(c, e, "crc14 launch");
}

int ft8_ldpc_check(ft8_ctx* c, const uint8_t* d_bits, int32_t n, int32_t* d_errors, void* stream) {
  if (c) c->replay_ok = c->snr_ok = false;
  if (!c || (n > 0 && (!d_bits || !d_errors))) return fail(c, FT8_E_ARG, "bad argument");
  DeviceGuard dg(c->device);
  hipError_t e = launch_ldpc_check(d_bits, n, d_errors, (hipStream_t)stream);
  return e == hipSuccess ? FT8_OK : hipfail(c, e, "ldpc_check launch");
}

int ft8_set_timing(ft8_ctx* c, int enable) {
  if (!c) return FT8_E_ARG;
  c->timing = enable != 0;
  if (c->timing && !c->stats.p) {
    DeviceGuard dg(c->device);
    const size_t bytes = (size_t)kStatRows * kStatStride * sizeof(unsigned long long);
    int rc = ensure(c, c->stats, bytes);
    if (rc) return rc;
    hipError_t e = hipMemset(c->stats.p, 0, bytes);
    if (e != hipSuccess) return hipfail(c, e, "stats reset");
  }
  return FT8_OK;
}

int ft8_set_timing_stages(ft8_ctx* c, uint32_t mask) {
  if (!c) return FT8_E_ARG;
  c->stage_mask = mask;
  return FT8_OK;
}

// the k_bp counter rows (kStatRows x kStatStride) summed per column (column 6, the longest wave,
// by maximum); reset zeroes columns [c0, c0 + 4) of every row
static int read_stat_rows(ft8_ctx* c, int c0, int reset, unsigned long long* out4) {
  std::vector<unsigned long long> v((size_t)kStatRows * kStatStride);
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(v.data(), c->stats.p, v.size() * sizeof(v[0]), hipMemcpyDeviceToHost);
  if (e == hipSuccess && reset)
    e = hipMemset2D((char*)c->stats.p + c0 * sizeof(v[0]), kStatStride * sizeof(v[0]), 0, 4 * sizeof(v[0]), kStatRows);
  if (e != hipSuccess) return hipfail(c, e, "counters");
  for (int i = 0; i < 4; ++i) out4[i] = 0;
  for (int r = 0; r < kStatRows; ++r)
    for (int i = 0; i < 4; ++i) {
      const unsigned long long x = v[(size_t)r * kStatStride + c0 + i];
      out4[i] = (c0 + i == 6) ? std::max(out4[i], x) : out4[i] + x;
    }
  return FT8_OK;
}

int ft8_get_counters(ft8_ctx* c, int64_t* out4, int reset) {
  if (!c || !out4) return FT8_E_ARG;
  for (int i = 0; i < 4; ++i) out4[i] = 0;
  if (!c->stats.p) return FT8_OK;
  DeviceGuard dg(c->device);
  unsigned long long v[4];
  int rc = read_stat_rows(c, 0, reset, v);
  if (rc) return rc;
  for (int i = 0; i < 4; ++i) out4[i] = (int64_t)v[i];
  return FT8_OK;
}

int ft8_get_bp_clock(ft8_ctx* c, int64_t* out5, int reset) {
  if (!c || !out5) return FT8_E_ARG;
  for (int i = 0; i < 5; ++i) out5[i] = 0;
  DeviceGuard dg(c->device);
  int khz = 0;
  hipError_t e = hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->device);
  if (e != hipSuccess) return hipfail(c, e, "wall clock rate");
  out5[4] = khz;
  if (!c->stats.p) return FT8_OK;
  unsigned long long v[4];
  int rc = read_stat_rows(c, 4, reset, v);
  if (rc) return rc;
  for (int i = 0; i < 4; ++i) out5[i] = (int64_t)v[i];
  return FT8_OK;
}

int ft8_get_timing(ft8_ctx* c, double* ms, int64_t* launches, int reset) {
  if (!c) return FT8_E_ARG;
  DeviceGuard dg(c->device);
  for (auto& t : c->pending) {
    hipError_t e = hipEventSynchronize(t.b);
    if (e != hipSuccess) return hipfail(c, e, "event sync");
    float v = 0.f;
    (void)hipEventElapsedTime(&v, t.a, t.b);
    c->ms[t.stage] += v;
    c->launches[t.stage] += 1;
    c->pool.push_back(t.a);
    c->pool.push_back(t.b);
  }
  c->pending.clear();
  for (int i = 0; i < FT8_N_STAGES; ++i) {
    if (ms) ms[i] = c->ms[i];
    if (launches) launches[i] = c->launches[i];
    if (reset) {
      c->ms[i] = 0;
      c->launches[i] = 0;
    }
  }
  return FT8_OK;
}

}  // extern "C"
