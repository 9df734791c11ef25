// bp32.hip -- LDPC(174,91) belief propagation in IEEE binary32, two candidates per wave (gfx950).
//
// The opt-in float32 decoder (ft8hip.h, "float32 belief propagation"; ft8_bp_f32, FT8_FLAG_BP_F32).  k_bp
// (bp.hip) stays the reference-exact float64 kernel and is not touched; this file restates what it needs
// of k_bp's message layout rather than sharing it, so that bp.hip has no diff.
//
// Shape: k_bp's.  Workgroups are single persistent waves that pull work from the 64-bit claim counter,
// the 522 Tanner-graph edges are dealt to lanes nine per lane (variable-major: three variables' edges;
// check-major: the seven edges of the lane's own check and two edges of the 19 leftover checks), and
// the messages live in one LDS array in k_bp's row-position-major layout.  What differs:
//   * a message slot is a float2: the same edge of TWO candidates (.x: item 2 k, .y: item 2 k + 1 of
//     the launch), so an 8-byte slot, every LDS address and every table of k_bp's layout carry over and
//     the polynomials, sums and products issue as packed float32 (v_pk_mul_f32 / v_pk_add_f32 /
//     v_pk_fma_f32): one instruction for both candidates;
//   * every division is the correctly rounded IEEE sequence hipcc emits for float `x / y`
//     (v_div_scale_f32 x2, v_rcp_f32, the Newton / residual FMAs, v_div_fmas_f32, v_div_fixup_f32),
//     written with builtins so that its six FMA / multiply steps are packed over the two candidates and
//     the three divisions of a group interleave.  No shared reciprocal, no folded scalings: in float32
//     underflow is near (a product of six toc reaches subnormals from |toc| ~ 1e-7), and every step
//     here is the contract's own operation on the contract's own operands;
//   * the two candidates of a wave stop independently (all-zero, converged, last iteration): a stopped
//     candidate's hard decision, error count and counters are frozen while its messages keep being
//     updated, unread, until its partner stops too.  Every message is bounded (fast_tanh clips), so a
//     stopped or absent candidate can raise nothing that reaches its partner: no operation mixes .x and .y.
//
// The contract's arithmetic, per candidate (bp32.py bp32_restate is the NumPy restatement):
//   c = (float)llr; messages = c + ((t0 + t1) + t2); Tnm = (c + t_a) + t_b;
//   toc = fast_tanh(-Tnm / 2) with np.clip(x, -4.97f, 4.97f) passing NaN;  Tmn = ((1 toc_0) toc_1) ..;
//   tov = -2 fast_atanh(Tmn); no FMA contraction (-ffp-contract=off), subnormals kept.
#include "ft8_internal.h"

namespace ft8 {
namespace {

typedef float f2 __attribute__((ext_vector_type(2)));

__constant__ uint16_t kChkStart32[FT8_LDPC_M + 1] = FT8_CHK_START_INIT;
__constant__ uint8_t kEdgeVar32[FT8_LDPC_E] = FT8_EDGE_VAR_INIT;
__constant__ uint16_t kVarEdge32[FT8_LDPC_N * 3] = FT8_VAR_EDGE_INIT;
__constant__ uint8_t kEdgeChk32[FT8_LDPC_E] = FT8_EDGE_CHK_INIT;

constexpr int kEdgeSlots = (FT8_LDPC_E + kWave - 1) / kWave;  // 9
constexpr int kVarSlots = (FT8_LDPC_N + kWave - 1) / kWave;   // 3
constexpr int kChkSlots = (FT8_LDPC_M + kWave - 1) / kWave;   // 2
constexpr int kDivGroup = 3;                                  // divisions interleaved stage by stage
static_assert(kEdgeSlots % kDivGroup == 0 && kVarSlots == 3, "division groups tile the slots exactly");
constexpr int kBp32WavesPerSimd = 4;   // 5.7 KB of LDS per wave: 16 waves per CU fit the 160 KB
constexpr int kBp32GridCus = 256;      // MI355X: 256 CUs
constexpr int kPair = 2;               // candidates per wave, and tickets per claim

// ---- message layout: k_bp's (bp.hip, "k_bp message layout"), with float2 slots -----------------------
// Checks renumbered degree-7 first (m' = 0..23), then the degree-6 rows; the message of edge (m', q), q
// the edge's position in its check's row, lives at index q * 83 + m' (q < 6) or 498 + m' (q = 6);
// indices 522..583 hold the constant 1.0 that stands in for a degree-6 row's missing seventh factor.
// Lane L owns row L check-major (rows 0..63); the 19 leftover rows 64..82 are edge-major on two more
// register slots: lane 19 q3 + r owns edges (64 + r, q3) and (64 + r, 3 + q3).
constexpr int kM7 = 24;
constexpr int kQS = FT8_LDPC_M;
constexpr int kQ6 = 6 * kQS;
constexpr int kMsgN = 584;
constexpr int kOne = kMsgN - 1;
constexpr int kHdr = 1024;
constexpr int kLeftRows = FT8_LDPC_M - kWave;
constexpr int kLeftLanes = 3 * kLeftRows;
constexpr int kRowB = 8 * kQS;         // byte stride of one row position (sizeof(f2) == 8)
static_assert(sizeof(f2) == 8, "a message slot is two floats");
static_assert(kEdgeSlots * kWave <= kMsgN && kQ6 + kM7 == FT8_LDPC_E, "row-major message layout");
static_assert(kWave + kLeftRows == FT8_LDPC_M && kLeftRows == 19 && kM7 <= kWave && kLeftLanes <= kWave, "64 + 19 rows");
static_assert(kQ6 + kWave - 1 < kMsgN, "a check-major lane's seventh factor is a message or a constant");
static_assert(kEdgeSlots == 7 + 2, "seven check-major products and two leftover ones per lane");
__host__ __device__ constexpr int left_q3(int lane) { return lane / kLeftRows < 3 ? lane / kLeftRows : 2; }
__host__ __device__ constexpr int left_r(int lane) { return lane % kLeftRows; }
__host__ __device__ constexpr int left_f0(int q3) { return q3 == 0 ? 1 : 0; }
__host__ __device__ constexpr int left_f1(int q3) { return q3 == 2 ? 1 : 2; }
__host__ __device__ constexpr int msg_idx(int q, int mp) { return q * kQS + mp; }
// the mapping as a model: every index phase D reads lies inside msg, each of a leftover edge's five
// factors is read exactly once and its own never, and the stores cover the 522 edges exactly once
__host__ __device__ constexpr bool phase_d_mapping_ok() {
  int stores[kMsgN] = {};
  for (int lane = 0; lane < kWave; ++lane) {
    for (int f = 0; f < 7; ++f) {
      if (msg_idx(f, lane) >= kMsgN) return false;
      if (f < 6 || lane < kM7) stores[msg_idx(f, lane)]++;
    }
    const int q3 = left_q3(lane), row = kWave + left_r(lane);
    for (int s = 0; s < 2; ++s) {
      const int fs[5] = {3 * s + left_f0(q3), 3 * s + left_f1(q3), 3 * (1 - s), 3 * (1 - s) + 1, 3 * (1 - s) + 2};
      int seen = 0;
      for (int k = 0; k < 5; ++k) {
        if (fs[k] < 0 || fs[k] > 5 || row >= FT8_LDPC_M || msg_idx(fs[k], row) >= kQ6) return false;
        seen |= 1 << fs[k];
      }
      if (seen != (0x3f & ~(1 << (3 * s + q3)))) return false;
      if (lane < kLeftLanes) stores[msg_idx(3 * s + q3, row)]++;
    }
  }
  for (int x = 0; x < kMsgN; ++x)
    if (stores[x] != (x < FT8_LDPC_E ? 1 : 0)) return false;
  return true;
}
static_assert(phase_d_mapping_ok(), "phase D reads inside msg and produces every edge exactly once");

struct Wave32Lds {
  uint8_t bits[256];               // hard decision of every variable (one candidate at a time)
  uint8_t a91[16];
  uint8_t rank[FT8_LDPC_M];        // prologue scratch: check m -> m'
  uint8_t chk_of[FT8_LDPC_M];      // prologue scratch: m' -> m
  uint8_t pad_[kHdr - 256 - 16 - 2 * FT8_LDPC_M];
  f2 msg[kMsgN];                   // tov between sweeps; toc within a sweep
};
static_assert(offsetof(Wave32Lds, msg) == kHdr, "msg follows the header");

// per-lane tables (registers, built once per wave): the LDS byte addresses of the three edge messages of
// variable n = lane + 64 j in kFTX_LDPC_Mn order, and the variables of check m' = lane + 64 k as a mask
struct Wave32Tables {
  uint32_t va[kVarSlots], va1[kVarSlots], vb[kVarSlots];
  uint32_t h[kChkSlots][kVarSlots][2];
};

typedef __attribute__((address_space(3))) f2 lds_f2;

__device__ __forceinline__ uint32_t lds_addr(const void* p) {
  return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const void*)p;
}
// one ds_read_b64 with the offset as its immediate (volatile: no pairing into ds_read2_b64, whose
// 8-bit offsets cannot span a row)
__device__ __forceinline__ f2 ldv(uint32_t addr) { return *(const volatile lds_f2*)(uintptr_t)addr; }
__device__ __forceinline__ void stv(uint32_t addr, f2 v) { *(lds_f2*)(uintptr_t)addr = v; }

__device__ void load_tables(Wave32Tables& t, Wave32Lds& L, int lane) {
  if (lane == 0) {  // degree-7 rows first, each group in check order
    int c7 = 0, c6 = kM7;
    for (int m = 0; m < FT8_LDPC_M; ++m) {
      const int r = (kChkStart32[m + 1] - kChkStart32[m]) == 7 ? c7++ : c6++;
      L.rank[m] = (uint8_t)r;
      L.chk_of[r] = (uint8_t)m;
    }
  }
  __syncthreads();
  const uint32_t msg0 = lds_addr(&L.msg[0]);
  auto addr_of = [&](int e) -> uint32_t {  // edge (CSR index) -> LDS byte address of its message
    const int m = kEdgeChk32[e], q = e - kChkStart32[m], r = L.rank[m];
    return msg0 + 8u * (uint32_t)(q < 6 ? q * kQS + r : kQ6 + r);
  };
#pragma unroll
  for (int j = 0; j < kVarSlots; ++j) {
    const int n = lane + kWave * j;
    if (n < FT8_LDPC_N) {
      t.va[j] = addr_of(kVarEdge32[3 * n]);
      t.va1[j] = addr_of(kVarEdge32[3 * n + 1]);
      t.vb[j] = addr_of(kVarEdge32[3 * n + 2]);
    } else {  // padding variable: reads the constant, never stores (see the sweep)
      t.va[j] = t.va1[j] = t.vb[j] = msg0 + 8u * kOne;
    }
  }
#pragma unroll
  for (int k = 0; k < kChkSlots; ++k) {
    const int mp = lane + kWave * k;
#pragma unroll
    for (int j = 0; j < kVarSlots; ++j) t.h[k][j][0] = t.h[k][j][1] = 0;
    if (mp < FT8_LDPC_M) {
      const int m = L.chk_of[mp];
      for (int e = kChkStart32[m]; e < kChkStart32[m + 1]; ++e) {
        const int v = kEdgeVar32[e];
#pragma unroll
        for (int j = 0; j < kVarSlots; ++j)
#pragma unroll
          for (int w = 0; w < 2; ++w)
            if (v >> 5 == 2 * j + w) t.h[k][j][w] |= 1u << (v & 31);
      }
    }
  }
  for (int x = FT8_LDPC_E + lane; x < kMsgN; x += kWave) L.msg[x] = f2{1.0f, 1.0f};  // the constants, once
  __syncthreads();
  // keep the tables in registers: opaque values cannot be rematerialised from memory in the loop
#pragma unroll
  for (int j = 0; j < kVarSlots; ++j) asm volatile("" : "+v"(t.va[j]), "+v"(t.va1[j]), "+v"(t.vb[j]));
#pragma unroll
  for (int k = 0; k < kChkSlots; ++k)
#pragma unroll
    for (int j = 0; j < kVarSlots; ++j) asm volatile("" : "+v"(t.h[k][j][0]), "+v"(t.h[k][j][1]));
}

struct Bp32Args {
  const int32_t* cand;
  const double* cand_score;
  const int32_t* cand_count;
  int N, n_items, mode;
  const double* llr_in;
  int max_iterations;
  uint8_t* plain_out;
  ft8_result* res;
  unsigned long long* work;      // claim counter (64-bit, never reset), kPair tickets per claim
  unsigned long long work_base;  // this launch's first ticket
  unsigned long long* stats;     // nullable, k_bp's rows: [candidates, iterations entered, message passes, converged]
  unsigned long long* clock;     // nullable, stats + 4: [wave cycles, wave wall ticks, max wave cycles, waves]
  int slot0;
};

// phase boundary inside a sweep: the workgroup is one wave and the LDS executes a wave's instructions in
// order, so only the compiler must not move LDS accesses across the boundary
__device__ __forceinline__ void sweep_sync() { asm volatile("" ::: "memory"); }

__device__ __forceinline__ f2 fma2(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }

// K correctly rounded float divisions of both candidates: the sequence hipcc emits for `x / y` (IEEE,
// subnormals kept), stage by stage so that the K chains interleave; the scale / reciprocal / fmas / fixup
// steps are per component, the FMAs and the multiply between them packed
template <int K>
__device__ __forceinline__ void div_rn32(f2* q, const f2* x, const f2* y) {
  f2 den[K], num[K], r[K], e[K], m[K];
  bool fl[K][2], f0;
#pragma unroll
  for (int i = 0; i < K; ++i)
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      den[i][u] = __builtin_amdgcn_div_scalef(x[i][u], y[i][u], false, &f0);
      num[i][u] = __builtin_amdgcn_div_scalef(x[i][u], y[i][u], true, &fl[i][u]);
    }
#pragma unroll
  for (int i = 0; i < K; ++i)
#pragma unroll
    for (int u = 0; u < 2; ++u) r[i][u] = __builtin_amdgcn_rcpf(den[i][u]);
#pragma unroll
  for (int i = 0; i < K; ++i) e[i] = fma2(-den[i], r[i], f2{1.0f, 1.0f});
#pragma unroll
  for (int i = 0; i < K; ++i) r[i] = fma2(e[i], r[i], r[i]);
#pragma unroll
  for (int i = 0; i < K; ++i) m[i] = num[i] * r[i];
#pragma unroll
  for (int i = 0; i < K; ++i) e[i] = fma2(-den[i], m[i], num[i]);
#pragma unroll
  for (int i = 0; i < K; ++i) m[i] = fma2(e[i], r[i], m[i]);
#pragma unroll
  for (int i = 0; i < K; ++i) e[i] = fma2(-den[i], m[i], num[i]);
#pragma unroll
  for (int i = 0; i < K; ++i)
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const float v = __builtin_amdgcn_div_fmasf(e[i][u], r[i][u], m[i][u], fl[i][u]);
      q[i][u] = __builtin_amdgcn_div_fixupf(v, y[i][u], x[i][u]);
    }
  (void)f0;
}

// np.clip(x, -4.97f, 4.97f): one v_med3_f32 per component; a NaN must pass, which only a pair with a NaN
// input can hold (nan_in, wave-uniform; every other message is finite)
__device__ __forceinline__ f2 clip497(f2 x, int nan_in) {
  f2 y;
#pragma unroll
  for (int u = 0; u < 2; ++u) y[u] = __builtin_amdgcn_fmed3f(x[u], -4.97f, 4.97f);
  if (nan_in) {
#pragma unroll
    for (int u = 0; u < 2; ++u) y[u] = x[u] != x[u] ? x[u] : y[u];
  }
  return y;
}

// toc = fast_tanh(-Tnm / 2) (ldpc_decoder.py:11-20, 97) of kDivGroup arguments Tnm, in place
__device__ __forceinline__ void tanh_group(f2* v, int nan_in) {
  f2 na[kDivGroup], nb[kDivGroup];
#pragma unroll
  for (int i = 0; i < kDivGroup; ++i) {
    const f2 x = clip497(v[i] * -0.5f, nan_in);   // -Tnm / 2: the same real value, rounded once
    const f2 x2 = x * x;
    na[i] = x * (945.0f + x2 * (105.0f + x2));
    nb[i] = 945.0f + x2 * (420.0f + x2 * 15.0f);
  }
  div_rn32<kDivGroup>(v, na, nb);
}

// tov = -2 fast_atanh(Tmn) (ldpc_decoder.py:22-30, 108) of kDivGroup products, in place
__device__ __forceinline__ void atanh_group(f2* v) {
  f2 na[kDivGroup], nb[kDivGroup];
#pragma unroll
  for (int i = 0; i < kDivGroup; ++i) {
    const f2 x = v[i], x2 = x * x;
    na[i] = x * (945.0f + x2 * (-735.0f + x2 * 64.0f));
    nb[i] = 945.0f + x2 * (-1050.0f + x2 * 225.0f);
  }
  div_rn32<kDivGroup>(v, na, nb);
#pragma unroll
  for (int i = 0; i < kDivGroup; ++i) v[i] = v[i] * -2.0f;
}

struct LeftAddr {
  uint32_t rb, f0, f1, st;
};
__device__ __forceinline__ LeftAddr left_addr(uint32_t msg0, int lane) {
  const int q3 = left_q3(lane);
  LeftAddr a;
  a.rb = msg0 + 8u * (uint32_t)(kWave + left_r(lane));
  a.f0 = a.rb + (uint32_t)(kRowB * left_f0(q3));
  a.f1 = a.rb + (uint32_t)(kRowB * left_f1(q3));
  a.st = a.rb + (uint32_t)(kRowB * q3);
  return a;
}

// the products of the lane's own check (row m' = lane): x[q] = the product of the check's toc but t[q],
// left to right from 1.0 (1.0 * t0 == t0, so a chain starts at its first factor); edges q >= 2 share the
// prefix (..(t0 t1)..) t[q-1] bit for bit.  A degree-6 row's t[6] is the constant 1.0 (p * 1.0 == p).
__device__ __forceinline__ void row_products(f2* x, uint32_t la) {
  f2 t[7];
#pragma unroll
  for (int f = 0; f < 7; ++f) t[f] = ldv(la + (uint32_t)(kRowB * f));
  f2 p = t[1];
#pragma unroll
  for (int f = 2; f < 7; ++f) p = p * t[f];
  x[0] = p;
  f2 pre = t[0];
#pragma unroll
  for (int q = 1; q < 7; ++q) {
    p = pre;
#pragma unroll
    for (int f = q + 1; f < 7; ++f) p = p * t[f];
    x[q] = p;
    pre = pre * t[q];
  }
}

// the products of the lane's two leftover edges (row 64 + r, positions q3 and 3 + q3)
__device__ __forceinline__ void left_products(f2* x, const LeftAddr& a) {
  f2 p = ldv(a.f0) * ldv(a.f1);      // slot A: (t1 | t0) (t1 | t2) t3 t4 t5
#pragma unroll
  for (int f = 3; f < 6; ++f) p = p * ldv(a.rb + (uint32_t)(kRowB * f));
  x[0] = p;
  p = ldv(a.rb);                     // slot B: t0 t1 t2 (t4 | t3) (t4 | t5)
#pragma unroll
  for (int f = 1; f < 3; ++f) p = p * ldv(a.rb + (uint32_t)(kRowB * f));
  p = p * ldv(a.f0 + (uint32_t)(kRowB * 3));
  p = p * ldv(a.f1 + (uint32_t)(kRowB * 3));
  x[1] = p;
}

// what the host knows of one candidate of the pair (wave-uniform)
struct Cand32 {
  int have;                  // an item of the launch with a candidate behind it
  unsigned item;
  int slot, at, af, cidx;
  double score;
};

// k_bp's outputs of one candidate: the plain hard decision, and the record with the CRC-14 tail
__device__ void write_outputs(const Bp32Args& a, Wave32Lds& L, const Cand32& c, const uint64_t (&hd)[kVarSlots],
                              int min_errors, int lane) {
  const bool pack = a.res && min_errors == 0;
  if (a.plain_out || pack) {
#pragma unroll
    for (int j = 0; j < kVarSlots; ++j) L.bits[lane + kWave * j] = (uint8_t)((hd[j] >> lane) & 1u);
    __syncthreads();
  }
  if (a.plain_out)
    for (int n = lane; n < FT8_LDPC_N; n += kWave) a.plain_out[(int64_t)c.item * FT8_LDPC_N + n] = L.bits[n];
  if (a.res) {
    // pack 91 bits MSB first (ft8_decode.py:200-215)
    if (pack && lane < 12) {
      const uint64_t w = *reinterpret_cast<const uint64_t*>(&L.bits[8 * lane]);
      const uint32_t lo = (uint32_t)w, hi = (uint32_t)(w >> 32);
      unsigned byte = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) byte |= ((lo >> (8 * j)) & 1u) << (7 - j);
#pragma unroll
      for (int j = 0; j < 4; ++j) byte |= ((hi >> (8 * j)) & 1u) << (3 - j);
      if (lane == 11) byte &= 0xE0u;  // bits 88..90 end the 91-bit message
      L.a91[lane] = (uint8_t)byte;
    }
    __syncthreads();
    if (lane == 0) {
      ft8_result r;
      r.score = c.score;
      r.slot = a.slot0 + c.slot;
      r.abs_time = c.at;
      r.abs_freq = c.af;
      r.ldpc_errors = (int16_t)min_errors;
      r.cand_index = (uint16_t)c.cidx;
      r.crc_extracted = 0;
      r.crc_calculated = 0;
      r.ok = 0;
      r.pass_index = 0;
      for (int i = 0; i < 10; ++i) r.payload[i] = 0;
      if (min_errors == 0) {
        const uint8_t* a91 = L.a91;
        const unsigned ce = ((a91[9] & 7u) << 11) | ((unsigned)a91[10] << 3) | (a91[11] >> 5);
        uint8_t buf[12];
        for (int i = 0; i < 10; ++i) buf[i] = a91[i];
        buf[9] &= 0xF8;
        buf[10] = 0;
        buf[11] = 0;
        unsigned rem = 0;  // crc.py:11-39
        for (int ib = 0; ib < 82; ++ib) {
          if ((ib & 7) == 0) rem ^= (unsigned)buf[ib >> 3] << 6;
          rem = (rem & 0x2000u) ? ((rem << 1) ^ 0x2757u) : (rem << 1);
        }
        const unsigned cc = rem & 0x3FFFu;
        r.crc_extracted = (uint16_t)ce;
        r.crc_calculated = (uint16_t)cc;
        if (ce == cc) {
          r.ok = 1;
          for (int i = 0; i < 10; ++i) r.payload[i] = a91[i];
          r.payload[9] &= 0xF8;
        }
      }
      a.res[c.item] = r;
    }
  }
  __syncthreads();  // bits / a91 are free for the pair's other candidate
}

// ---- k_bp32: persistent waves, two candidates at a time --------------------------------------------
// modes: 0 per-slot candidate lists (records carry slot / abs_time / abs_freq / score), 2 plain LLRs.
// A single-wave workgroup: no FT8_RACE_PROLOGUE (ft8_internal.h asks for it from two waves on).
__global__ __launch_bounds__(kWave) void k_bp32(Bp32Args a) {
  const unsigned long long clk0 = a.clock ? clock64() : 0ull, wall0 = a.clock ? wall_clock64() : 0ull;
  __shared__ Wave32Lds L;
  const int lane = threadIdx.x;
  Wave32Tables tb;
  load_tables(tb, L, lane);
  // padding variables (variable slot 2, lanes >= 46) never store their messages
  const bool var2 = lane + kWave * (kVarSlots - 1) < FT8_LDPC_N;
  const uint64_t var2_mask = (1ull << (FT8_LDPC_N - kWave * (kVarSlots - 1))) - 1ull;
  uint32_t la = lds_addr(&L.msg[0]) + 8u * (uint32_t)lane;
  asm volatile("" : "+v"(la));
  LeftAddr lf = left_addr(la - 8u * (uint32_t)lane, lane);
  asm volatile("" : "+v"(lf.rb), "+v"(lf.f0), "+v"(lf.f1), "+v"(lf.st));

  unsigned st_cand = 0, st_iter = 0, st_pass = 0, st_conv = 0;
  for (;;) {
    unsigned long long ticket = 0;
    if (lane == 0) ticket = atomicAdd(a.work, (unsigned long long)kPair);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)ticket);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(ticket >> 32));
    // tickets of this launch start at work_base and come in pairs; a wave retires at its first pair
    // past the items (launch_bp32 advances the host base by what that consumes)
    const unsigned long long rel = (((unsigned long long)hi << 32) | lo) - a.work_base;
    if (rel >= (unsigned long long)a.n_items) break;

    Cand32 cd[kPair];
#pragma unroll
    for (int u = 0; u < kPair; ++u) {
      Cand32& c = cd[u];
      c.item = (unsigned)rel + (unsigned)u;
      c.have = c.item < (unsigned)a.n_items ? 1 : 0;
      c.slot = c.at = c.af = c.cidx = 0;
      c.score = 0.0;
      if (c.have && a.mode == 0) {
        c.slot = c.item / a.N;
        c.cidx = c.item % a.N;
        if (c.cidx >= a.cand_count[c.slot]) {
          c.have = 0;
        } else {
          c.at = a.cand[((int64_t)c.slot * a.N + c.cidx) * 2];
          c.af = a.cand[((int64_t)c.slot * a.N + c.cidx) * 2 + 1];
          c.score = a.cand_score[(int64_t)c.slot * a.N + c.cidx];
        }
      }
    }
    if (!(cd[0].have | cd[1].have)) continue;

    // c = (float)llr, round to nearest (beyond float32's range: +-inf; below it: subnormal or 0).
    // Padding variables and an absent candidate hold -1.0: bounded messages, a hard decision of 0.
    f2 cv[kVarSlots];
#pragma unroll
    for (int j = 0; j < kVarSlots; ++j) {
      const int n = lane + kWave * j;
#pragma unroll
      for (int u = 0; u < kPair; ++u)
        cv[j][u] = (cd[u].have && n < FT8_LDPC_N) ? (float)a.llr_in[(int64_t)cd[u].item * FT8_LDPC_N + n] : -1.0f;
    }
    bool lane_nan = false;
#pragma unroll
    for (int j = 0; j < kVarSlots; ++j) lane_nan = lane_nan || cv[j].x != cv[j].x || cv[j].y != cv[j].y;
    int nan_in = __builtin_amdgcn_readfirstlane(__ballot(lane_nan) != 0 ? 1 : 0);
    asm volatile("" : "+s"(nan_in));

    // tov = 0 on every real edge (indices 0..521; the constants above never change)
#pragma unroll
    for (int i = 0; i < kEdgeSlots; ++i)
      if (i < kEdgeSlots - 1 || lane + kWave * i < FT8_LDPC_E) stv(la + 512u * i, f2{0.0f, 0.0f});
    __syncthreads();

    uint64_t hd[kPair][kVarSlots] = {};
    int min_errors[kPair] = {FT8_LDPC_M, FT8_LDPC_M};
    int entered[kPair] = {0, 0}, passes[kPair] = {0, 0};
    int done[kPair] = {!cd[0].have, !cd[1].have};  // wave-uniform
    for (int iter = 0; iter < a.max_iterations; ++iter) {
#pragma unroll
      for (int j = 0; j < kVarSlots; ++j) asm volatile("" : "+v"(tb.va[j]), "+v"(tb.va1[j]), "+v"(tb.vb[j]));
      // (A) variable-major: the hard-decision sums and the three variable->check arguments of each of the
      // lane's variables, in registers
      f2 msum[kVarSlots], T[kVarSlots][3];
#pragma unroll
      for (int j = 0; j < kVarSlots; ++j) {
        const f2 t0 = *(const lds_f2*)(uintptr_t)tb.va[j];
        const f2 t1 = *(const lds_f2*)(uintptr_t)tb.va1[j];
        const f2 t2 = *(const lds_f2*)(uintptr_t)tb.vb[j];
        const f2 c = cv[j];
        msum[j] = c + ((t0 + t1) + t2);  // messages = codeword + sum(tov, axis=1)
        const f2 c0 = c + t0;            // Tnm = codeword[n] + the other two tov in check order
        T[j][0] = (c + t1) + t2;
        T[j][1] = c0 + t2;
        T[j][2] = c0 + t1;
      }
      // (B) per candidate still running: hard decision, all-zero stop, parity, min_errors, last iteration
#pragma unroll
      for (int u = 0; u < kPair; ++u) {
        if (done[u]) continue;
        entered[u]++;
#pragma unroll
        for (int j = 0; j < kVarSlots; ++j) hd[u][j] = __ballot(msum[j][u] > 0.0f);
        hd[u][kVarSlots - 1] &= var2_mask;
        if ((hd[u][0] | hd[u][1] | hd[u][2]) == 0) {  // ldpc_decoder.py:76-78
          done[u] = 1;
          continue;
        }
        int errs = 0;
#pragma unroll
        for (int k = 0; k < kChkSlots; ++k) {
          uint32_t x = 0;
#pragma unroll
          for (int j = 0; j < kVarSlots; ++j) {
            x ^= tb.h[k][j][0] & (uint32_t)hd[u][j];
            x ^= tb.h[k][j][1] & (uint32_t)(hd[u][j] >> 32);
          }
          errs += __popcll(__ballot(__builtin_popcount(x) & 1));
        }
        if (errs < min_errors[u]) {
          min_errors[u] = errs;
          if (errs == 0) {
            done[u] = 1;
            continue;
          }
        }
        // the last iteration's message update is never read
        if (iter + 1 == a.max_iterations) done[u] = 1;
      }
      if (done[0] & done[1]) break;
      passes[0] += !done[0];
      passes[1] += !done[1];
      // (C) variable -> check messages, a variable's three edges one division group
#pragma unroll
      for (int j = 0; j < kVarSlots; ++j) {
        tanh_group(T[j], nan_in);
        if (j < kVarSlots - 1 || var2) {
          stv(tb.va[j], T[j][0]);
          stv(tb.va1[j], T[j][1]);
          stv(tb.vb[j], T[j][2]);
        }
      }
      sweep_sync();
      // (D) check -> variable messages; x[0..6]: the lane's own check, x[7..8]: its two leftover edges;
      // all reads precede the stores
      f2 x[kEdgeSlots];
      row_products(x, la);
      left_products(&x[7], lf);
#pragma unroll
      for (int g = 0; g < kEdgeSlots; g += kDivGroup) atanh_group(&x[g]);
#pragma unroll
      for (int f = 0; f < 6; ++f) stv(la + (uint32_t)(kRowB * f), x[f]);
      if (lane < kM7) stv(la + (uint32_t)(kRowB * 6), x[6]);  // rows >= 24 have a constant 1.0 there
      if (lane < kLeftLanes) {
        stv(lf.st, x[7]);
        stv(lf.st + (uint32_t)(kRowB * 3), x[8]);
      }
      sweep_sync();
    }
#pragma unroll
    for (int u = 0; u < kPair; ++u) {
      if (!cd[u].have) continue;
      st_cand++;
      st_iter += entered[u];
      st_pass += passes[u];
      st_conv += min_errors[u] == 0;
      write_outputs(a, L, cd[u], hd[u], min_errors[u], lane);
    }
  }
  const unsigned row = (blockIdx.x & (unsigned)(kStatRows - 1)) * (unsigned)kStatStride;
  if (a.stats && lane == 0 && st_cand) {
    atomicAdd(&a.stats[row + 0], (unsigned long long)st_cand);
    atomicAdd(&a.stats[row + 1], (unsigned long long)st_iter);
    atomicAdd(&a.stats[row + 2], (unsigned long long)st_pass);
    atomicAdd(&a.stats[row + 3], (unsigned long long)st_conv);
  }
  if (a.clock && lane == 0) {
    const unsigned long long cyc = clock64() - clk0, wall = wall_clock64() - wall0;
    atomicAdd(&a.clock[row + 0], cyc);
    atomicAdd(&a.clock[row + 1], wall);
    atomicMax(&a.clock[row + 2], cyc);
    atomicAdd(&a.clock[row + 3], 1ull);
  }
}

}  // namespace

hipError_t launch_bp32(const BpLaunch& L, hipStream_t s) {
  if (L.n_items <= 0) return hipSuccess;
  if (L.mode != 0 && L.mode != 2) return hipErrorInvalidValue;
  Bp32Args a{};
  a.cand = L.cand;
  a.cand_score = L.cand_score;
  a.cand_count = L.cand_count;
  a.N = L.N;
  a.n_items = L.n_items;
  a.mode = L.mode;
  a.llr_in = L.llr_in;
  a.max_iterations = L.max_iterations;
  a.plain_out = L.plain_out;
  a.res = L.res;
  a.work = L.work;
  a.work_base = L.work_base ? *L.work_base : 0ull;
  a.stats = L.stats;
  a.clock = L.clock;
  a.slot0 = L.slot0;
  const int per_simd = max(1, min(L.grid_waves, kBp32WavesPerSimd));
  const int pairs = (L.n_items + kPair - 1) / kPair;
  const int waves = min(pairs, kBp32GridCus * 4 * per_simd);  // resident waves, persistent
  hipLaunchKernelGGL(k_bp32, dim3(waves), dim3(kWave), 0, s, a);
  const hipError_t e = hipGetLastError();
  // every claim takes kPair tickets: one claim per pair of items, then one per retiring wave
  if (e == hipSuccess && L.work_base)
    *L.work_base += (unsigned long long)kPair * ((unsigned long long)pairs + (unsigned long long)waves);
  return e;
}

}  // namespace ft8
