// osd.hip -- ordered-statistics decoding of the LDPC(174,91) code, order 0 .. 2, for the candidates
// belief propagation failed on (include/ft8hip.h, "ordered-statistics decoding"; osd.py restates it).
//
// k_osd, one 256-thread workgroup per list position, all arithmetic in integers:
//   1. q = min(floor(|L| 256), 65535) and the hard decisions; a NaN or all q == 0 ends the attempt
//   2. bitonic sort of the 174 keys (65535 - q) << 8 | i (padded to 256) in LDS -> perm
//   3. the generator [I | P] with its columns in perm order, 91 bit-rows of 3 x 64 bits (bit p of a row
//      is bit p % 64 of word p / 64), built by ballot from each lane's column
//   4. per-byte weight tables T[b][v] = sum of q over the set bits of v in positions 8 b .. 8 b + 7
//   5. wave 0: Gauss-Jordan elimination over the columns in perm order, two rows per lane (pivot by
//      ballot, pivot row by shuffle) -> M, row k the one with a 1 in the k-th basis column; then c0 and
//      d0 = c0 ^ hard
//   6. the 1 / 92 / 4187 candidates d0, d0 ^ M[k], d0 ^ M[k1] ^ M[k2] strided over the threads, 22 table
//      lookups each, and a min-reduce of weight << 32 | enumeration index
//   7. the winner in natural bit order through the reference tail (tx_device.h's CRC) and the acceptance
//      test; an accepted one rewrites its record through retry_accept with 0xF0
#include "ft8_internal.h"
#include "tx_device.h"

namespace ft8 {
namespace {

constexpr int kOsdThreads = 256;
static_assert(sizeof(ft8_osd_rec) == 12, "ft8_osd_rec layout");
constexpr int kK = FT8_LDPC_K, kN = FT8_LDPC_N;   // 91, 174
constexpr int kBytes = 22;                        // 174 bits
constexpr int kQMax = 65535;
constexpr unsigned kFirstPair = 1 + kK;           // enumeration index of (k1, k2) = (0, 1)

struct OsdLds {
  int32_t T[kBytes][256];     // step 4
  uint32_t keys[256];         // step 2
  uint64_t M[kK][3];          // steps 3 and 5
  uint64_t hp[3], d0[3];      // hard decisions in perm order; c0 ^ hard
  uint64_t best[kOsdThreads / kWave];
  int32_t qp[kBytes * 8];     // q in perm order, 0 past 174
  uint8_t perm[kN];
  uint8_t hard[kN + 2];       // natural order; later the winner's bits in natural order (+ 2 zero bits)
};

__device__ __forceinline__ uint64_t shfl64(uint64_t v, int src) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src);
  return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int mask) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, mask), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), mask);
  return ((uint64_t)hi << 32) | lo;
}
// bit p of a 174-bit row (selects, so a row held in registers stays there)
__device__ __forceinline__ bool bit_of(const uint64_t (&w)[3], int p) {
  const uint64_t x = p < 64 ? w[0] : p < 128 ? w[1] : w[2];
  return (x >> (p & 63)) & 1ull;
}

// rule 5 through the tables: 22 lookups
__device__ __forceinline__ int32_t weight_of(const OsdLds& L, uint64_t w0, uint64_t w1, uint64_t w2) {
  int32_t s = 0;
#pragma unroll
  for (int b = 0; b < 8; ++b) s += L.T[b][(w0 >> (8 * b)) & 0xFF];
#pragma unroll
  for (int b = 0; b < 8; ++b) s += L.T[8 + b][(w1 >> (8 * b)) & 0xFF];
#pragma unroll
  for (int b = 0; b < 6; ++b) s += L.T[16 + b][(w2 >> (8 * b)) & 0xFF];
  return s;
}

// enumeration index of the pair k1 < k2, and back
__device__ __forceinline__ unsigned pair_index(int k1, int k2) {
  return kFirstPair + (unsigned)(k1 * (2 * kK - 1 - k1) / 2 + (k2 - k1 - 1));
}

__device__ __forceinline__ void write_skipped(const OsdLaunch& a, int64_t src, int status) {
  const int t = threadIdx.x;
  if (a.info && t == 0) a.info[src] = ft8_osd_rec{0, -1, {-1, -1}, 0, (uint8_t)status};
  if (a.codeword && t < kBytes) a.codeword[src * kBytes + t] = 0;
}

__global__ __launch_bounds__(kOsdThreads) void k_osd(OsdLaunch a) {
  FT8_RACE_PROLOGUE();
  __shared__ OsdLds L;
  const int t = threadIdx.x, lane = t % kWave, wave = t / kWave;
  const int64_t pos = blockIdx.x;
  const int slot = (int)(pos / a.M), j = (int)(pos % a.M);
  if (slot >= a.n_slots || j >= (a.count ? min(a.M, max(a.count[slot], 0)) : a.M)) return;
  const int orig = a.list ? a.list[pos] : j;
  if (orig < 0 || orig >= a.N) return;
  const int64_t src = (int64_t)slot * a.N + orig;
  ft8_result* rec = a.res + src;
  if (rec->ok) {   // workgroup-uniform
    write_skipped(a, src, 3);
    return;
  }

  // ---- 1. reliabilities ------------------------------------------------------------------------
  int q = 0;
  bool nan = false;
  if (t < kN) {
    const double v = a.llr[src * kN + t];
    nan = v != v;
    const double m = fabs(v) * 256.0;             // exact: a power of two
    q = nan ? 0 : (m >= (double)kQMax ? kQMax : (int)m);
    L.hard[t] = v > 0.0;
  }
  const int any_nan = __syncthreads_or(nan);
  const int any_q = __syncthreads_or(q != 0);
  if (any_nan || !any_q) {
    write_skipped(a, src, 2);
    return;
  }

  // ---- 2. order: q descending, equal q by index ascending ---------------------------------------
  L.keys[t] = t < kN ? ((uint32_t)(kQMax - q) << 8) | (uint32_t)t : 0xFFFFFFFFu;
  __syncthreads();
  for (int k = 2; k <= kOsdThreads; k <<= 1) {
    for (int s = k >> 1; s > 0; s >>= 1) {
      const int o = t ^ s;
      if (o > t) {
        const uint32_t x = L.keys[t], y = L.keys[o];
        if ((x > y) == ((t & k) == 0)) {
          L.keys[t] = y;
          L.keys[o] = x;
        }
      }
      __syncthreads();
    }
  }
  const int col = t < kN ? (int)(L.keys[t] & 0xFFu) : 0;   // this thread's position p = t holds bit `col`
  if (t < kN) L.perm[t] = (uint8_t)col;
  if (t < kBytes * 8) L.qp[t] = t < kN ? kQMax - (int)(L.keys[t] >> 8) : 0;
  {
    const uint64_t m = __ballot(t < kN && L.hard[col]);
    if (lane == 0 && wave < 3) L.hp[wave] = m;
  }

  // ---- 3. the generator's columns in perm order, as bit-rows ------------------------------------
  if (wave < 3) {
    uint64_t c0 = 0, c1 = 0;   // this lane's column: bit k of (c0: rows 0 .. 63, c1: rows 64 .. 90)
    if (t < kN) {
      if (col < kK) {
        if (col < 64) c0 = 1ull << col;
        else c1 = 1ull << (col - 64);
      } else {   // parity row col - 91, 91 bits MSB first
        const uint8_t* g = tx::kGenRowsTx + (col - kK) * 12;
        c0 = __builtin_bitreverse64(tx::be64(g, 8));
        c1 = __builtin_bitreverse64(tx::be64(g + 8, 4));
      }
    }
    for (int k = 0; k < kK; ++k) {
      const uint64_t m = __ballot(((k < 64 ? c0 >> k : c1 >> (k - 64)) & 1ull) != 0);
      if (lane == 0) L.M[k][wave] = m;
    }
  }
  __syncthreads();

  // ---- 4. weight tables -------------------------------------------------------------------------
  for (int b = 0; b < kBytes; ++b) {
    int32_t s = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) s += ((t >> i) & 1) ? L.qp[8 * b + i] : 0;
    L.T[b][t] = s;
  }

  // ---- 5. elimination, c0, d0 (wave 0; lane l holds rows l and l + 64) --------------------------
  if (wave == 0) {
    const bool has_b = lane + 64 < kK;
    uint64_t ra[3], rb[3];
#pragma unroll
    for (int w = 0; w < 3; ++w) {
      ra[w] = L.M[lane][w];
      rb[w] = has_b ? L.M[lane + 64][w] : 0ull;
    }
    int pa = -1, pb = -1, ca = 0, cb = 0;   // the rows' pivot rank k and pivot column
    int rank = 0;
    for (int p = 0; p < kN && rank < kK; ++p) {
      const int w = p >> 6, sh = p & 63;
      const uint64_t wa = w == 0 ? ra[0] : w == 1 ? ra[1] : ra[2];
      const uint64_t wb = w == 0 ? rb[0] : w == 1 ? rb[1] : rb[2];
      const bool ba = (wa >> sh) & 1ull, bb = (wb >> sh) & 1ull;
      const uint64_t ma = __ballot(ba && pa < 0), mb = __ballot(bb && pb < 0);
      if ((ma | mb) == 0) continue;   // dependent on the basis columns before it
      const bool from_a = ma != 0;
      const int piv = from_a ? __ffsll((unsigned long long)ma) - 1 : __ffsll((unsigned long long)mb) - 1;
      uint64_t pr[3];
#pragma unroll
      for (int x = 0; x < 3; ++x) pr[x] = shfl64(from_a ? ra[x] : rb[x], piv);
      const bool me_a = from_a && lane == piv, me_b = !from_a && lane == piv;
      if (ba && !me_a) {
#pragma unroll
        for (int x = 0; x < 3; ++x) ra[x] ^= pr[x];
      }
      if (bb && !me_b) {
#pragma unroll
        for (int x = 0; x < 3; ++x) rb[x] ^= pr[x];
      }
      if (me_a) pa = rank, ca = p;
      if (me_b) pb = rank, cb = p;
      ++rank;
    }
    uint64_t hp[3], c0[3];
#pragma unroll
    for (int w = 0; w < 3; ++w) hp[w] = L.hp[w];
    const bool sa = pa >= 0 && bit_of(hp, ca), sb = pb >= 0 && bit_of(hp, cb);
#pragma unroll
    for (int w = 0; w < 3; ++w) {
      uint64_t x = (sa ? ra[w] : 0ull) ^ (sb ? rb[w] : 0ull);
      for (int d = kWave / 2; d > 0; d >>= 1) x ^= shfl_xor64(x, d);
      c0[w] = x;
    }
#pragma unroll
    for (int w = 0; w < 3; ++w) {
      if (pa >= 0) L.M[pa][w] = ra[w];
      if (pb >= 0) L.M[pb][w] = rb[w];
    }
    if (lane == 0)
      for (int w = 0; w < 3; ++w) L.d0[w] = c0[w] ^ hp[w];
  }
  __syncthreads();

  // ---- 6. search ----------------------------------------------------------------------------------
  const uint64_t d0 = L.d0[0], d1 = L.d0[1], d2 = L.d0[2];
  uint64_t best = ~0ull;
  if (t == 0) best = (uint64_t)(uint32_t)weight_of(L, d0, d1, d2) << 32;
  if (a.order >= 1 && t < kK) {
    const uint64_t key = ((uint64_t)(uint32_t)weight_of(L, d0 ^ L.M[t][0], d1 ^ L.M[t][1], d2 ^ L.M[t][2]) << 32) |
                         (uint32_t)(1 + t);
    best = key < best ? key : best;
  }
  if (a.order >= 2) {
    for (int g = t; g < kK * kK; g += kOsdThreads) {
      const int k1 = g / kK, k2 = g % kK;
      if (k1 >= k2) continue;
      const int32_t w = weight_of(L, d0 ^ L.M[k1][0] ^ L.M[k2][0], d1 ^ L.M[k1][1] ^ L.M[k2][1],
                                  d2 ^ L.M[k1][2] ^ L.M[k2][2]);
      const uint64_t key = ((uint64_t)(uint32_t)w << 32) | pair_index(k1, k2);
      best = key < best ? key : best;
    }
  }
  for (int d = kWave / 2; d > 0; d >>= 1) {
    const uint64_t o = shfl_xor64(best, d);
    best = o < best ? o : best;
  }
  if (lane == 0) L.best[wave] = best;
  __syncthreads();
  best = L.best[0];
  for (int w = 1; w < kOsdThreads / kWave; ++w) best = L.best[w] < best ? L.best[w] : best;

  // ---- 7. the winner: flips, natural bit order, tail, acceptance --------------------------------------
  const int32_t weight = (int32_t)(best >> 32);
  const unsigned e = (unsigned)(best & 0xFFFFFFFFull);
  int k1 = -1, k2 = -1, n_flips = 0;
  if (e >= kFirstPair) {
    unsigned idx = e - kFirstPair;
    k1 = 0;
    while (k1 < kK - 2 && idx >= (unsigned)(kK - 1 - k1)) idx -= (unsigned)(kK - 1 - k1), ++k1;
    k2 = min(k1 + 1 + (int)idx, kK - 1);
    n_flips = 2;
  } else if (e >= 1) {
    k1 = (int)e - 1;
    n_flips = 1;
  }
  uint64_t d[3] = {d0, d1, d2};
#pragma unroll
  for (int w = 0; w < 3; ++w) {
    if (k1 >= 0) d[w] ^= L.M[k1][w];
    if (k2 >= 0) d[w] ^= L.M[k2][w];
  }
  const int n_hard = __popcll(d[0]) + __popcll(d[1]) + __popcll(d[2]);
  // every thread is past its reads of L.hard (step 2) since the barriers of step 3
  if (t < kN) L.hard[col] = (uint8_t)(bit_of(d, t) != bit_of(L.hp, t));
  if (t >= kN && t < kN + 2) L.hard[t] = 0;
  __syncthreads();
  uint8_t* cw = reinterpret_cast<uint8_t*>(L.keys);   // the sort is over: 22 bytes, MSB first
  if (t < kBytes) {
    unsigned byte = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) byte |= (unsigned)L.hard[8 * t + i] << (7 - i);
    cw[t] = (uint8_t)byte;
    if (a.codeword) a.codeword[src * kBytes + t] = (uint8_t)byte;
  }
  __syncthreads();
  if (t == 0) {
    // the reference tail on plain = codeword, ldpc_errors = 0 (bp.hip's epilogue; crc.py:41-54)
    ft8_result got{};
    const unsigned ce = ((cw[9] & 7u) << 11) | ((unsigned)cw[10] << 3) | (cw[11] >> 5);
    uint8_t pay[10];
    for (int i = 0; i < 10; ++i) pay[i] = cw[i];
    pay[9] &= 0xF8;
    const unsigned cc = tx::crc14_words(tx::be64(pay, 8), tx::be64(pay + 8, 2), 82);
    bool nonzero = false;
    for (int i = 0; i < 10; ++i) {
      got.payload[i] = pay[i];
      nonzero |= pay[i] != 0;
    }
    got.crc_extracted = (uint16_t)ce;
    got.crc_calculated = (uint16_t)cc;
    got.ldpc_errors = 0;
    const bool accept = ce == cc && n_hard <= a.max_hard && nonzero;
    if (accept) retry_accept(rec, got, 0xF0);
    if (a.info)
      a.info[src] = ft8_osd_rec{weight, (int16_t)n_hard, {(int16_t)k1, (int16_t)k2}, (uint8_t)n_flips,
                                (uint8_t)(accept ? 0 : 1)};
  }
}

}  // namespace

hipError_t launch_osd(const OsdLaunch& a, hipStream_t s) {
  if (a.n_slots <= 0 || a.M <= 0 || a.N <= 0) return hipSuccess;
  if (a.order < 0 || a.order > 2 || (int64_t)a.n_slots * a.M > (int64_t)INT32_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_osd, dim3((unsigned)(a.n_slots * a.M)), dim3(kOsdThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace ft8
