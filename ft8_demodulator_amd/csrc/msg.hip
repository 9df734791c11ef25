// msg.hip -- the message layer on the device: ft8_result records -> ft8_text (k_unpack77), and the
// two host entry points that reach the same unpacker without a context or a GPU
// (ft8_unpack77_host, ft8_hash_call).  The field arithmetic is msg77.h's, for both.
#include <cstring>

#include "ft8_internal.h"
#include "msg77.h"

namespace ft8 {

// ---- k_unpack77 -----------------------------------------------------------------------------------
// One workgroup per slot, one lane per record (looping when cap exceeds the workgroup).  Each lane
// unpacks its record's payload and looks for the first earlier ok record of the slot with the same
// 77 bits.  The search compares a 16-byte key per record: payload bytes 0..7, then byte 8, byte 9 &
// 0xF8 and the ok flag -- a record that is not ok therefore never equals the key of a searching
// (ok) record.  The slot's keys are staged in LDS when cap <= kMsgStageCap (48 KB); a larger cap
// reads them from the records.  Every lane of a wave reads the same key j at the same time (an LDS
// broadcast), so the search costs one LDS read per comparison per wave.
constexpr int kMsgThreads = 256;
constexpr int kMsgStageCap = 3072;

__device__ __forceinline__ void load_key(const ft8_result* r, uint64_t& hi, uint64_t& lo) {
  const uint8_t* p = r->payload;
  uint64_t h = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) h = (h << 8) | p[i];
  hi = h;
  lo = (uint64_t)p[8] | ((uint64_t)(p[9] & 0xF8) << 8) | ((uint64_t)(r->ok != 0) << 16);
}

__global__ __launch_bounds__(kMsgThreads) void k_unpack77(const ft8_result* rec, const int32_t* counts, int cap,
                                                          int staged, ft8_text* out) {
  FT8_RACE_PROLOGUE();
  extern __shared__ uint64_t s_key[];  // staged: [n][2]
  const int s = blockIdx.x, tid = threadIdx.x;
  const int n = counts ? min(max(counts[s], 0), cap) : cap;
  const ft8_result* R = rec + (int64_t)s * cap;
  ft8_text* O = out + (int64_t)s * cap;
  if (staged) {
    for (int r = tid; r < n; r += kMsgThreads) {
      uint64_t hi, lo;
      load_key(R + r, hi, lo);
      s_key[2 * r] = hi;
      s_key[2 * r + 1] = lo;
    }
    __syncthreads();
  }
  for (int r = tid; r < cap; r += kMsgThreads) {
    ft8_text t;
    uint64_t hi = 0, lo = 0;
    if (r < n) {
      if (staged) hi = s_key[2 * r], lo = s_key[2 * r + 1];
      else load_key(R + r, hi, lo);
    }
    if (!((lo >> 16) & 1)) {  // past the count, or not ok
      msg77::not_ok(&t);
    } else {
      uint8_t p[10];
#pragma unroll
      for (int i = 0; i < 8; ++i) p[i] = (uint8_t)(hi >> (8 * (7 - i)));
      p[8] = (uint8_t)lo;
      p[9] = (uint8_t)(lo >> 8);
      msg77::unpack(p, &t);
      int dup = -1;
      for (int j = 0; j < r; ++j) {
        uint64_t h2, l2;
        if (staged) h2 = s_key[2 * j], l2 = s_key[2 * j + 1];
        else load_key(R + j, h2, l2);
        if (h2 == hi && l2 == lo) {
          dup = j;
          break;
        }
      }
      t.dup_of = (int16_t)dup;
    }
    O[r] = t;
  }
}

hipError_t launch_unpack77(const ft8_result* rec, const int32_t* counts, int n_slots, int cap, ft8_text* out,
                           hipStream_t s) {
  if (n_slots <= 0 || cap <= 0) return hipSuccess;
  const int staged = cap <= kMsgStageCap;
  const size_t lds = staged ? (size_t)cap * 2 * sizeof(uint64_t) : 0;
  hipLaunchKernelGGL(k_unpack77, dim3(n_slots), dim3(kMsgThreads), lds, s, rec, counts, cap, staged, out);
  return hipGetLastError();
}

}  // namespace ft8

int ft8_unpack77_host(const uint8_t* payloads, int32_t n, ft8_text* out) {
  if (n < 0 || (n > 0 && (!payloads || !out))) return FT8_E_ARG;
  for (int32_t i = 0; i < n; ++i) msg77::unpack(payloads + 10 * (size_t)i, out + i);
  return FT8_OK;
}

int ft8_hash_call(const char* call, uint32_t* n22) {
  if (!call || !n22) return FT8_E_ARG;
  const size_t len = strnlen(call, 12);
  if (len > 11) return FT8_E_ARG;
  return msg77::hash22(call, (int)len, n22) == 0 ? FT8_OK : FT8_E_ARG;
}
