// ft4_device.h -- the FT4 frame layout and transmit chain as device functions (gfx950), beside
// tx_device.h whose CRC-14 and LDPC generator it reuses (ft8hip.h, "FT4"; ft8_demodulator_amd/ft4.py
// states the same in NumPy).
//
//   payload (77 bits) ^ rvec -> a91 = scrambled | CRC-14 -> 174-bit codeword          tx::encode
//   codeword -> 87 Gray-mapped 2-bit symbols + the four sync groups -> 103 tones
//   tones -> GFSK phase in closed form, as tx_device.h derives it, with BT = 1.0, no extension pulses
//   and one ramp symbol on either side: the waveform has 105 nsps samples, sample n belongs to symbol
//   n / nsps - 1, and symbol j's frequency pulse (length 3 nsps) starts at waveform sample j nsps:
//     phi(n) = 2 pi / fs * (f0 * n + spacing * G(n)),  G(u) = sum_{j=0}^{102} tone_j P(u - j nsps)
//   with P the cumulative pulse (0 for x <= 0, P(3 nsps) beyond) and G(0) = 0.
#pragma once
#include "tx_device.h"

namespace ft8 {
namespace ft4 {

constexpr int kSymbols = FT8_FT4_SYMBOLS;   // 103
constexpr int kDataSymbols = 87;
constexpr int kWaveSymbols = kSymbols + 2;  // with the ramp symbols
constexpr int kSyncStride = 33;             // sync group m starts at symbol 33 m
constexpr int kCostasC[4][4] = {{0, 1, 3, 2}, {1, 0, 2, 3}, {2, 3, 1, 0}, {3, 2, 0, 1}};
// the same table for device code, two bits per entry (entry 4 m + k at bits 8 m + 2 k)
__host__ __device__ constexpr int costas(int m, int k) { return (int)((0x4B1EE1B4u >> (8 * m + 2 * k)) & 3u); }
constexpr bool costas_packed_ok() {
  for (int m = 0; m < 4; ++m)
    for (int k = 0; k < 4; ++k)
      if (costas(m, k) != kCostasC[m][k]) return false;
  return true;
}
static_assert(costas_packed_ok(), "the packed sync tones are the table's");
// Gray map {0, 1, 3, 2}: the tone of the two bits j (its own inverse)
__host__ __device__ constexpr int gray(int j) { return j ^ (j >> 1); }
static_assert(gray(0) == 0 && gray(1) == 1 && gray(2) == 3 && gray(3) == 2, "Gray map");
namespace {
__constant__ uint8_t kRvecD[10] = {0x4a, 0x5e, 0x89, 0xb4, 0xb0, 0x8a, 0x79, 0x55, 0xbe, 0x28};  // 77 bits, MSB first
}  // namespace

// symbol of data symbol k (0 .. 86)
__host__ __device__ constexpr int data_symbol(int k) { return k + (k < 29 ? 4 : k < 58 ? 8 : 12); }

// payload -> a91[12], codeword[22], tones[103] (each nullable)
__device__ inline void encode(const uint8_t* payload, uint8_t* a91, uint8_t* cw, uint8_t* tones) {
  uint8_t scr[10], c[22];
#pragma unroll
  for (int i = 0; i < 10; ++i) scr[i] = payload[i] ^ kRvecD[i];
  tx::encode(scr, 10, a91, c, nullptr);
  if (cw) {
#pragma unroll
    for (int i = 0; i < 22; ++i) cw[i] = c[i];
  }
  if (tones) {
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int k = 0; k < 4; ++k) tones[kSyncStride * m + k] = (uint8_t)costas(m, k);
    for (int k = 0; k < kDataSymbols; ++k) {
      const int i = 2 * k;   // bits i, i + 1 share a byte (i is even)
      const unsigned v = (c[i >> 3] >> (6 - (i & 7))) & 3u;
      tones[data_symbol(k)] = (uint8_t)gray((int)v);
    }
  }
}

// G(u) for u in [0, 105 nsps): E[0 .. 102] the tones, PS[k] = sum_{i<k} E[i] (k = 0 .. 103), P[0 .. 3 nsps]
__device__ __forceinline__ double gfsk_G(const int* E, const int* PS, const double* P, int nsps, int u) {
  const int q = u / nsps, r = u - q * nsps;                    // u >= 0
  const int full = min(max(q - 2, 0), kSymbols);               // pulses j <= q - 3 are complete
  double s = (double)PS[full] * P[3 * nsps];
  if (q - 2 >= 0 && q - 2 < kSymbols) s += (double)E[q - 2] * P[r + 2 * nsps];
  if (q - 1 >= 0 && q - 1 < kSymbols) s += (double)E[q - 1] * P[r + nsps];
  if (q < kSymbols) s += (double)E[q] * P[r];
  return s;
}

// the envelope at waveform sample n of L = 105 nsps
template <typename T>
__device__ __forceinline__ T ramp(int n, int L, int nsps) {
  if (n < nsps) return (T)0.5 * ((T)1 - cos((T)M_PI * (T)n / (T)nsps));
  const int i = L - 1 - n;
  if (i < nsps) return (T)0.5 * ((T)1 - cos((T)M_PI * (T)i / (T)nsps));
  return (T)1;
}

}  // namespace ft4
}  // namespace ft8
