// msg77_check -- csrc/msg77.h on the host, alone: the known vectors, then seeded random payloads,
// each result checked for what must hold of any record.  Meant to be built with
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover
// so that an out-of-bounds write, a shift or an overflow in the field arithmetic stops it
// (tests/test_message77.py builds and runs it).  Usage: msg77_check [n_random = 1000000]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../ft8_demodulator_amd/csrc/msg77.h"

namespace {

struct Vec {
  const char* hex;
  const char* text;
};
const Vec kVectors[] = {
    {"000000204def1a8a1988", "CQ K1ABC FN42"},
    {"09bde3506149dc1faa08", "K1ABC W9XYZ -11"},
    {"0c293b804def1abfaa88", "W9XYZ K1ABC R-09"},
    {"09bde3506149dc1fa4c8", "K1ABC W9XYZ RR73"},
    {"09bde3506149dc1fbd48", "K1ABC W9XYZ -35"},
    {"000046f04def1a8a1988", "CQ DX K1ABC FN42"},
    {"000007e06149dc085648", "CQ 123 W9XYZ EN37"},
    {"0c293b884def1aea1988", "W9XYZ/R K1ABC/R R FN42"},
    {"090c166dbdd62a113590", "G4ABC/P PA9XYZ JO22"},
    {"09bde3501a95851fa508", "K1ABC <...> 73"},
    {"63edcee2a4ae07f50000", "TNX BOB 73 GL"},
    {"2468acf13579bde02540", "123456789ABCDEF012"},
    {"56b001a3a311caa00460", "CQ PJ4/K1ABC"},
    {"f31001a3a311caa00520", "<...> PJ4/K1ABC RR73"},
    {"f31001a3a311caa007a0", "PJ4/K1ABC <...> 73"},
    {"000000011ba611923748", "DE 3DA0XYZ KG53"},
    {"00000015f376e01fa448", "QRZ 3XA7AB"},
};

int nibble(char c) { return c <= '9' ? c - '0' : c - 'a' + 10; }

// what holds of every record the unpacker writes
bool sane(const ft8_text& t) {
  if (t.status > 2 || t.dup_of != -1) return false;
  if (t.text[27] != 0 || t.learn_call[11] != 0) return false;
  const size_t n = strnlen(t.text, sizeof t.text);
  for (size_t i = 0; i < sizeof t.text; ++i) {
    const char c = t.text[i];
    if (i < n ? (c < 0x20 || c > 0x7e) : c != 0) return false;
  }
  if (n && (t.text[0] == ' ' || t.text[n - 1] == ' ')) return false;
  if (t.status != 0 && (n || t.learn_call[0] || t.hash_bits[0] || t.hash_bits[1] || t.learn_hash22)) return false;
  for (int k = 0; k < 2; ++k) {
    if (t.hash_bits[k] != 0 && t.hash_bits[k] != 12 && t.hash_bits[k] != 22) return false;
    if (t.hash_bits[k] ? (t.hash[k] >> t.hash_bits[k]) != 0 : t.hash[k] != 0) return false;
  }
  if (t.learn_call[0]) {
    uint32_t h = 0;
    const int len = (int)strnlen(t.learn_call, sizeof t.learn_call);
    if (msg77::hash22(t.learn_call, len, &h) != 0 || h != t.learn_hash22) return false;
  }
  for (int i = 0; i < 5; ++i)
    if (t.reserved[i]) return false;
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  const long n_random = argc > 1 ? atol(argv[1]) : 1000000;
  int bad = 0;
  for (const Vec& v : kVectors) {
    uint8_t p[10];
    for (int i = 0; i < 10; ++i) p[i] = (uint8_t)(nibble(v.hex[2 * i]) * 16 + nibble(v.hex[2 * i + 1]));
    ft8_text t;
    memset(&t, 0xA5, sizeof t);  // the unpacker must write every byte
    msg77::unpack(p, &t);
    if (t.status != 0 || strcmp(t.text, v.text) != 0 || !sane(t)) {
      printf("vector %s: expected \"%s\", got \"%.28s\" (status %d)\n", v.hex, v.text, t.text, t.status);
      ++bad;
    }
  }
  uint64_t x = 0x9E3779B97F4A7C15ull;  // splitmix64, seeded
  long by_status[3] = {0, 0, 0};
  for (long i = 0; i < n_random; ++i) {
    uint8_t p[10];
    for (int k = 0; k < 10; k += 8) {
      x += 0x9E3779B97F4A7C15ull;
      uint64_t z = x;
      z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
      z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
      z ^= z >> 31;
      for (int b = 0; b < 8 && k + b < 10; ++b) p[k + b] = (uint8_t)(z >> (8 * b));
    }
    // half of the payloads get a type the unpacker decodes, so those paths see most of the work
    if (i & 1) p[9] = (uint8_t)((p[9] & 0xC7) | ((i >> 1) % 3 == 0 ? 0x08 : (i >> 1) % 3 == 1 ? 0x20 : 0x00));
    ft8_text t;
    memset(&t, 0xA5, sizeof t);
    msg77::unpack(p, &t);
    if (!sane(t)) {
      printf("payload %02x%02x%02x%02x%02x%02x%02x%02x%02x%02x: record not sane (status %d, text \"%.28s\")\n", p[0],
             p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], t.status, t.text);
      if (++bad > 20) break;
    } else {
      ++by_status[t.status];
    }
  }
  printf("msg77_check: %d vectors, %ld random payloads (status 0/1/2: %ld/%ld/%ld), %d failures\n",
         (int)(sizeof kVectors / sizeof kVectors[0]), n_random, by_status[0], by_status[1], by_status[2], bad);
  return bad ? 1 : 0;
}
