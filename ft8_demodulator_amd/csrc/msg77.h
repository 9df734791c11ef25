// msg77.h -- the message layer of the FT8 protocol: a 77-bit payload -> text (ft8_text), and the
// callsign hashes.  Plain C++17 with no HIP type in its interface: hipcc compiles it for the
// device (k_unpack77, msg.hip) and for the host (ft8_unpack77_host), g++ compiles it alone
// (tools/msg77_check.cc).  This is the only implementation of the field arithmetic.
//
// Bit k (0..76) of a payload is (payload[k >> 3] >> (7 - (k & 7))) & 1; fields are big-endian runs
// of bits.  i3 = bits 74..76, n3 = bits 71..73 (meaningful when i3 == 0).  Layouts:
//   i3 = 1, 2   n28a ipa n28b ipb ir g15 i3               standard message
//   i3 = 4      h12 c58 iflip nrpt(2) icq i3              one non-standard callsign
//   i3 = 0      f71 n3 i3, n3 = 0 free text, n3 = 5 telemetry
// Every other type is recognised and left undecoded (status 1).
#pragma once
#include <stdint.h>

#include "../../include/ft8hip.h"

#if defined(__HIPCC__)
#define MSG77_HD __host__ __device__
#else
#define MSG77_HD
#endif

namespace msg77 {

constexpr uint32_t NTOKENS = 2063592u;
constexpr uint32_t MAX22 = 4194304u;
constexpr uint32_t MAXGRID4 = 32400u;
constexpr uint64_t ipow(uint64_t b, int e) { return e == 0 ? 1 : b * ipow(b, e - 1); }
constexpr uint64_t POW38_11 = ipow(38, 11);  // c58 values at or above it are invalid (38^11 < 2^58)

enum : uint8_t { ST_OK = 0, ST_UNDECODED = 1, ST_RANGE = 2, ST_NOT_OK = 3 };
constexpr int kTextMax = 27;  // characters text[] can hold before its NUL

// ---- alphabets (index -> character), as arithmetic so that host and device share them ----------
MSG77_HD inline char a1(uint32_t i) {  // " 0-9A-Z"
  return i == 0 ? ' ' : i < 11 ? (char)('0' + (i - 1)) : (char)('A' + (i - 11));
}
MSG77_HD inline char a2(uint32_t i) { return i < 10 ? (char)('0' + i) : (char)('A' + (i - 10)); }  // "0-9A-Z"
MSG77_HD inline char a3(uint32_t i) { return (char)('0' + i); }                                     // "0-9"
MSG77_HD inline char a4(uint32_t i) { return i == 0 ? ' ' : (char)('A' + (i - 1)); }               // " A-Z"
MSG77_HD inline char a38(uint32_t i) { return i < 37 ? a1(i) : '/'; }                              // " 0-9A-Z/"
MSG77_HD inline char a42(uint32_t i) {                                                             // " 0-9A-Z+-./?"
  if (i < 37) return a1(i);
  switch (i) {
    case 37: return '+';
    case 38: return '-';
    case 39: return '.';
    case 40: return '/';
    default: return '?';
  }
}
// character -> index in A38, -1 when outside it
MSG77_HD inline int idx38(char c) {
  if (c == ' ') return 0;
  if (c >= '0' && c <= '9') return 1 + (c - '0');
  if (c >= 'A' && c <= 'Z') return 11 + (c - 'A');
  if (c == '/') return 37;
  return -1;
}

// bits [start, start + len) of the payload as a big-endian number, len <= 64
MSG77_HD inline uint64_t field(const uint8_t* p, int start, int len) {
  uint64_t v = 0;
  for (int k = start; k < start + len; ++k) v = (v << 1) | (uint64_t)((p[k >> 3] >> (7 - (k & 7))) & 1);
  return v;
}

// ---- callsign hash -----------------------------------------------------------------------------
// n22 of the callsign left-justified in 11 characters: m = its base-38 value over A38,
// n22 = (47055833459 m mod 2^64) >> 42; n12 = n22 >> 10, n10 = n22 >> 12.  Returns 0, or -1 for a
// length above 11 or a character outside A38.
MSG77_HD inline int hash22(const char* call, int len, uint32_t* n22) {
  if (len < 0 || len > 11) return -1;
  uint64_t m = 0;
  for (int i = 0; i < 11; ++i) {
    const int j = idx38(i < len ? call[i] : ' ');
    if (j < 0) return -1;
    m = m * 38u + (uint64_t)j;
  }
  *n22 = (uint32_t)((47055833459ull * m) >> 42);
  return 0;
}

// ---- text assembly -----------------------------------------------------------------------------
struct Writer {
  char* t;
  int n;
  MSG77_HD void put(char c) {
    if (n < kTextMax) t[n++] = c;
  }
  MSG77_HD void put(const char* s, int len) {
    for (int i = 0; i < len; ++i) put(s[i]);
  }
  // a field after the ones before it: one space between non-empty fields
  MSG77_HD void sep() {
    if (n > 0) put(' ');
  }
};

// buf[0 .. len) without its leading and trailing spaces: the new start, *len updated
MSG77_HD inline const char* trim(const char* buf, int* len) {
  int a = 0, b = *len;
  while (a < b && buf[a] == ' ') ++a;
  while (b > a && buf[b - 1] == ' ') --b;
  *len = b - a;
  return buf + a;
}

enum CallKind { CALL_TOKEN = 0, CALL_HASH = 1, CALL_STD = 2 };

// n28 -> the call as text in buf (at most 11 characters, "<...>" for a hash).  Returns the length,
// or -1 when n28 is out of range or the call is empty.  *kind: CallKind; *h22: the hash value.
MSG77_HD inline int call28(uint32_t n28, char* buf, int* kind, uint32_t* h22) {
  *kind = CALL_TOKEN;
  *h22 = 0;
  if (n28 < 3) {
    const char* w = n28 == 0 ? "DE" : n28 == 1 ? "QRZ" : "CQ";
    const int len = n28 == 1 ? 3 : 2;
    for (int i = 0; i < len; ++i) buf[i] = w[i];
    return len;
  }
  if (n28 < 1003) {  // CQ nnn
    const uint32_t n = n28 - 3;
    buf[0] = 'C', buf[1] = 'Q', buf[2] = ' ';
    buf[3] = (char)('0' + n / 100), buf[4] = (char)('0' + n / 10 % 10), buf[5] = (char)('0' + n % 10);
    return 6;
  }
  if (n28 < 532444) {  // CQ + up to four letters
    uint32_t n = n28 - 1003;
    char c[4];
    for (int i = 3; i >= 0; --i) c[i] = a4(n % 27), n /= 27;
    int len = 4;
    const char* s = trim(c, &len);
    buf[0] = 'C', buf[1] = 'Q';
    if (len == 0) return 2;
    buf[2] = ' ';
    for (int i = 0; i < len; ++i) buf[3 + i] = s[i];
    return 3 + len;
  }
  if (n28 < NTOKENS) return -1;
  if (n28 < NTOKENS + MAX22) {
    *kind = CALL_HASH;
    *h22 = n28 - NTOKENS;
    const char* w = "<...>";
    for (int i = 0; i < 5; ++i) buf[i] = w[i];
    return 5;
  }
  *kind = CALL_STD;
  uint32_t n = n28 - NTOKENS - MAX22;
  char c[8];
  c[5] = a4(n % 27), n /= 27;
  c[4] = a4(n % 27), n /= 27;
  c[3] = a4(n % 27), n /= 27;
  c[2] = a3(n % 10), n /= 10;
  c[1] = a2(n % 36), n /= 36;
  c[0] = a1(n);  // n <= 36: 2^28 - 1 - NTOKENS - MAX22 < 37 * 36 * 10 * 27^3
  int len = 6;
  if (c[0] == '3' && c[1] == 'D' && c[2] == '0' && c[3] != ' ') {  // 3D0xyz -> 3DA0xyz
    c[6] = c[5], c[5] = c[4], c[4] = c[3], c[3] = '0', c[2] = 'A';
    len = 7;
  } else if (c[0] == 'Q' && c[1] >= 'A' && c[1] <= 'Z') {  // Qxnnnn -> 3Xxnnnn
    for (int i = 6; i >= 2; --i) c[i] = c[i - 1];
    c[0] = '3', c[1] = 'X';
    len = 7;
  }
  const char* s = trim(c, &len);
  if (len == 0) return -1;
  for (int i = 0; i < len; ++i) buf[i] = s[i];
  return len;
}

MSG77_HD inline void put_word(Writer& w, uint32_t k) {  // 1 RRR, 2 RR73, 3 73
  if (k == 1) w.sep(), w.put("RRR", 3);
  else if (k == 2) w.sep(), w.put("RR73", 4);
  else if (k == 3) w.sep(), w.put("73", 2);
}

// i3 = 1 / 2
MSG77_HD inline uint8_t unpack_std(const uint8_t* p, uint32_t i3, ft8_text* o) {
  const uint32_t n28a = (uint32_t)field(p, 0, 28), ipa = (uint32_t)field(p, 28, 1);
  const uint32_t n28b = (uint32_t)field(p, 29, 28), ipb = (uint32_t)field(p, 57, 1);
  const uint32_t ir = (uint32_t)field(p, 58, 1), g15 = (uint32_t)field(p, 59, 15);
  char ca[12], cb[12];
  int ka, kb;
  uint32_t ha, hb;
  const int la = call28(n28a, ca, &ka, &ha), lb = call28(n28b, cb, &kb, &hb);
  if (la < 0 || lb < 0) return ST_RANGE;
  if (g15 == MAXGRID4 || g15 > MAXGRID4 + 105) return ST_RANGE;
  Writer w{o->text, 0};
  int nh = 0;
  const char sfx = i3 == 1 ? 'R' : 'P';
  w.put(ca, la);
  if (ipa && ka != CALL_TOKEN) w.put('/'), w.put(sfx);
  if (ka == CALL_HASH) o->hash[nh] = ha, o->hash_bits[nh] = 22, ++nh;
  w.sep();
  w.put(cb, lb);
  if (ipb && kb != CALL_TOKEN) w.put('/'), w.put(sfx);
  if (kb == CALL_HASH) o->hash[nh] = hb, o->hash_bits[nh] = 22, ++nh;
  if (g15 < MAXGRID4) {
    uint32_t n = g15;
    char g[4];
    g[3] = (char)('0' + n % 10), n /= 10;
    g[2] = (char)('0' + n % 10), n /= 10;
    g[1] = (char)('A' + n % 18), n /= 18;
    g[0] = (char)('A' + n);
    w.sep();
    if (ir) w.put('R'), w.put(' ');
    w.put(g, 4);
  } else {
    const uint32_t irpt = g15 - MAXGRID4;
    if (irpt >= 2 && irpt <= 4) {
      put_word(w, irpt - 1);
    } else if (irpt >= 5) {
      int snr = (int)irpt - 35;
      if (snr > 50) snr -= 101;
      w.sep();
      if (ir) w.put('R');
      w.put(snr < 0 ? '-' : '+');
      const int a = snr < 0 ? -snr : snr;
      w.put((char)('0' + a / 10)), w.put((char)('0' + a % 10));
    }
  }
  if (kb == CALL_STD) {
    for (int i = 0; i < lb; ++i) o->learn_call[i] = cb[i];
    (void)hash22(cb, lb, &o->learn_hash22);
  }
  return ST_OK;
}

// i3 = 4
MSG77_HD inline uint8_t unpack_nonstd(const uint8_t* p, ft8_text* o) {
  const uint32_t h12 = (uint32_t)field(p, 0, 12);
  uint64_t n58 = field(p, 12, 58);
  const uint32_t iflip = (uint32_t)field(p, 70, 1), nrpt = (uint32_t)field(p, 71, 2), icq = (uint32_t)field(p, 73, 1);
  if (n58 >= POW38_11) return ST_RANGE;
  char c[11];
  for (int i = 10; i >= 0; --i) c[i] = a38((uint32_t)(n58 % 38u)), n58 /= 38u;
  int len = 11;
  const char* call = trim(c, &len);
  if (len == 0) return ST_RANGE;
  Writer w{o->text, 0};
  if (icq) {
    w.put("CQ", 2), w.sep(), w.put(call, len);
  } else {
    if (iflip) w.put(call, len), w.sep(), w.put("<...>", 5);
    else w.put("<...>", 5), w.sep(), w.put(call, len);
    o->hash[0] = h12, o->hash_bits[0] = 12;
    put_word(w, nrpt);
  }
  for (int i = 0; i < len; ++i) o->learn_call[i] = call[i];
  (void)hash22(call, len, &o->learn_hash22);
  return ST_OK;
}

// i3 = 0, n3 = 0 (free text) and n3 = 5 (telemetry): f71 as a 9-byte big-endian number
MSG77_HD inline uint8_t unpack_f71(const uint8_t* p, uint32_t n3, ft8_text* o) {
  uint8_t b[9];
  for (int i = 0; i < 9; ++i) b[i] = (uint8_t)((p[i] >> 1) | (i ? (p[i - 1] & 1) << 7 : 0));
  Writer w{o->text, 0};
  if (n3 == 5) {
    for (int i = 0; i < 9; ++i) {
      const uint32_t hi = b[i] >> 4, lo = b[i] & 15;
      w.put((char)(hi < 10 ? '0' + hi : 'A' + (hi - 10)));
      w.put((char)(lo < 10 ? '0' + lo : 'A' + (lo - 10)));
    }
    return ST_OK;
  }
  char c[13];
  for (int i = 12; i >= 0; --i) {  // long division of the 9 bytes by 42
    uint32_t rem = 0;
    for (int j = 0; j < 9; ++j) {
      rem = (rem << 8) | b[j];
      b[j] = (uint8_t)(rem / 42u);
      rem %= 42u;
    }
    c[i] = a42(rem);
  }
  for (int j = 0; j < 9; ++j)
    if (b[j]) return ST_RANGE;  // f71 >= 42^13
  int len = 13;
  const char* s = trim(c, &len);
  w.put(s, len);
  return ST_OK;
}

// payload (10 bytes, 77 bits used) -> *o, every byte of it written; dup_of = -1
MSG77_HD inline void unpack(const uint8_t* p, ft8_text* o) {
  *o = ft8_text{};
  o->dup_of = -1;
  const uint32_t i3 = (uint32_t)field(p, 74, 3), n3 = (uint32_t)field(p, 71, 3);
  uint8_t st = ST_UNDECODED;
  if (i3 == 1 || i3 == 2) st = unpack_std(p, i3, o);
  else if (i3 == 4) st = unpack_nonstd(p, o);
  else if (i3 == 0 && (n3 == 0 || n3 == 5)) st = unpack_f71(p, n3, o);
  if (st != ST_OK) {  // nothing of a field out of range stays behind
    *o = ft8_text{};
    o->dup_of = -1;
  }
  o->i3 = (uint8_t)i3;
  o->n3 = (uint8_t)(i3 == 0 ? n3 : 0);
  o->status = st;
}

// a record that was not unpacked (ok == 0, or past the slot's count)
MSG77_HD inline void not_ok(ft8_text* o) {
  *o = ft8_text{};
  o->dup_of = -1;
  o->status = ST_NOT_OK;
}

}  // namespace msg77
