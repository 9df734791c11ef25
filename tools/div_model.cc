// div_model.cc -- host model of k_bp's shared-reciprocal division (csrc/div_shared.h).
//
//   div_model K LOG2_EPS0 N_DIVISIONS [SEED]   ->  prints "K=.. eps0=2^-.. divisions=.. mismatches=.."
//                                                   exit status 1 when any quotient differs
//
// The hardware seed is modelled as (1 / Q) (1 + d), d uniform in +-eps0 (v_rcp_f64: about 2^-23).
// Numerators and denominators come from the kernel's own polynomials (bp.hip tanh_group /
// atanh_group, folded forms): fast_tanh over |y| <= 9.94, fast_atanh over |x| <= 1.0073, a share of
// the arguments scaled down as far as the kernel's short path admits them (2^-100, 2^-600), and a
// share of the denominators with an all-ones or a 1.0...01 significand (the hardest roundings).
// Every quotient is compared bit for bit with the host's x / y.
// Build with -ffp-contract=off (as the kernel is).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../ft8_demodulator_amd/csrc/div_shared.h"

namespace {

struct Rng {  // splitmix64
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
  }
  double unit() { return (double)(next() >> 11) * 0x1p-53; }        // [0, 1)
  double sym() { return 2.0 * unit() - 1.0; }                        // [-1, 1)
};

struct SeedModel {
  Rng* rng;
  double eps0;
  double operator()(double v) const { return (1.0 / v) * (1.0 + eps0 * rng->sym()); }
};

uint64_t bits_of(double v) {
  uint64_t b;
  std::memcpy(&b, &v, 8);
  return b;
}

double with_significand(double v, uint64_t frac) {
  uint64_t b = (bits_of(v) & 0xfff0000000000000ull) | frac;
  std::memcpy(&v, &b, 8);
  return v;
}

// an argument of magnitude <= bound; one in eight scaled down by up to 2^-max_down
double argument(Rng& r, double bound, int max_down) {
  double v = bound * r.sym();
  if ((r.next() & 7) == 0) v = std::ldexp(v, -(int)(r.next() % (uint64_t)(max_down + 1)));
  return v;
}

// one in eight denominators: significand all ones, or 1.0...01
double hard_denominator(Rng& r, double nb) {
  const uint64_t c = r.next() & 15;
  if (c == 0) return with_significand(nb, 0x000fffffffffffffull);
  if (c == 1) return with_significand(nb, 1ull);
  return nb;
}

void tanh_pair(Rng& r, double& na, double& nb) {  // bp.hip tanh_group, short path
  const double yv = argument(r, 9.94, 100), z = yv * yv;
  na = yv * (15120.0 + z * (420.0 + z));
  nb = hard_denominator(r, -30240.0 + z * (-3360.0 + z * -30.0));
}

void atanh_pair(Rng& r, double& na, double& nb) {  // bp.hip atanh_group
  const double xv = argument(r, 1.0073, 600), x2 = xv * xv;
  na = xv * (945.0 + x2 * __builtin_fma(x2, 64.0, -735.0));
  nb = hard_denominator(r, -472.5 + x2 * (525.0 + x2 * -112.5));
}

template <int K>
long run(long groups, double eps0, uint64_t seed) {
  Rng gen{seed}, noise{seed ^ 0x5851f42d4c957f2dull};
  SeedModel rcp{&noise, eps0};
  long bad = 0;
  for (long g = 0; g < groups; ++g) {
    double x[K], y[K], q[K];
    const bool th = (g & 1) == 0;  // a group is one phase's divisions: all tanh or all atanh
    for (int i = 0; i < K; ++i) th ? tanh_pair(gen, x[i], y[i]) : atanh_pair(gen, x[i], y[i]);
    ft8::div_shared<K>(q, x, y, rcp);
    for (int i = 0; i < K; ++i) {
      const double want = x[i] / y[i];
      if (bits_of(q[i]) != bits_of(want)) {
        if (bad < 10) std::printf("mismatch: %a / %a = %a, got %a\n", x[i], y[i], want, q[i]);
        ++bad;
      }
    }
  }
  return bad;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 4) {
    std::fprintf(stderr, "usage: div_model K LOG2_EPS0 N_DIVISIONS [SEED]\n");
    return 2;
  }
  const int K = std::atoi(argv[1]), l2 = std::atoi(argv[2]);
  const long n = std::atol(argv[3]);
  const uint64_t seed = argc > 4 ? std::strtoull(argv[4], nullptr, 10) : 1;
  if ((K != 3 && K != 9) || l2 > -1 || l2 < -52 || n <= 0) {
    std::fprintf(stderr, "K is 3 or 9, LOG2_EPS0 in [-52, -1], N_DIVISIONS > 0\n");
    return 2;
  }
  const long groups = (n + K - 1) / K;
  const double eps0 = std::ldexp(1.0, l2);
  const long bad = K == 3 ? run<3>(groups, eps0, seed) : run<9>(groups, eps0, seed);
  std::printf("K=%d eps0=2^%d divisions=%ld mismatches=%ld\n", K, l2, groups * K, bad);
  return bad ? 1 : 0;
}
