// div_shared.h -- K IEEE-754 double divisions on one hardware reciprocal (device and host).
//
// k_bp's short division (bp.hip div_fast) spends one v_rcp_f64 -- a quarter-rate instruction -- per
// quotient.  When every denominator of a group is a finite normal number far from 0 and from
// overflow, and so is the group's product, the K reciprocals follow from ONE reciprocal of the
// product by plain multiplies (simultaneous inversion):
//
//   pre[i] = y[0] y[1] .. y[i]                                    K-1 multiplies
//   r      = 1 / pre[K-1]          seed + two Newton steps, exactly as div_fast refines its seed
//   yi[i]  = r pre[i-1],  r = r y[i]   for i = K-1 .. 1;  yi[0] = r      2 (K-1) multiplies
//
// Each yi[i] then takes div_fast's last Newton step on its OWN denominator and div_fast's quotient
// tail unchanged, so nothing is dropped: every reciprocal has two Newton steps from the seed behind
// it (on the product) and one of its own.
//
// Exactness.  Let e0 be the seed's relative error (v_rcp_f64: about 2^-23; the host model in
// tools/div_model.cc also runs 2^-20).  After two Newton steps the product's reciprocal is within
// e0^4 + a few 2^-53 of exact.  A derived yi[i] is that value times at most K-1 rounded prefix
// factors and K-1 rounded back-multiplications of its own chain: at most about K + 3 roundings in
// all, i.e. <= 12 * 2^-53 < 2^-49.4 relative at K = 9.  The sequence the compiler emits for x / y
// holds e0^2 + 2^-53 (about 2^-46) at the same point, after ITS first Newton step -- a looser
// value.  Both then run the identical last Newton step (error^2 plus one rounding: within an ulp of
// 1/y) and the identical tail m = x yi, e = fma(-y, m, x), q = fma(e, yi, m), whose correct
// rounding needs only a reciprocal within an ulp and no underflow or overflow in x, m, e -- the
// conditions div_fast's callers already establish.  So q == RN(x / y) wherever div_fast's is.
//
// Preconditions (the caller's): every y[i] finite, normal, and the K-fold product neither
// overflows nor leaves the normal range with its reciprocal (k_bp: |product| in about
// [6e13, 2.4e52] at K = 9, see bp.hip); every x[i] as div_fast requires.  A NaN, infinity or zero
// in ONE denominator would spoil all K quotients: callers with such inputs keep the per-division
// sequence.
//
// rcp is a functor: __builtin_amdgcn_rcp on the device, a model of it on the host.  The code is
// written stage by stage over the group, like div_fast, so the dependent chains interleave.  It
// must be compiled with -ffp-contract=off: every fma below is explicit and every other product
// rounds on its own.
#pragma once

#if defined(__HIPCC__)
#define FT8_DIV_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define FT8_DIV_HD inline
#endif

namespace ft8 {

// A point the instruction scheduler does not move code across (device), nothing on the host
#if defined(__HIP_DEVICE_COMPILE__)
#define FT8_DIV_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
#else
#define FT8_DIV_SCHED_FENCE() ((void)0)
#endif

// q[i] = RN(x[i] / y[i]), i < K, on one reciprocal.  The per-division part (last Newton step and
// tail) runs C divisions at a time, stage by stage; C < K keeps the temporaries of the other
// chunks out of the register file (a scheduler free to interleave all K holds them all).
template <int K, int C = K, class Rcp>
FT8_DIV_HD void div_shared(double* q, const double* x, const double* y, Rcp rcp) {
  static_assert(K >= 2 && C >= 1 && K % C == 0, "one reciprocal for >= 2 divisions, in whole chunks");
  double pre[K], yi[K];
  // prefix products (pre[K-1]: the group's product)
  pre[0] = y[0];
#pragma unroll
  for (int i = 1; i < K; ++i) pre[i] = pre[i - 1] * y[i];
  // one seed, refined twice
  double r = rcp(pre[K - 1]);
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const double e = __builtin_fma(-pre[K - 1], r, 1.0);
    r = __builtin_fma(r, e, r);
  }
  // back-substitution: r = 1 / (y[0] .. y[i]) on entry to step i
#pragma unroll
  for (int i = K - 1; i >= 1; --i) {
    yi[i] = r * pre[i - 1];
    r = r * y[i];
  }
  yi[0] = r;
  // div_fast's last Newton step on each denominator, then its quotient tail
#pragma unroll
  for (int c = 0; c < K; c += C) {
    if (C < K) FT8_DIV_SCHED_FENCE();
    double e[C], m[C], t[C];
#pragma unroll
    for (int i = 0; i < C; ++i) e[i] = __builtin_fma(-y[c + i], yi[c + i], 1.0);
#pragma unroll
    for (int i = 0; i < C; ++i) t[i] = __builtin_fma(yi[c + i], e[i], yi[c + i]);
#pragma unroll
    for (int i = 0; i < C; ++i) m[i] = x[c + i] * t[i];
#pragma unroll
    for (int i = 0; i < C; ++i) e[i] = __builtin_fma(-y[c + i], m[i], x[c + i]);
#pragma unroll
    for (int i = 0; i < C; ++i) q[c + i] = __builtin_fma(e[i], t[i], m[i]);
  }
}

}  // namespace ft8
