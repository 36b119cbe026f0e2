// Per-factor device arithmetic of the cross-kernel K(x, z) = scale prod_j (1 + l_j part_j(x, z)), shared by the
// prediction kernels (fgp_predict.hip, d <= FGP_MAX_D) and the wide ones (fgp_wide.hip, d <= FGP_WIDE_MAX_D): one
// definition, so a factor has the same value in both.
#pragma once

#include "fgp_common.h"

namespace fgp {

// ------------------------------------------------------------------------------------------------
// Per-factor arithmetic.  Lattice: even Bernoulli polynomials are polynomials in u = t(t - 1), and
// B_{2a}((x - z) % 1) = B_{2a}(|x - z|) exactly for x, z in [0, 1] (B_{2a}(1 - t) = B_{2a}(t)), so
//   1 + l c B2 = fma(a, u, 1 + a/6)                 a = l c
//   1 + l c B4 = fma(a u, u, 1 - a/30)              (B4 = u^2 - 1/30)
//   1 + l c B6 = fma(a u^2, u - 1/2, 1 + a/42)      (B6 = u^2 (u - 1/2) + 1/42)
//   1 + l c B8 = fma(a u^2, u (u - 4/3) + 2/3, 1 - a/30)
// (identical to the reference's Horner evaluation up to rounding).  Net (order-1 Walsh):
//   1 + l walsh1(delta) = (1 + l) - 3 l 2^(floor(log2 delta) - t)   (= 1 + l when delta = 0)
__device__ __forceinline__ double fac_const(int order, double a) {
  switch (order) {
    case 2: return 1.0 + a * (1.0 / 6.0);
    case 6: return 1.0 + a * (1.0 / 42.0);
    default: return 1.0 - a * (1.0 / 30.0);   // 4, 8
  }
}

__device__ __forceinline__ double lat_factor(int order, double t, double a, double c) {
  const double u = fma(t, t, -t);
  switch (order) {
    case 2: return fma(a, u, c);
    case 4: return fma(a * u, u, c);
    case 6: return fma(a * u * u, u - 0.5, c);
    default: return fma(a * u * u, fma(u, u - 4.0 / 3.0, 2.0 / 3.0), c);
  }
}

__device__ __forceinline__ double net_factor(unsigned long long delta, int tbits, double c1, double c3) {
  if (delta == 0ull) return c1;
  const int fl = 63 - __clzll((long long)delta);
  return c1 - ldexp(c3, fl - tbits);
}

// Net factor of Walsh order ord: order 1 as above (fa = 1 + l, fc = 3 l); orders 2..4
// 1 + l omega_ord(delta) (fa = l; walsh_omega, fgp_common.h)
__device__ __forceinline__ double net_fa(int ord, double l) { return ord <= 1 ? 1.0 + l : l; }
__device__ __forceinline__ double net_factor_o(int ord, unsigned long long delta, int tbits, double fa, double fc) {
  if (ord <= 1) return net_factor(delta, tbits, fa, fc);
  return __builtin_fma(fa, walsh_omega(ord, delta, tbits), 1.0);
}

__device__ __forceinline__ unsigned long long to_bits(double v, int tbits) {
  double r = fmod(v, 1.0);
  if (r != 0.0 && r < 0.0) r += 1.0;                 // torch.remainder(v, 1)
  return (unsigned long long)(long long)floor(r * ldexp(1.0, tbits));
}

// One derivative part of the task-pair kernel (k_mt_parts' arithmetic): coef B_order(dl) for lattices (dl = (x - z)
// mod 1), coef (add + omega_order(dv)) for nets (dv = x XOR z as t-bit integers).  Shared by the wide (fgp_wide_mt.hip)
// and the d <= 8 (fgp_mt_pred.hip) kernels; wmt_base / wmt_finish are its two steps, for a kernel that fetches coef and
// add only after the polynomial.
__device__ __forceinline__ double wmt_base(int fam, int order, double dl, unsigned long long dv, int t) {
  if (fam == 0) return bernoulli_any(order, dl);
  return order == 1 ? walsh1(dv, t) : walsh_omega(order, dv, t);
}
__device__ __forceinline__ double wmt_finish(int fam, double coef, double add, double base) {
  return fam == 0 ? coef * base : coef * (add + base);
}
__device__ __forceinline__ double wmt_part(int fam, int order, double coef, double add, double dl,
                                           unsigned long long dv, int t) {
  return wmt_finish(fam, coef, add, wmt_base(fam, order, dl, dv, t));
}

}  // namespace fgp
