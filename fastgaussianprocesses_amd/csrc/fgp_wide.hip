// Wide inputs: the d-dependent kernels for 9 <= d <= FGP_WIDE_MAX_D (64) dimensions, beside the d <= FGP_MAX_D ones
// (whose per-thread register arrays and by-value arguments are sized by FGP_MAX_D and stay as they are).
//
//   points / parts   fgp_wide_lattice_points, fgp_wide_lattice_parts, fgp_wide_net_parts: the narrow kernels'
//                    arithmetic (fgp_nll.hip) with per-dimension tables of 64 entries
//   first column     k_wide_k1:      k1[g, i] = s_g prod_j (1 + l_gj parts[j, i])  (abstract_fast_gp.py:181-191)
//                    k_wide_k1_bwd:  its adjoint for the natural scale / lengthscale rows (what autograd's prod
//                                    backward computes from a [G, d, n] temporary), leave-one-out products from
//                                    prefix / suffix products (a factor may be zero or negative)
//   prediction       k_wide_rows (kernel rows, abstract_gp.py:407-411,452-457) and k_wide_post_mean (matrix-free
//                    posterior mean, abstract_gp.py:352-380) with the factor arithmetic of fgp_factors.h
//
// No per-thread array is indexed by a run-time dimension: dimensions run in blocks of 8 (k1), in a padded
// compile-time count (k1 backward; a padded dimension has lengthscale 0 and part 0: its factor is exactly 1, the
// convention of fgp_nll.h) or one at a time with the per-dimension constants in LDS / kernel arguments (uniform
// reads).  Every reduction is fixed-order (wave tree, per-block partials, one workgroup per output): no atomics,
// no inter-workgroup hand-off.
#include <algorithm>
#include <cmath>
#include <type_traits>

#include "fgp_common.h"
#include "fgp_factors.h"
#include "fgp_runtime.h"
#include "fgp_wide.h"
#include "../../include/fgp_hip.h"

namespace fgp {

constexpr int kWPmB = 4;              // outputs per post_mean kernel evaluation (as fgp_post_mean)
constexpr int kWSlab = 64;            // training points per LDS slab of k_wide_post_mean (64 dims x 64 points = 32 KB)
constexpr int kWIB = 8;               // training points whose products a thread holds at once
constexpr int kWRowsG = 4;            // hyper-parameter rows per k_wide_k1 / k_wide_rows workgroup

struct WideGen {
  unsigned z[kWD];   // z_j mod 2^bits
};

// ------------------------------------------------------------------------------------------------
// points and parts (the arithmetic of k_lattice_points / k_lattice_parts / k_net_parts, fgp_nll.hip)
__global__ __launch_bounds__(kWG) void k_wide_lattice_points(WideGen g, const double* __restrict__ shift, int64_t n0,
                                                             int64_t n1, int d, int bits, double* __restrict__ x) {
  const int64_t i = n0 + (int64_t)blockIdx.x * kWG + threadIdx.x;
  if (i >= n1) return;
  const unsigned br = brev_bits((unsigned)i, bits), mask = bits >= 32 ? 0xffffffffu : (1u << bits) - 1u;
  const double inv = ldexp(1.0, -bits);
  for (int j = 0; j < d; ++j) {
    double v = (double)((br * g.z[j]) & mask) * inv;
    v = v + shift[j];
    if (v >= 1.0) v -= 1.0;
    x[(i - n0) * d + j] = v;
  }
}

__global__ __launch_bounds__(kWG) void k_wide_lattice_parts(const double* __restrict__ x, int64_t xs,
                                                            const double* __restrict__ z, int64_t n, int d,
                                                            WideSpec spec, double* __restrict__ parts) {
  const int64_t i = (int64_t)blockIdx.x * kWG + threadIdx.x;
  if (i >= n) return;
  for (int j = 0; j < d; ++j) {
    const double delta = mod1(x[i * xs + j] - z[j]);
    parts[(int64_t)j * n + i] = spec.coef[j] * bernoulli(spec.order[j], delta);
  }
}

__global__ __launch_bounds__(kWG) void k_wide_net_parts(const int64_t* __restrict__ xb, int64_t xs,
                                                        const int64_t* __restrict__ z, int64_t n, int d, int t,
                                                        WideSpec spec, double* __restrict__ parts) {
  const int64_t i = (int64_t)blockIdx.x * kWG + threadIdx.x;
  if (i >= n) return;
  for (int j = 0; j < d; ++j) {
    const unsigned long long delta = (unsigned long long)(xb[i * xs + j] ^ z[j]);
    parts[(int64_t)j * n + i] = spec.order[j] == 1 ? walsh1(delta, t) : walsh_omega(spec.order[j], delta, t);
  }
}

// ------------------------------------------------------------------------------------------------
// first column, forward: thread = point i, NG hyper-parameter rows per workgroup (blockIdx.y), the lengthscale rows
// in LDS (broadcast reads), the dimensions in blocks of 8 loads.  Product in ascending j, then the scale (k1_from,
// fgp_nll.h).
template <int NG>
__global__ __launch_bounds__(kWG) void k_wide_k1(const double* __restrict__ parts, int64_t n, int d,
                                                 const double* __restrict__ scale, const double* __restrict__ ls, int G,
                                                 double* __restrict__ k1) {
  __shared__ double ls_s[NG][kWD];
  const int tid = threadIdx.x;
  const int g0 = blockIdx.y * NG;
  for (int e = tid; e < NG * kWD; e += kWG) {
    const int b = e / kWD, j = e % kWD;
    const int g = g0 + b < G ? g0 + b : G - 1;
    ls_s[b][j] = j < d ? ls[(int64_t)g * d + j] : 0.0;
  }
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * kWG + tid;
  if (i >= n) return;
  double p[NG];
#pragma unroll
  for (int b = 0; b < NG; ++b) p[b] = 1.0;
  for (int j0 = 0; j0 < d; j0 += 8) {
    double pv[8];
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) pv[jj] = j0 + jj < d ? parts[(int64_t)(j0 + jj) * n + i] : 0.0;
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) {
#pragma unroll
      for (int b = 0; b < NG; ++b) p[b] *= __builtin_fma(ls_s[b][j0 + jj], pv[jj], 1.0);
    }
  }
#pragma unroll
  for (int b = 0; b < NG; ++b)
    if (g0 + b < G) k1[(int64_t)(g0 + b) * n + i] = scale[g0 + b] * p[b];
}

// first column, backward: workgroup = (256 points, row g), thread = point; the point's d parts in registers (DB
// blocks of 8, padded), one pass over them.  With f_j = 1 + l_j p_j, per point
//   q = 0:      u prod_j f_j
//   q = 1 + j:  (u s p_j) prod_{j' != j} f_j'
// the leave-one-out product = (blocks before) (prefix within the block) (suffix within the block) (blocks after).
// Each quantity is summed over the workgroup as it is formed (wave tree, then the 4 waves in order) into
// partial[g][q][blk]; k_wide_k1_bwd_sum reduces over blk.
__device__ __forceinline__ void wide_wave_sum_to(double v, double* red_q) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) red_q[threadIdx.x >> 6] = v;
}

template <int DB>
__global__ __launch_bounds__(kWG) void k_wide_k1_bwd(const double* __restrict__ parts, int64_t n, int d,
                                                     const double* __restrict__ scale, const double* __restrict__ ls,
                                                     const double* __restrict__ u, int64_t nblk,
                                                     double* __restrict__ partial) {
  constexpr int DP = 8 * DB;
  __shared__ double ls_s[DP];
  __shared__ double red[DP + 1][kWG / 64];
  const int tid = threadIdx.x;
  const int g = blockIdx.y;
  if (tid < DP) ls_s[tid] = tid < d ? ls[(int64_t)g * d + tid] : 0.0;
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * kWG + tid;
  const bool live = i < n;
  const int64_t il = live ? i : 0;
  double pv[DP];
#pragma unroll
  for (int j = 0; j < DP; ++j) pv[j] = j < d ? parts[(int64_t)j * n + il] : 0.0;
  const double ui = live ? u[(int64_t)g * n + i] : 0.0;      // (a point past n contributes u = 0)
  double sufB[DB + 1];
  sufB[DB] = 1.0;
#pragma unroll
  for (int b = DB - 1; b >= 0; --b) {
    double bp = 1.0;
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) bp *= __builtin_fma(ls_s[8 * b + jj], pv[8 * b + jj], 1.0);
    sufB[b] = sufB[b + 1] * bp;
  }
  wide_wave_sum_to(ui * sufB[0], red[0]);
  const double us = ui * scale[g];
  double pre = 1.0;
#pragma unroll
  for (int b = 0; b < DB; ++b) {
    double f[8], suf[9];
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) f[jj] = __builtin_fma(ls_s[8 * b + jj], pv[8 * b + jj], 1.0);
    suf[8] = sufB[b + 1];
#pragma unroll
    for (int jj = 7; jj >= 0; --jj) suf[jj] = suf[jj + 1] * f[jj];
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) {
      wide_wave_sum_to((us * pv[8 * b + jj]) * (pre * suf[jj + 1]), red[1 + 8 * b + jj]);
      pre *= f[jj];
    }
  }
  __syncthreads();
  if (tid <= d) {
    double tot = red[tid][0];
#pragma unroll
    for (int w = 1; w < kWG / 64; ++w) tot += red[tid][w];
    partial[((int64_t)g * (1 + d) + tid) * nblk + blockIdx.x] = tot;
  }
}

// out[(e / N) * out_stride + e % N] = sum_c partial[e, c]: one workgroup per output element, fixed reduction tree
// (k_sum_chunks of fgp_predict.hip)
__global__ __launch_bounds__(kWG) void k_wide_sum(const double* __restrict__ partial, int64_t nchunks,
                                                  double* __restrict__ out, int64_t out_stride, int64_t N) {
  __shared__ double red[kWG / 64];
  const int64_t e = blockIdx.x;
  double s = 0.0;
  for (int64_t c = threadIdx.x; c < nchunks; c += kWG) s += partial[e * nchunks + c];
  s = block_sum(s, red);
  if (threadIdx.x == 0) out[(e / N) * out_stride + e % N] = s;
}

// the sums of k_wide_k1_bwd's partials: element (g, 0) -> dscale[g], (g, 1 + j) -> dls[g, j]
__global__ __launch_bounds__(kWG) void k_wide_k1_bwd_sum(const double* __restrict__ partial, int64_t nblk, int d,
                                                         double* __restrict__ dscale, double* __restrict__ dls) {
  __shared__ double red[kWG / 64];
  const int64_t e = blockIdx.x;
  double s = 0.0;
  for (int64_t c = threadIdx.x; c < nblk; c += kWG) s += partial[e * nblk + c];
  s = block_sum(s, red);
  if (threadIdx.x == 0) {
    const int64_t g = e / (1 + d);
    const int q = (int)(e % (1 + d));
    if (q == 0) dscale[g] = s;
    else dls[g * d + q - 1] = s;
  }
}

// ------------------------------------------------------------------------------------------------
// kernel rows: thread = training point i, workgroup = (256 points, test point t, NG rows); the test point and the
// per-(row, dimension) factor constants in LDS.  Same factor arithmetic as k_kernel_rows.
template <int FAM, int NG>
__global__ __launch_bounds__(kWG) void k_wide_rows(const double* __restrict__ xt, int64_t N, const void* __restrict__ z,
                                                   int64_t n, int d, WideSpec spec, int tbits,
                                                   const double* __restrict__ hyp, int Gk, double* __restrict__ rows) {
  __shared__ double xs[kWD];
  __shared__ double fa_s[NG][kWD], fc_s[NG][kWD];
  const int tid = threadIdx.x;
  const int64_t t = blockIdx.y;
  const int g0 = blockIdx.z * NG;
  if (tid < d) {
    const int j = tid;
    const double v = xt[t * d + j];
    if constexpr (FAM == 0) xs[j] = v;
    else xs[j] = __longlong_as_double((long long)to_bits(v, tbits));
#pragma unroll
    for (int b = 0; b < NG; ++b) {
      const int g = g0 + b < Gk ? g0 + b : Gk - 1;
      const double l = hyp[(int64_t)g * (1 + d) + 1 + j];
      if constexpr (FAM == 0) {
        const double a = l * spec.coef[j];
        fa_s[b][j] = a;
        fc_s[b][j] = fac_const(spec.order[j], a);
      } else {
        fa_s[b][j] = net_fa(spec.order[j], l);
        fc_s[b][j] = 3.0 * l;
      }
    }
  }
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * kWG + tid;
  if (i >= n) return;
  double p[NG];
#pragma unroll
  for (int b = 0; b < NG; ++b) p[b] = 1.0;
  for (int j = 0; j < d; ++j) {
    const int ord = spec.order[j];
    if constexpr (FAM == 0) {
      const double tj = fabs(xs[j] - static_cast<const double*>(z)[(int64_t)j * n + i]);
#pragma unroll
      for (int b = 0; b < NG; ++b) p[b] *= lat_factor(ord, tj, fa_s[b][j], fc_s[b][j]);
    } else {
      const unsigned long long dv = (unsigned long long)__double_as_longlong(xs[j]) ^
                                    (unsigned long long)static_cast<const long long*>(z)[(int64_t)j * n + i];
#pragma unroll
      for (int b = 0; b < NG; ++b) p[b] *= net_factor_o(ord, dv, tbits, fa_s[b][j], fc_s[b][j]);
    }
  }
#pragma unroll
  for (int b = 0; b < NG; ++b)
    if (g0 + b < Gk) rows[((int64_t)(g0 + b) * N + t) * n + i] = hyp[(int64_t)(g0 + b) * (1 + d)] * p[b];
}

// ------------------------------------------------------------------------------------------------
// posterior mean.  Test points dimension-major (xT[j][t]; nets: already as t-bit integers) so that a wave's load
// of one coordinate is contiguous.
template <int FAM>
__global__ __launch_bounds__(kWG) void k_wide_xt(const double* __restrict__ xt, int64_t N, int d, int tbits,
                                                 double* __restrict__ xT) {
  const int64_t e = (int64_t)blockIdx.x * kWG + threadIdx.x;
  if (e >= N * d) return;
  const int64_t t = e / d;
  const int j = (int)(e % d);
  const double v = xt[e];
  if constexpr (FAM == 0) xT[(int64_t)j * N + t] = v;
  else xT[(int64_t)j * N + t] = __longlong_as_double((long long)to_bits(v, tbits));
}

// pmean partials: thread = test point, workgroup = (chunk training points, 256 test points, problem) as k_post_mean.
// The training points of a slab (all d coordinates) and its coefficients in LDS; a thread holds the running
// products of kWIB training points x NB outputs and walks the dimensions once per such tile: the factor constants
// of dimension j (LDS, broadcast) and the thread's own coordinate j (one coalesced load, fetched one dimension ahead)
// serve kWIB x NB factors.  ORD = 4: every dimension of Bernoulli order 4 (alpha = 2), folded as in k_post_mean
// when every a = l c != 0:  1 + a B4(t) = a (u^2 + c'), c' = (1 - a/30) / a, prod_j a_j moved into the output scale.
template <int FAM, int NB, int ORD>
__global__ __launch_bounds__(kWG) void k_wide_post_mean(const double* __restrict__ xT, int64_t N,
                                                        const void* __restrict__ z, int64_t n, int d, WideSpec spec,
                                                        int tbits, const double* __restrict__ hyp, int Gk,
                                                        const double* __restrict__ coeffs, int64_t coeff_stride, int B,
                                                        double* __restrict__ partial, int64_t nchunks, int64_t hyp_ps,
                                                        int64_t coeff_ps, int64_t chunk) {
  __shared__ double zs[kWD][kWSlab];
  __shared__ double cs[NB][kWSlab];
  __shared__ double fa_s[NB][kWD], fc_s[NB][kWD];
  const int tid = threadIdx.x;
  const int64_t t = (int64_t)blockIdx.y * kWG + tid;
  const bool live = t < N;
  const int64_t tl = live ? t : 0;
  const int64_t p = blockIdx.z;      // block of outputs with their own hyper-parameters (fgp_wide_post_mean, B > 4)
  hyp += p * hyp_ps;
  coeffs += p * coeff_ps;
  partial += p * (int64_t)B * N * nchunks;
  int nz = 1;
  if (tid < d) {
    const int j = tid;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const int g = (b < B ? b : 0) % Gk;
      const double l = hyp[(int64_t)g * (1 + d) + 1 + j];
      if constexpr (FAM == 0) {
        const int ord = ORD ? ORD : spec.order[j];
        const double a = l * spec.coef[j];
        fa_s[b][j] = a;
        fc_s[b][j] = fac_const(ord, a);
        nz = nz && a != 0.0;
      } else {
        fa_s[b][j] = net_fa(spec.order[j], l);
        fc_s[b][j] = 3.0 * l;
      }
    }
  }
  bool fold = false;
  if constexpr (FAM == 0 && ORD == 4) {
    fold = __syncthreads_and(nz) != 0;
    if (fold) {
      if (tid < d) {
#pragma unroll
        for (int b = 0; b < NB; ++b) fc_s[b][tid] = fc_s[b][tid] / fa_s[b][tid];
      }
      __syncthreads();
    }
  } else {
    __syncthreads();
  }
  double sc[NB], acc[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    sc[b] = hyp[(int64_t)((b < B ? b : 0) % Gk) * (1 + d)];
    acc[b] = 0.0;
  }
  const int64_t i0 = (int64_t)blockIdx.x * chunk;
  const int64_t i1 = i0 + chunk < n ? i0 + chunk : n;
  auto slabs = [&](auto fold_c) {
    constexpr bool FOLD = decltype(fold_c)::value;
    for (int64_t s0 = i0; s0 < i1; s0 += kWSlab) {
      const int cnt = (int)((i1 - s0) < kWSlab ? (i1 - s0) : kWSlab);
      __syncthreads();
      // (points past cnt: coordinate 0 and coefficient 0 -- a finite product times 0)
      for (int e = tid; e < d * kWSlab; e += kWG) {
        const int j = e / kWSlab, ii = e % kWSlab;
        double v = 0.0;
        if (ii < cnt) {
          if constexpr (FAM == 0) v = static_cast<const double*>(z)[(int64_t)j * n + s0 + ii];
          else v = __longlong_as_double(static_cast<const long long*>(z)[(int64_t)j * n + s0 + ii]);
        }
        zs[j][ii] = v;
      }
      if (tid < NB * kWSlab) {
        const int b = tid / kWSlab, ii = tid % kWSlab;
        cs[b][ii] = (b < B && ii < cnt) ? coeffs[(int64_t)b * coeff_stride + s0 + ii] : 0.0;
      }
      __syncthreads();
      for (int it = 0; it < cnt; it += kWIB) {
        double pr[kWIB][NB];
#pragma unroll
        for (int ii = 0; ii < kWIB; ++ii) {
#pragma unroll
          for (int b = 0; b < NB; ++b) pr[ii][b] = 1.0;
        }
        double xn = xT[tl];
        for (int j = 0; j < d; ++j) {
          const double xv = xn;
          if (j + 1 < d) xn = xT[(int64_t)(j + 1) * N + tl];
          double fa[NB], fc[NB];
#pragma unroll
          for (int b = 0; b < NB; ++b) {
            fa[b] = fa_s[b][j];
            fc[b] = fc_s[b][j];
          }
          const int ord = ORD ? ORD : spec.order[j];
#pragma unroll
          for (int ii = 0; ii < kWIB; ++ii) {
            if constexpr (FAM == 0) {
              const double tj = fabs(xv - zs[j][it + ii]);
              if constexpr (FOLD) {
                const double u = fma(tj, tj, -tj);
#pragma unroll
                for (int b = 0; b < NB; ++b) pr[ii][b] *= fma(u, u, fc[b]);
              } else {
#pragma unroll
                for (int b = 0; b < NB; ++b) pr[ii][b] *= lat_factor(ord, tj, fa[b], fc[b]);
              }
            } else {
              const unsigned long long delta = (unsigned long long)__double_as_longlong(xv) ^
                                               (unsigned long long)__double_as_longlong(zs[j][it + ii]);
#pragma unroll
              for (int b = 0; b < NB; ++b) pr[ii][b] *= net_factor_o(ord, delta, tbits, fa[b], fc[b]);
            }
          }
        }
#pragma unroll
        for (int ii = 0; ii < kWIB; ++ii) {
#pragma unroll
          for (int b = 0; b < NB; ++b) acc[b] = fma(pr[ii][b], cs[b][it + ii], acc[b]);
        }
      }
    }
  };
  if (FAM == 0 && ORD == 4 && fold) {
    slabs(std::integral_constant<bool, FAM == 0 && ORD == 4>{});
    for (int j = 0; j < d; ++j) {
#pragma unroll
      for (int b = 0; b < NB; ++b) sc[b] *= fa_s[b][j];
    }
  } else {
    slabs(std::integral_constant<bool, false>{});
  }
  if (live) {
#pragma unroll
    for (int b = 0; b < NB; ++b)
      if (b < B) partial[((int64_t)b * N + t) * nchunks + blockIdx.x] = sc[b] * acc[b];
  }
}

// ------------------------------------------------------------------------------------------------ host side
// (kWD, WideSpec, wide_d_ok and wide_spec: fgp_wide.h)
template <int FAM>
static int wide_post_mean_launch(const double* xT, int64_t N, const void* z, int64_t n, int d, const WideSpec& spec,
                                 int tbits, const double* hyp, int Gk, const double* coeffs, int64_t cstride, int B,
                                 double* out, int64_t out_stride, double* work, int64_t chunk, int P, int64_t hyp_ps,
                                 int64_t coeff_ps, hipStream_t st) {
  const int64_t nchunks = (n + chunk - 1) / chunk;
  const dim3 grid((unsigned)nchunks, (unsigned)((N + kWG - 1) / kWG), (unsigned)P);
  bool uniform4 = FAM == 0;
  for (int j = 0; j < d; ++j) uniform4 = uniform4 && spec.order[j] == 4;
#define FGP_W(NBB, ORDD)                                                                                         \
  k_wide_post_mean<FAM, NBB, ORDD><<<grid, kWG, 0, st>>>(xT, N, z, n, d, spec, tbits, hyp, Gk, coeffs, cstride, B, \
                                                          work, nchunks, hyp_ps, coeff_ps, chunk)
  constexpr int O4 = FAM == 0 ? 4 : 0;   // (nets: no uniform-order instance)
  if (B == 1) {
    if (uniform4) FGP_W(1, O4);
    else FGP_W(1, 0);
  } else {
    if (uniform4) FGP_W(kWPmB, O4);
    else FGP_W(kWPmB, 0);
  }
#undef FGP_W
  int rc = check_launch("k_wide_post_mean");
  if (rc != kOk) return rc;
  k_wide_sum<<<(unsigned)((int64_t)P * B * N), kWG, 0, st>>>(work, nchunks, out, out_stride, N);
  return check_launch("k_wide_sum");
}

// fgp_post_mean's calling convention on dimension-major test points: B <= 4 outputs (g = b mod Gk), or any B with
// Gk == B as blocks of 4 outputs in one launch plus the remaining outputs in a second
template <int FAM>
static int wide_post_mean(const double* xT, int64_t N, const void* z, int64_t n, int d, const WideSpec& spec, int tbits,
                          const double* hyp, int Gk, const double* coeffs, int64_t cstride, int B, double* out,
                          int64_t out_stride, double* work, int64_t chunk, hipStream_t st) {
  if (B > kWPmB) {
    const int nblk = B / kWPmB, rem = B - nblk * kWPmB;
    int rc = wide_post_mean_launch<FAM>(xT, N, z, n, d, spec, tbits, hyp, kWPmB, coeffs, cstride, kWPmB, out, N, work,
                                        chunk, nblk, (int64_t)kWPmB * (1 + d), (int64_t)kWPmB * cstride, st);
    if (rc != kOk || rem == 0) return rc;
    const int b0 = nblk * kWPmB;
    return wide_post_mean_launch<FAM>(xT, N, z, n, d, spec, tbits, hyp + (int64_t)b0 * (1 + d), rem,
                                      coeffs + (int64_t)b0 * cstride, cstride, rem, out + (int64_t)b0 * N, N, work, chunk,
                                      1, 0, 0, st);
  }
  return wide_post_mean_launch<FAM>(xT, N, z, n, d, spec, tbits, hyp, Gk, coeffs, cstride, B, out, out_stride, work,
                                    chunk, 1, 0, 0, st);
}

}  // namespace fgp

using namespace fgp;

extern "C" {

int fgp_wide_lattice_points(const int64_t* z, const double* shift, int64_t n_min, int64_t n_max, int d, double* x,
                            void* stream) {
  int rc = wide_d_ok("fgp_wide_lattice_points", d);
  if (rc != kOk) return rc;
  if (n_min < 0 || n_max < n_min || n_max > ((int64_t)1 << 30))
    return set_error(kErrInvalid, "fgp_wide_lattice_points: bad n_min/n_max");
  if (!z || !shift || !x) return set_error(kErrInvalid, "fgp_wide_lattice_points: null pointer");
  if (n_max == n_min) return kOk;
  int bits = 0;
  while (((int64_t)1 << bits) < n_max) ++bits;
  WideGen g{};
  for (int j = 0; j < d; ++j) {
    if (z[j] <= 0 || z[j] >= ((int64_t)1 << (53 - bits)))
      return set_error(kErrUnsupported, "fgp_wide_lattice_points: z[%d] outside (0, 2^(53-bits))", j);
    g.z[j] = (unsigned)((uint64_t)z[j] & ((1ull << bits) - 1));
  }
  const int64_t cnt = n_max - n_min;
  k_wide_lattice_points<<<(unsigned)((cnt + kWG - 1) / kWG), kWG, 0, (hipStream_t)stream>>>(g, shift, n_min, n_max, d,
                                                                                            bits, x);
  return check_launch("k_wide_lattice_points");
}

int fgp_wide_lattice_parts(const double* x, int64_t x_row_stride, const double* z, int64_t n, int d, const int* order,
                           const double* coef, double* parts, void* stream) {
  int rc = wide_d_ok("fgp_wide_lattice_parts", d);
  if (rc != kOk) return rc;
  if (n < 0 || x_row_stride < 0) return set_error(kErrInvalid, "fgp_wide_lattice_parts: negative size");
  if (!x || !z || !parts || !order || !coef) return set_error(kErrInvalid, "fgp_wide_lattice_parts: null pointer");
  WideSpec spec;
  rc = wide_spec("fgp_wide_lattice_parts", FGP_FAMILY_LATTICE, d, order, coef, spec);
  if (rc != kOk) return rc;
  if (n == 0) return kOk;
  k_wide_lattice_parts<<<(unsigned)((n + kWG - 1) / kWG), kWG, 0, (hipStream_t)stream>>>(x, x_row_stride, z, n, d, spec,
                                                                                         parts);
  return check_launch("k_wide_lattice_parts");
}

int fgp_wide_net_parts(const int64_t* xb, int64_t xb_row_stride, const int64_t* z, int64_t n, int d, int t,
                       const int* order, double* parts, void* stream) {
  int rc = wide_d_ok("fgp_wide_net_parts", d);
  if (rc != kOk) return rc;
  if (n < 0 || xb_row_stride < 0 || t < 1 || t > 63) return set_error(kErrInvalid, "fgp_wide_net_parts: bad n/stride/t");
  if (!xb || !z || !parts) return set_error(kErrInvalid, "fgp_wide_net_parts: null pointer");
  WideSpec spec;
  rc = wide_spec("fgp_wide_net_parts", FGP_FAMILY_NET, d, order, nullptr, spec);
  if (rc != kOk) return rc;
  if (n == 0) return kOk;
  k_wide_net_parts<<<(unsigned)((n + kWG - 1) / kWG), kWG, 0, (hipStream_t)stream>>>(xb, xb_row_stride, z, n, d, t, spec,
                                                                                     parts);
  return check_launch("k_wide_net_parts");
}

int fgp_wide_k1(const double* parts, int64_t n, int d, const double* scale, const double* ls, int G, double* k1,
                void* stream) {
  int rc = wide_d_ok("fgp_wide_k1", d);
  if (rc != kOk) return rc;
  if (n < 0 || G < 1 || G > 65535 * kWRowsG) return set_error(kErrInvalid, "fgp_wide_k1: bad n=%lld / G=%d", (long long)n, G);
  if (!parts || !scale || !ls || !k1) return set_error(kErrInvalid, "fgp_wide_k1: null pointer");
  if (n == 0) return kOk;
  hipStream_t st = (hipStream_t)stream;
  const unsigned nb = (unsigned)((n + kWG - 1) / kWG);
  if (G == 1) k_wide_k1<1><<<dim3(nb, 1), kWG, 0, st>>>(parts, n, d, scale, ls, G, k1);
  else k_wide_k1<kWRowsG><<<dim3(nb, (unsigned)((G + kWRowsG - 1) / kWRowsG)), kWG, 0, st>>>(parts, n, d, scale, ls, G, k1);
  return check_launch("k_wide_k1");
}

int fgp_wide_k1_bwd_work(int64_t n, int d, int G, int64_t* len) {
  int rc = wide_d_ok("fgp_wide_k1_bwd_work", d);
  if (rc != kOk) return rc;
  if (n < 0 || G < 1) return set_error(kErrInvalid, "fgp_wide_k1_bwd_work: bad n=%lld / G=%d", (long long)n, G);
  if (!len) return set_error(kErrInvalid, "fgp_wide_k1_bwd_work: null pointer");
  *len = std::max<int64_t>(1, (int64_t)G * (1 + d) * ((n + kWG - 1) / kWG));
  return kOk;
}

int fgp_wide_k1_bwd(const double* parts, int64_t n, int d, const double* scale, const double* ls, int G, const double* u,
                    double* dscale, double* dls, double* work, void* stream) {
  int rc = wide_d_ok("fgp_wide_k1_bwd", d);
  if (rc != kOk) return rc;
  if (n < 1 || n > ((int64_t)1 << 31) || G < 1 || G > 65535)
    return set_error(kErrInvalid, "fgp_wide_k1_bwd: bad n=%lld / G=%d", (long long)n, G);
  if (!parts || !scale || !ls || !u || !dscale || !dls || !work)
    return set_error(kErrInvalid, "fgp_wide_k1_bwd: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const int64_t nblk = (n + kWG - 1) / kWG;
  const dim3 grid((unsigned)nblk, (unsigned)G);
  rc = dispatch_range<2, 8>((d + 7) / 8, [&](auto dbc) {
    k_wide_k1_bwd<decltype(dbc)::value><<<grid, kWG, 0, st>>>(parts, n, d, scale, ls, u, nblk, work);
    return check_launch("k_wide_k1_bwd");
  });
  if (rc != kOk) return rc == kNoMatch ? set_error(kErrInvalid, "fgp_wide_k1_bwd: d=%d", d) : rc;
  k_wide_k1_bwd_sum<<<(unsigned)((int64_t)G * (1 + d)), kWG, 0, st>>>(work, nblk, d, dscale, dls);
  return check_launch("k_wide_k1_bwd_sum");
}

int fgp_wide_kernel_rows(int family, const double* xt, int64_t N, const void* z, int64_t n, int d, int tbits,
                         const int* order, const double* coef, const double* hyp, int Gk, double* rows, void* stream) {
  int rc = wide_d_ok("fgp_wide_kernel_rows", d);
  if (rc != kOk) return rc;
  if (N < 0 || n < 1 || Gk < 1 || N > 65535 || Gk > 65535 * kWRowsG)
    return set_error(kErrInvalid, "fgp_wide_kernel_rows: bad sizes (N=%lld n=%lld Gk=%d)", (long long)N, (long long)n, Gk);
  if (!xt || !z || !hyp || !rows) return set_error(kErrInvalid, "fgp_wide_kernel_rows: null pointer");
  WideSpec spec;
  rc = wide_spec("fgp_wide_kernel_rows", family, d, order, coef, spec);
  if (rc != kOk) return rc;
  if (N == 0) return kOk;
  hipStream_t st = (hipStream_t)stream;
  const unsigned nb = (unsigned)((n + kWG - 1) / kWG);
  const bool lat = family == FGP_FAMILY_LATTICE;
  if (Gk == 1) {
    const dim3 grid(nb, (unsigned)N, 1);
    if (lat) k_wide_rows<0, 1><<<grid, kWG, 0, st>>>(xt, N, z, n, d, spec, tbits, hyp, Gk, rows);
    else k_wide_rows<1, 1><<<grid, kWG, 0, st>>>(xt, N, z, n, d, spec, tbits, hyp, Gk, rows);
  } else {
    const dim3 grid(nb, (unsigned)N, (unsigned)((Gk + kWRowsG - 1) / kWRowsG));
    if (lat) k_wide_rows<0, kWRowsG><<<grid, kWG, 0, st>>>(xt, N, z, n, d, spec, tbits, hyp, Gk, rows);
    else k_wide_rows<1, kWRowsG><<<grid, kWG, 0, st>>>(xt, N, z, n, d, spec, tbits, hyp, Gk, rows);
  }
  return check_launch("k_wide_rows");
}

int fgp_wide_post_mean(int family, const double* xt, int64_t N, const void* z, int64_t n, int d, int tbits,
                       const int* order, const double* coef, const double* hyp, int Gk, const double* coeffs,
                       int64_t coeff_stride, int B, double* out, int64_t out_stride, double* work, int64_t chunk,
                       void* stream) {
  int rc = wide_d_ok("fgp_wide_post_mean", d);
  if (rc != kOk) return rc;
  if (N < 0 || n < 1 || B < 1 || Gk < 1 || chunk < 1 || coeff_stride < 0 || out_stride < 0 || (B > kWPmB && Gk != B) ||
      B / kWPmB > 65535 || (N + kWG - 1) / kWG > 65535)
    return set_error(kErrInvalid, "fgp_wide_post_mean: bad sizes (N=%lld n=%lld B=%d Gk=%d chunk=%lld)", (long long)N,
                     (long long)n, B, Gk, (long long)chunk);
  if (B > kWPmB && out_stride != N) return set_error(kErrInvalid, "fgp_wide_post_mean: B > %d needs out_stride == N", kWPmB);
  if (!xt || !z || !hyp || !coeffs || !out || !work) return set_error(kErrInvalid, "fgp_wide_post_mean: null pointer");
  WideSpec spec;
  rc = wide_spec("fgp_wide_post_mean", family, d, order, coef, spec);
  if (rc != kOk) return rc;
  if (N == 0) return kOk;
  hipStream_t st = (hipStream_t)stream;
  const int64_t nchunks = (n + chunk - 1) / chunk;
  double* xT = work + nchunks * B * N;
  const unsigned gx = (unsigned)((N * d + kWG - 1) / kWG);
  if (family == FGP_FAMILY_LATTICE) k_wide_xt<0><<<gx, kWG, 0, st>>>(xt, N, d, tbits, xT);
  else k_wide_xt<1><<<gx, kWG, 0, st>>>(xt, N, d, tbits, xT);
  rc = check_launch("k_wide_xt");
  if (rc != kOk) return rc;
  if (family == FGP_FAMILY_LATTICE)
    return wide_post_mean<0>(xT, N, z, n, d, spec, tbits, hyp, Gk, coeffs, coeff_stride, B, out, out_stride, work, chunk, st);
  return wide_post_mean<1>(xT, N, z, n, d, spec, tbits, hyp, Gk, coeffs, coeff_stride, B, out, out_stride, work, chunk, st);
}

}  // extern "C"
