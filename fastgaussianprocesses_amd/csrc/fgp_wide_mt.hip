// Wide inputs, multitask / derivative-informed kernels: the task-pair kernel of abstract_fast_gp.py:173-191 for
// 9 <= d <= FGP_WIDE_MAX_D (64) dimensions and 1 <= P <= FGP_WIDE_MT_MAX_P (16) derivative multi-index pairs,
//
//   K_ab(x, z) = scale sum_p cc[p] prod_j (ind[p][j] + l_j part[p][j](x, z)),
//   part = coef B_order((x_j - z_j) mod 1)  (lattice),  coef (add + omega_order(x_j XOR z_j))  (net),
//
// beside the d <= FGP_MAX_D kernel k_mt_parts (fgp_multitask.hip), whose arithmetic the parts here share
// (bernoulli_any, walsh1 / walsh_omega, fgp_common.h).
//
//   k_wmt_parts      parts[p][j][e], dimension-major (e: the (x_i, z_k) pairs or the zipped pairs)
//   k_wmt_k1         k1[g, i] = s_g sum_p cc[p] prod_j f_pj,  f_pj = ind[p][j] + l_gj parts[p][j][i]
//   k_wmt_k1_bwd     its adjoint for the natural scale / lengthscale rows; leave-one-out products from prefix / suffix
//                    products (a factor is exactly 0 where ind = 0 and l part = 0, and factors may be negative)
//   k_wmt_rows       rows[g][t][i] = K_ab(xt_t, z_i), the parts formed from the points; k_wmt_rows_zip the N values
//                    K_ab(xt_t, z_t)
//
// The conventions of fgp_wide.hip: no per-thread array indexed by a run-time dimension (dimensions in blocks of 8 or
// a padded compile-time count; a padded dimension has ind = 1, l = 0 and part = 0: its factor is exactly 1); the
// per-(p, j) constants come from LDS or kernel arguments with uniform reads; every reduction is fixed-order (wave
// tree, the 4 waves in order, per-block partials, one workgroup per output): no atomics, no inter-workgroup hand-off.
// The product runs in ascending j, the sum in ascending p, then the scale.
#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "fgp_common.h"
#include "fgp_factors.h"
#include "fgp_runtime.h"
#include "fgp_wide.h"
#include "../../include/fgp_hip.h"

namespace fgp {

constexpr int kMtP = FGP_WIDE_MT_MAX_P;   // derivative multi-index pairs of the fused kernels
constexpr int kMtRowsG = 4;               // hyper-parameter rows per k_wmt_k1 / k_wmt_rows workgroup

// what k1 and its adjoint need of the spec, by value: bit j of ind[p] = ind[p][j] (bits d .. 63 set: padded
// dimensions have the factor 1), cc[p]
struct MtInd {
  unsigned long long ind[kMtP];
  double cc[kMtP];
};

// the [P][64] tables of the parts, on the device (20 KB): code = order | ind << 8
struct MtTables {
  int code[kMtP * kWD];
  double coef[kMtP * kWD];
  double add[kMtP * kWD];
};

struct MtCc {
  double cc[kMtP];
};

// (wmt_part, one derivative part from the coordinate difference: fgp_factors.h)

// ------------------------------------------------------------------------------------------------ parts
// thread = pair e; the tables in LDS; parts[(p d + j) E + e]: a wave's store of one (p, j) is contiguous
__global__ __launch_bounds__(kWG) void k_wmt_parts(int family, const void* __restrict__ xv, int64_t xs, int64_t N,
                                                   const void* __restrict__ zv, int64_t zs, int64_t M, int zip, int d,
                                                   int P, const MtTables* __restrict__ tab, int t,
                                                   double* __restrict__ out) {
  __shared__ int code_s[kMtP * kWD];
  __shared__ double coef_s[kMtP * kWD], add_s[kMtP * kWD];
  for (int e = threadIdx.x; e < P * kWD; e += kWG) {
    code_s[e] = tab->code[e];
    coef_s[e] = tab->coef[e];
    add_s[e] = tab->add[e];
  }
  __syncthreads();
  const int64_t E = zip ? N : N * M;
  const int64_t e = (int64_t)blockIdx.x * kWG + threadIdx.x;
  if (e >= E) return;
  const int64_t i = zip ? e : e / M, k = zip ? e : e - i * M;
  for (int j = 0; j < d; ++j) {
    double dl = 0.0;
    unsigned long long dv = 0ull;
    if (family == 0)
      dl = mod1(static_cast<const double*>(xv)[i * xs + j] - static_cast<const double*>(zv)[k * zs + j]);
    else
      dv = (unsigned long long)(static_cast<const int64_t*>(xv)[i * xs + j] ^ static_cast<const int64_t*>(zv)[k * zs + j]);
    for (int p = 0; p < P; ++p) {
      const int q = p * kWD + j;
      out[((int64_t)p * d + j) * E + e] = wmt_part(family, code_s[q] & 0xff, coef_s[q], add_s[q], dl, dv, t);
    }
  }
}

// ------------------------------------------------------------------------------------------------ first column
// thread = point i, NG hyper-parameter rows per workgroup (blockIdx.y), the lengthscale rows in LDS, the dimensions
// in blocks of 8 loads (k_wide_k1); per p the product over j ascending from 1.0, then acc = fma(cc[p], prod, acc)
template <int NG>
__global__ __launch_bounds__(kWG) void k_wmt_k1(const double* __restrict__ parts, int64_t n, int d, int P, MtInd spec,
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
  double acc[NG];
#pragma unroll
  for (int b = 0; b < NG; ++b) acc[b] = 0.0;
  for (int p = 0; p < P; ++p) {
    const unsigned long long m = spec.ind[p];
    const double* pp = parts + (int64_t)p * d * n + i;
    double pr[NG];
#pragma unroll
    for (int b = 0; b < NG; ++b) pr[b] = 1.0;
    for (int j0 = 0; j0 < d; j0 += 8) {
      double pv[8];
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) pv[jj] = j0 + jj < d ? pp[(int64_t)(j0 + jj) * n] : 0.0;
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) {
        const double one = ((m >> (j0 + jj)) & 1ull) ? 1.0 : 0.0;
#pragma unroll
        for (int b = 0; b < NG; ++b) pr[b] *= __builtin_fma(ls_s[b][j0 + jj], pv[jj], one);
      }
    }
    const double c = spec.cc[p];
#pragma unroll
    for (int b = 0; b < NG; ++b) acc[b] = __builtin_fma(c, pr[b], acc[b]);
  }
#pragma unroll
  for (int b = 0; b < NG; ++b)
    if (g0 + b < G) k1[(int64_t)(g0 + b) * n + i] = scale[g0 + b] * acc[b];
}

// first column, backward: workgroup = (256 points, row g), thread = point; per p the point's d parts in registers
// (DB blocks of 8, padded) and one pass over them as k_wide_k1_bwd.  With f_j = ind_j + l_j p_j, per point and p
//   q = 0:      (u cc) prod_j f_j
//   q = 1 + j:  ((u s cc) p_j) prod_{j' != j} f_j'
// Each quantity is summed over the wave as it is formed and added, in ascending p, to the wave's LDS slot (the per-p
// partials never sit in registers: DB = 8 holds 64 parts already); the 4 waves are then added in order into
// partial[g][q][blk], and k_wmt_k1_bwd_sum reduces over blk.
__device__ __forceinline__ void wmt_wave_sum_acc(double v, double* red_q, bool first) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) {
    const int w = threadIdx.x >> 6;
    red_q[w] = first ? v : red_q[w] + v;
  }
}

template <int DB>
__global__ __launch_bounds__(kWG) void k_wmt_k1_bwd(const double* __restrict__ parts, int64_t n, int d, int P,
                                                    MtInd spec, const double* __restrict__ scale,
                                                    const double* __restrict__ ls, const double* __restrict__ u,
                                                    int64_t nblk, double* __restrict__ partial) {
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
  const double ui = live ? u[(int64_t)g * n + i] : 0.0;      // (a point past n contributes u = 0)
  const double sg = scale[g];
  for (int p = 0; p < P; ++p) {
    const unsigned long long m = spec.ind[p];
    const double* pp = parts + (int64_t)p * d * n + il;
    const bool first = p == 0;
    double pv[DP];
#pragma unroll
    for (int j = 0; j < DP; ++j) pv[j] = j < d ? pp[(int64_t)j * n] : 0.0;
    double sufB[DB + 1];
    sufB[DB] = 1.0;
#pragma unroll
    for (int b = DB - 1; b >= 0; --b) {
      double bp = 1.0;
#pragma unroll
      for (int jj = 0; jj < 8; ++jj)
        bp *= __builtin_fma(ls_s[8 * b + jj], pv[8 * b + jj], ((m >> (8 * b + jj)) & 1ull) ? 1.0 : 0.0);
      sufB[b] = sufB[b + 1] * bp;
    }
    const double uc = ui * spec.cc[p];
    wmt_wave_sum_acc(uc * sufB[0], red[0], first);
    const double us = uc * sg;
    double pre = 1.0;
#pragma unroll
    for (int b = 0; b < DB; ++b) {
      double f[8], suf[9];
#pragma unroll
      for (int jj = 0; jj < 8; ++jj)
        f[jj] = __builtin_fma(ls_s[8 * b + jj], pv[8 * b + jj], ((m >> (8 * b + jj)) & 1ull) ? 1.0 : 0.0);
      suf[8] = sufB[b + 1];
#pragma unroll
      for (int jj = 7; jj >= 0; --jj) suf[jj] = suf[jj + 1] * f[jj];
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) {
        wmt_wave_sum_acc((us * pv[8 * b + jj]) * (pre * suf[jj + 1]), red[1 + 8 * b + jj], first);
        pre *= f[jj];
      }
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

// the sums of k_wmt_k1_bwd's partials (k_wide_k1_bwd_sum): element (g, 0) -> dscale[g], (g, 1 + j) -> dls[g, j]
__global__ __launch_bounds__(kWG) void k_wmt_k1_bwd_sum(const double* __restrict__ partial, int64_t nblk, int d,
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

// ------------------------------------------------------------------------------------------------ kernel rows
// The tables and the lengthscale rows in LDS; a thread walks p (outer, the running sum) and j (inner, the running
// product of its NG rows).  Odd Bernoulli orders are not symmetric about 1/2: the argument is (x - z) mod 1.
template <int NG>
struct MtRowsLds {
  int code[kMtP * kWD];
  double coef[kMtP * kWD];
  double add[kMtP * kWD];
  double ls[NG][kWD];
};

template <int NG>
__device__ __forceinline__ void wmt_rows_tables(MtRowsLds<NG>& s, const MtTables* __restrict__ tab, int P, int d,
                                                const double* __restrict__ hyp, int g0, int Gk) {
  for (int e = threadIdx.x; e < P * kWD; e += kWG) {
    s.code[e] = tab->code[e];
    s.coef[e] = tab->coef[e];
    s.add[e] = tab->add[e];
  }
  for (int e = threadIdx.x; e < NG * kWD; e += kWG) {
    const int b = e / kWD, j = e % kWD;
    const int g = g0 + b < Gk ? g0 + b : Gk - 1;
    s.ls[b][j] = j < d ? hyp[(int64_t)g * (1 + d) + 1 + j] : 0.0;
  }
}

// acc[b] = sum_p cc[p] prod_j (ind + l_bj part_pj) of one (test point, training point) pair: coordinate j of the test
// point from xj(j) (LDS or global), of the training point from z[j * zs + zi]
template <int FAM, int NG, typename XJ>
__device__ __forceinline__ void wmt_rows_pair(const MtRowsLds<NG>& s, const MtCc& cc, int P, int d, int tbits, XJ xj,
                                              const void* __restrict__ z, int64_t zs, int64_t zi, double (&acc)[NG]) {
#pragma unroll
  for (int b = 0; b < NG; ++b) acc[b] = 0.0;
  for (int p = 0; p < P; ++p) {
    double pr[NG];
#pragma unroll
    for (int b = 0; b < NG; ++b) pr[b] = 1.0;
    for (int j = 0; j < d; ++j) {
      const int q = p * kWD + j;
      const int code = s.code[q];
      double dl = 0.0;
      unsigned long long dv = 0ull;
      if constexpr (FAM == 0) {
        dl = mod1(xj(j) - static_cast<const double*>(z)[(int64_t)j * zs + zi]);
      } else {
        dv = (unsigned long long)__double_as_longlong(xj(j)) ^
             (unsigned long long)static_cast<const long long*>(z)[(int64_t)j * zs + zi];
      }
      const double part = wmt_part(FAM, code & 0xff, s.coef[q], s.add[q], dl, dv, tbits);
      const double one = (code >> 8) ? 1.0 : 0.0;
#pragma unroll
      for (int b = 0; b < NG; ++b) pr[b] *= __builtin_fma(s.ls[b][j], part, one);
    }
    const double c = cc.cc[p];
#pragma unroll
    for (int b = 0; b < NG; ++b) acc[b] = __builtin_fma(c, pr[b], acc[b]);
  }
}

// thread = training point i, workgroup = (256 points, test point t, NG rows); the test point in LDS (nets: as t-bit
// integers)
template <int FAM, int NG>
__global__ __launch_bounds__(kWG) void k_wmt_rows(const double* __restrict__ xt, int64_t N, const void* __restrict__ z,
                                                  int64_t n, int d, int P, const MtTables* __restrict__ tab, MtCc cc,
                                                  int tbits, const double* __restrict__ hyp, int Gk,
                                                  double* __restrict__ rows) {
  __shared__ MtRowsLds<NG> s;
  __shared__ double xs[kWD];
  const int tid = threadIdx.x;
  const int64_t t = blockIdx.y;
  const int g0 = blockIdx.z * NG;
  wmt_rows_tables<NG>(s, tab, P, d, hyp, g0, Gk);
  if (tid < d) {
    const double v = xt[t * d + tid];
    if constexpr (FAM == 0) xs[tid] = v;
    else xs[tid] = __longlong_as_double((long long)to_bits(v, tbits));
  }
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * kWG + tid;
  if (i >= n) return;
  double acc[NG];
  wmt_rows_pair<FAM, NG>(s, cc, P, d, tbits, [&](int j) { return xs[j]; }, z, n, i, acc);
#pragma unroll
  for (int b = 0; b < NG; ++b)
    if (g0 + b < Gk) rows[((int64_t)(g0 + b) * N + t) * n + i] = hyp[(int64_t)(g0 + b) * (1 + d)] * acc[b];
}

// zip: thread = pair t, rows[g][t] = K(xt_t, z_t); workgroup = (256 pairs, NG rows)
template <int FAM, int NG>
__global__ __launch_bounds__(kWG) void k_wmt_rows_zip(const double* __restrict__ xt, int64_t N,
                                                      const void* __restrict__ z, int d, int P,
                                                      const MtTables* __restrict__ tab, MtCc cc, int tbits,
                                                      const double* __restrict__ hyp, int Gk, double* __restrict__ rows) {
  __shared__ MtRowsLds<NG> s;
  const int g0 = blockIdx.y * NG;
  wmt_rows_tables<NG>(s, tab, P, d, hyp, g0, Gk);
  __syncthreads();
  const int64_t t = (int64_t)blockIdx.x * kWG + threadIdx.x;
  if (t >= N) return;
  double acc[NG];
  wmt_rows_pair<FAM, NG>(
      s, cc, P, d, tbits,
      [&](int j) {
        const double v = xt[t * d + j];
        if constexpr (FAM == 0) return v;
        else return __longlong_as_double((long long)to_bits(v, tbits));
      },
      z, N, t, acc);
#pragma unroll
  for (int b = 0; b < NG; ++b)
    if (g0 + b < Gk) rows[(int64_t)(g0 + b) * N + t] = hyp[(int64_t)(g0 + b) * (1 + d)] * acc[b];
}

// ------------------------------------------------------------------------------------------------ posterior mean
// partial[b][t][c] = sum_{i in chunk c} K^{(g(b))}(xt_t, z_i) coeffs[b][i] of one task pair, no kernel row stored.
// k_wmt_rows' mapping: thread = training point, striding through the chunk in steps of kWG; workgroup = (chunk c, test
// point t, NB output rows).  The pair's value is wmt_rows_pair's and then the scale, the bits k_wmt_rows writes; a thread
// adds its points in ascending i with sum = fma(K, c_i, sum), block_sum adds the threads.  NK kernel rows per workgroup:
// 1 when every output row shares the hyper-parameters (Gk == 1: the kernel is evaluated once for the NB rows), else NB.
// A row past B repeats row B - 1 and is not stored.  The chunk bounds depend on n and the chunk length alone.
constexpr int kMtPmB = 4;                   // output rows per workgroup
constexpr int64_t kMtPmChunk = 1024;        // default chunk of training points: 4 per thread
constexpr int64_t kMtPmNt = 65535;          // test points per launch (grid.y)

template <int FAM, int NK, int NB>
__global__ __launch_bounds__(kWG) void k_wmt_post_mean(const double* __restrict__ xt, int64_t N,
                                                       const void* __restrict__ z, int64_t n, int d, int P,
                                                       const MtTables* __restrict__ tab, MtCc cc, int tbits,
                                                       const double* __restrict__ hyp, int Gk,
                                                       const double* __restrict__ coeffs, int64_t cstride, int B,
                                                       int64_t chunk, int64_t nchunks, double* __restrict__ partial) {
  static_assert(NK == 1 || NK == NB, "one kernel row for all output rows, or one each");
  __shared__ MtRowsLds<NK> s;
  __shared__ double xs[kWD];
  __shared__ double red[kWG / 64];
  const int tid = threadIdx.x;
  const int64_t t = blockIdx.y;
  const int b0 = blockIdx.z * NB;
  wmt_rows_tables<NK>(s, tab, P, d, hyp, NK == 1 ? 0 : b0, Gk);
  if (tid < d) {
    const double v = xt[t * d + tid];
    if constexpr (FAM == 0) xs[tid] = v;
    else xs[tid] = __longlong_as_double((long long)to_bits(v, tbits));
  }
  __syncthreads();
  double sc[NK], sum[NB];
  const double* cb[NB];
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const int g = NK == 1 ? 0 : (b0 + k < Gk ? b0 + k : Gk - 1);
    sc[k] = hyp[(int64_t)g * (1 + d)];
  }
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    sum[b] = 0.0;
    cb[b] = coeffs + (int64_t)(b0 + b < B ? b0 + b : B - 1) * cstride;
  }
  const int64_t i0 = (int64_t)blockIdx.x * chunk;
  const int64_t i1 = i0 + chunk < n ? i0 + chunk : n;
  for (int64_t i = i0 + tid; i < i1; i += kWG) {
    double acc[NK];
    wmt_rows_pair<FAM, NK>(s, cc, P, d, tbits, [&](int j) { return xs[j]; }, z, n, i, acc);
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const int k = NK == 1 ? 0 : b;
      sum[b] = __builtin_fma(sc[k] * acc[k], cb[b][i], sum[b]);
    }
  }
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const double v = block_sum(sum[b], red);
    if (tid == 0 && b0 + b < B) partial[((int64_t)(b0 + b) * N + t) * nchunks + blockIdx.x] = v;
  }
}

// out[b][t] = beta out[b][t] + w[b] sum_c partial[b][t][c]: one workgroup per output, a lane over every kWG-th chunk in
// ascending order, then block_sum's fixed tree (k_wide_sum); w NULL: 1; beta 0 (out is not read) or 1
__global__ __launch_bounds__(kWG) void k_wmt_post_mean_sum(const double* __restrict__ partial, int64_t nchunks, int64_t N,
                                                           const double* __restrict__ w, int beta,
                                                           double* __restrict__ out, int64_t out_stride) {
  __shared__ double red[kWG / 64];
  const int64_t t = blockIdx.x, b = blockIdx.y;
  const double* p = partial + (b * N + t) * nchunks;
  double s = 0.0;
  for (int64_t c = threadIdx.x; c < nchunks; c += kWG) s += p[c];
  s = block_sum(s, red);
  if (threadIdx.x == 0) {
    const double v = w ? w[b] * s : s;
    double* o = out + b * out_stride + t;
    *o = beta ? *o + v : v;
  }
}

// ------------------------------------------------------------------------------------------------ host side
// argument checks shared by the entry points (before any HIP call)
static int wmt_dp_ok(const char* fn, int d, int P) {
  int rc = wide_d_ok(fn, d);
  if (rc != kOk) return rc;
  if (P < 1) return set_error(kErrInvalid, "%s: P=%d (at least 1 derivative multi-index pair)", fn, P);
  if (P > kMtP) return set_error(kErrUnsupported, "%s: P=%d above %d (the torch formulation covers more)", fn, P, kMtP);
  return kOk;
}

static int wmt_ind(const char* fn, int d, int P, const int* ind, const double* cc, MtInd& out) {
  if (!ind || !cc) return set_error(kErrInvalid, "%s: null pointer (ind / cc)", fn);
  for (int p = 0; p < kMtP; ++p) {
    unsigned long long m = ~0ull;
    for (int j = 0; p < P && j < d; ++j) {
      const int v = ind[p * d + j];
      if (v != 0 && v != 1) return set_error(kErrInvalid, "%s: ind[%d][%d]=%d is not 0 or 1", fn, p, j, v);
      if (!v) m &= ~(1ull << j);
    }
    out.ind[p] = m;
    out.cc[p] = p < P ? cc[p] : 0.0;
  }
  return kOk;
}

static int wmt_tables(const char* fn, int family, int d, int P, const int* order, const double* coef, const double* add,
                      const int* ind, int tbits, MtTables& tab) {
  if (family != FGP_FAMILY_LATTICE && family != FGP_FAMILY_NET) return set_error(kErrInvalid, "%s: bad family %d", fn, family);
  const bool net = family == FGP_FAMILY_NET;
  if (!order || !coef || (net && !add)) return set_error(kErrInvalid, "%s: null pointer (order / coef / add)", fn);
  if (net && (tbits < 1 || tbits > 63)) return set_error(kErrInvalid, "%s: tbits=%d outside 1..63", fn, tbits);
  std::memset(&tab, 0, sizeof(tab));
  for (int p = 0; p < P; ++p)
    for (int j = 0; j < kWD; ++j) {
      const int q = p * kWD + j;
      if (j >= d) {
        tab.code[q] = 1 | (1 << 8);
        continue;
      }
      const int o = order[p * d + j];
      if (o < 1 || o > (net ? 4 : 8))
        return set_error(kErrUnsupported, "%s: %s order[%d][%d]=%d outside 1..%d", fn, net ? "Walsh" : "Bernoulli", p, j, o,
                         net ? 4 : 8);
      const int one = ind ? ind[p * d + j] : 1;
      if (one != 0 && one != 1) return set_error(kErrInvalid, "%s: ind[%d][%d]=%d is not 0 or 1", fn, p, j, one);
      tab.code[q] = o | (one << 8);
      tab.coef[q] = coef[p * d + j];
      tab.add[q] = (net || add) ? add[p * d + j] : 0.0;
    }
  return kOk;
}

// The tables of a spec on the current device, uploaded once (a blocking copy into a buffer of their own, so nothing
// in flight reads it) and found again by content: the entry points take host tables -- they validate them -- and the
// kernels read 20 KB that no kernel-argument block holds.  At most kSpecCache specs are kept; past that every buffer
// is released after a device synchronisation.
struct SpecEntry {
  int dev;
  MtTables host;
  MtTables* devp;
};
constexpr size_t kSpecCache = 64;
static std::mutex g_spec_mu;
static std::vector<SpecEntry*> g_specs;

static int wmt_device_tables(const char* fn, const MtTables& tab, const MtTables** out) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return set_error(kErrHip, "%s: hipGetDevice failed", fn);
  std::lock_guard<std::mutex> lk(g_spec_mu);
  for (SpecEntry* e : g_specs)
    if (e->dev == dev && std::memcmp(&e->host, &tab, sizeof(MtTables)) == 0) {
      *out = e->devp;
      return kOk;
    }
  if (g_specs.size() >= kSpecCache) {
    if (hipDeviceSynchronize() != hipSuccess) return set_error(kErrHip, "%s: hipDeviceSynchronize failed", fn);
    for (SpecEntry* e : g_specs) {
      (void)hipFree(e->devp);
      delete e;
    }
    g_specs.clear();
  }
  SpecEntry* e = new SpecEntry{dev, tab, nullptr};
  if (hipMalloc((void**)&e->devp, sizeof(MtTables)) != hipSuccess ||
      hipMemcpy(e->devp, &tab, sizeof(MtTables), hipMemcpyHostToDevice) != hipSuccess) {
    if (e->devp) (void)hipFree(e->devp);
    delete e;
    return set_error(kErrHip, "%s: uploading the spec tables failed", fn);
  }
  g_specs.push_back(e);
  *out = e->devp;
  return kOk;
}

}  // namespace fgp

using namespace fgp;

extern "C" {

int fgp_wide_mt_parts(int family, const void* x, int64_t x_row_stride, int64_t N, const void* z, int64_t z_row_stride,
                      int64_t M, int zip, int d, int P, const int* order, const double* coef, const double* add,
                      int tbits, double* parts, void* stream) {
  static const char* fn = "fgp_wide_mt_parts";
  int rc = wmt_dp_ok(fn, d, P);
  if (rc != kOk) return rc;
  if (N < 0 || M < 0 || x_row_stride < 0 || z_row_stride < 0)
    return set_error(kErrInvalid, "%s: negative size (N=%lld M=%lld)", fn, (long long)N, (long long)M);
  if (zip && N != M) return set_error(kErrInvalid, "%s: zip needs N == M", fn);
  if (!x || !z || !parts) return set_error(kErrInvalid, "%s: null pointer (x / z / parts)", fn);
  static thread_local MtTables tab;
  rc = wmt_tables(fn, family, d, P, order, coef, add, nullptr, tbits, tab);
  if (rc != kOk) return rc;
  const int64_t cnt = zip ? N : N * M;
  if (cnt == 0) return kOk;
  if ((cnt + kWG - 1) / kWG > 0x7fffffffll) return set_error(kErrUnsupported, "%s: %lld pairs", fn, (long long)cnt);
  const MtTables* dt = nullptr;
  rc = wmt_device_tables(fn, tab, &dt);
  if (rc != kOk) return rc;
  k_wmt_parts<<<(unsigned)((cnt + kWG - 1) / kWG), kWG, 0, (hipStream_t)stream>>>(family, x, x_row_stride, N, z,
                                                                                    z_row_stride, M, zip, d, P, dt, tbits,
                                                                                    parts);
  return check_launch("k_wmt_parts");
}

int fgp_wide_mt_k1(const double* parts, int64_t n, int d, int P, const int* ind, const double* cc, const double* scale,
                   const double* ls, int G, double* k1, void* stream) {
  static const char* fn = "fgp_wide_mt_k1";
  int rc = wmt_dp_ok(fn, d, P);
  if (rc != kOk) return rc;
  if (n < 0 || G < 1 || G > 65535 * kMtRowsG) return set_error(kErrInvalid, "%s: bad n=%lld / G=%d", fn, (long long)n, G);
  if (!parts || !scale || !ls || !k1) return set_error(kErrInvalid, "%s: null pointer (parts / scale / ls / k1)", fn);
  MtInd spec;
  rc = wmt_ind(fn, d, P, ind, cc, spec);
  if (rc != kOk) return rc;
  if (n == 0) return kOk;
  hipStream_t st = (hipStream_t)stream;
  const unsigned nb = (unsigned)((n + kWG - 1) / kWG);
  if (G == 1) k_wmt_k1<1><<<dim3(nb, 1), kWG, 0, st>>>(parts, n, d, P, spec, scale, ls, G, k1);
  else k_wmt_k1<kMtRowsG><<<dim3(nb, (unsigned)((G + kMtRowsG - 1) / kMtRowsG)), kWG, 0, st>>>(parts, n, d, P, spec, scale, ls, G, k1);
  return check_launch("k_wmt_k1");
}

int fgp_wide_mt_k1_bwd_work(int64_t n, int d, int P, int G, int64_t* len) {
  static const char* fn = "fgp_wide_mt_k1_bwd_work";
  int rc = wmt_dp_ok(fn, d, P);
  if (rc != kOk) return rc;
  if (n < 0 || G < 1) return set_error(kErrInvalid, "%s: bad n=%lld / G=%d", fn, (long long)n, G);
  if (!len) return set_error(kErrInvalid, "%s: null pointer (len)", fn);
  *len = std::max<int64_t>(1, (int64_t)G * (1 + d) * ((n + kWG - 1) / kWG));
  return kOk;
}

int fgp_wide_mt_k1_bwd(const double* parts, int64_t n, int d, int P, const int* ind, const double* cc,
                       const double* scale, const double* ls, int G, const double* u, double* dscale, double* dls,
                       double* work, void* stream) {
  static const char* fn = "fgp_wide_mt_k1_bwd";
  int rc = wmt_dp_ok(fn, d, P);
  if (rc != kOk) return rc;
  if (n < 1 || n > ((int64_t)1 << 31) || G < 1 || G > 65535)
    return set_error(kErrInvalid, "%s: bad n=%lld / G=%d", fn, (long long)n, G);
  if (!parts || !scale || !ls || !u || !dscale || !dls || !work)
    return set_error(kErrInvalid, "%s: null pointer (parts / scale / ls / u / dscale / dls / work)", fn);
  MtInd spec;
  rc = wmt_ind(fn, d, P, ind, cc, spec);
  if (rc != kOk) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int64_t nblk = (n + kWG - 1) / kWG;
  const dim3 grid((unsigned)nblk, (unsigned)G);
  rc = dispatch_range<2, 8>((d + 7) / 8, [&](auto dbc) {
    k_wmt_k1_bwd<decltype(dbc)::value><<<grid, kWG, 0, st>>>(parts, n, d, P, spec, scale, ls, u, nblk, work);
    return check_launch("k_wmt_k1_bwd");
  });
  if (rc != kOk) return no_kernel(rc, fn, d);
  k_wmt_k1_bwd_sum<<<(unsigned)((int64_t)G * (1 + d)), kWG, 0, st>>>(work, nblk, d, dscale, dls);
  return check_launch("k_wmt_k1_bwd_sum");
}

int fgp_wide_mt_rows(int family, const double* xt, int64_t N, const void* z, int64_t n, int zip, int d, int P,
                     const int* order, const double* coef, const double* add, const int* ind, const double* cc,
                     int tbits, const double* hyp, int Gk, double* rows, void* stream) {
  static const char* fn = "fgp_wide_mt_rows";
  int rc = wmt_dp_ok(fn, d, P);
  if (rc != kOk) return rc;
  if (N < 0 || n < 1 || Gk < 1 || Gk > 65535 * kMtRowsG || (!zip && N > 65535))
    return set_error(kErrInvalid, "%s: bad sizes (N=%lld n=%lld Gk=%d)", fn, (long long)N, (long long)n, Gk);
  if (zip && N != n) return set_error(kErrInvalid, "%s: zip needs N == n", fn);
  if (!xt || !z || !hyp || !rows) return set_error(kErrInvalid, "%s: null pointer (xt / z / hyp / rows)", fn);
  MtInd is;
  rc = wmt_ind(fn, d, P, ind, cc, is);
  if (rc != kOk) return rc;
  static thread_local MtTables tab;
  rc = wmt_tables(fn, family, d, P, order, coef, add, ind, tbits, tab);
  if (rc != kOk) return rc;
  if (N == 0) return kOk;
  MtCc c;
  for (int p = 0; p < kMtP; ++p) c.cc[p] = is.cc[p];
  const MtTables* dt = nullptr;
  rc = wmt_device_tables(fn, tab, &dt);
  if (rc != kOk) return rc;
  hipStream_t st = (hipStream_t)stream;
  const bool lat = family == FGP_FAMILY_LATTICE;
  const unsigned gb = Gk == 1 ? 1u : (unsigned)((Gk + kMtRowsG - 1) / kMtRowsG);
#define FGP_WMT(KERNEL, GRID, ...)                                                         \
  do {                                                                                     \
    if (lat && Gk == 1) KERNEL<0, 1><<<GRID, kWG, 0, st>>>(__VA_ARGS__);                   \
    else if (lat) KERNEL<0, kMtRowsG><<<GRID, kWG, 0, st>>>(__VA_ARGS__);                  \
    else if (Gk == 1) KERNEL<1, 1><<<GRID, kWG, 0, st>>>(__VA_ARGS__);                     \
    else KERNEL<1, kMtRowsG><<<GRID, kWG, 0, st>>>(__VA_ARGS__);                           \
  } while (0)
  if (zip) {
    const dim3 grid((unsigned)((N + kWG - 1) / kWG), gb);
    FGP_WMT(k_wmt_rows_zip, grid, xt, N, z, d, P, dt, c, tbits, hyp, Gk, rows);
    return check_launch("k_wmt_rows_zip");
  }
  const dim3 grid((unsigned)((n + kWG - 1) / kWG), (unsigned)N, gb);
  FGP_WMT(k_wmt_rows, grid, xt, N, z, n, d, P, dt, c, tbits, hyp, Gk, rows);
#undef FGP_WMT
  return check_launch("k_wmt_rows");
}

// the chunk of training points of fgp_mt_wide_post_mean: 0 = the default, else a positive multiple of kWG
static int wmt_pm_sizes(const char* fn, int64_t N, int64_t n, int B, int64_t chunk, int64_t* chunk_out,
                        int64_t* nchunks) {
  if (N < 0) return set_error(kErrInvalid, "%s: N=%lld is negative", fn, (long long)N);
  if (n < 1) return set_error(kErrInvalid, "%s: n=%lld (at least 1 training point)", fn, (long long)n);
  if (B < 1 || B > 65535) return set_error(kErrInvalid, "%s: B=%d outside 1..65535", fn, B);
  if (chunk < 0 || chunk % kWG != 0)
    return set_error(kErrInvalid, "%s: chunk=%lld is not 0 (default) or a positive multiple of %d", fn, (long long)chunk, kWG);
  const int64_t ch = chunk ? chunk : kMtPmChunk;
  const int64_t nc = (n - 1) / ch + 1;
  if (nc > 0x7fffffffll) return set_error(kErrUnsupported, "%s: n=%lld needs %lld chunks", fn, (long long)n, (long long)nc);
  *chunk_out = ch;
  *nchunks = nc;
  return kOk;
}

int fgp_mt_wide_post_mean_work(int64_t N, int64_t n, int B, int64_t chunk, int64_t* len) {
  static const char* fn = "fgp_mt_wide_post_mean_work";
  int64_t ch = 0, nc = 0;
  int rc = wmt_pm_sizes(fn, N, n, B, chunk, &ch, &nc);
  if (rc != kOk) return rc;
  if (!len) return set_error(kErrInvalid, "%s: null pointer (len)", fn);
  *len = std::max<int64_t>(1, (int64_t)B * std::min<int64_t>(N, kMtPmNt) * nc);
  return kOk;
}

int fgp_mt_wide_post_mean(int family, const double* xt, int64_t N, const void* z, int64_t n, int d, int P,
                          const int* order, const double* coef, const double* add, const int* ind, const double* cc,
                          int tbits, const double* hyp, int Gk, const double* coeffs, int64_t coeff_stride, int B,
                          const double* w, int beta, double* out, int64_t out_stride, double* work, int64_t chunk,
                          void* stream) {
  static const char* fn = "fgp_mt_wide_post_mean";
  int rc = wmt_dp_ok(fn, d, P);
  if (rc != kOk) return rc;
  int64_t ch = 0, nchunks = 0;
  rc = wmt_pm_sizes(fn, N, n, B, chunk, &ch, &nchunks);
  if (rc != kOk) return rc;
  if (Gk != 1 && Gk != B) return set_error(kErrInvalid, "%s: Gk=%d is neither 1 nor B=%d", fn, Gk, B);
  if (beta != 0 && beta != 1) return set_error(kErrInvalid, "%s: beta=%d is not 0 or 1", fn, beta);
  if (coeff_stride < (B > 1 ? n : 0))
    return set_error(kErrInvalid, "%s: coeff_stride=%lld below n=%lld", fn, (long long)coeff_stride, (long long)n);
  if (out_stride < (B > 1 ? N : 0))
    return set_error(kErrInvalid, "%s: out_stride=%lld below N=%lld", fn, (long long)out_stride, (long long)N);
  if (!xt) return set_error(kErrInvalid, "%s: null pointer (xt)", fn);
  if (!z) return set_error(kErrInvalid, "%s: null pointer (z)", fn);
  if (!hyp) return set_error(kErrInvalid, "%s: null pointer (hyp)", fn);
  if (!coeffs) return set_error(kErrInvalid, "%s: null pointer (coeffs)", fn);
  if (!out) return set_error(kErrInvalid, "%s: null pointer (out)", fn);
  if (!work) return set_error(kErrInvalid, "%s: null pointer (work)", fn);
  MtInd is;
  rc = wmt_ind(fn, d, P, ind, cc, is);
  if (rc != kOk) return rc;
  static thread_local MtTables tab;
  rc = wmt_tables(fn, family, d, P, order, coef, add, ind, tbits, tab);
  if (rc != kOk) return rc;
  if (N == 0) return kOk;
  MtCc c;
  for (int p = 0; p < kMtP; ++p) c.cc[p] = is.cc[p];
  const MtTables* dt = nullptr;
  rc = wmt_device_tables(fn, tab, &dt);
  if (rc != kOk) return rc;
  hipStream_t st = (hipStream_t)stream;
  const bool lat = family == FGP_FAMILY_LATTICE;
  const unsigned gz = B == 1 ? 1u : (unsigned)((B + kMtPmB - 1) / kMtPmB);
  // the test points in launches of at most kMtPmNt: a point's chunks and their order do not depend on the split
  for (int64_t t0 = 0; t0 < N; t0 += kMtPmNt) {
    const int64_t Nc = std::min<int64_t>(kMtPmNt, N - t0);
    const dim3 grid((unsigned)nchunks, (unsigned)Nc, gz);
#define FGP_WMT_PM(FAM, NK, NB)                                                                                          \
  k_wmt_post_mean<FAM, NK, NB><<<grid, kWG, 0, st>>>(xt + t0 * d, Nc, z, n, d, P, dt, c, tbits, hyp, Gk, coeffs, coeff_stride, \
                                                      B, ch, nchunks, work)
    if (lat) {
      if (B == 1) FGP_WMT_PM(0, 1, 1);
      else if (Gk == 1) FGP_WMT_PM(0, 1, kMtPmB);
      else FGP_WMT_PM(0, kMtPmB, kMtPmB);
    } else {
      if (B == 1) FGP_WMT_PM(1, 1, 1);
      else if (Gk == 1) FGP_WMT_PM(1, 1, kMtPmB);
      else FGP_WMT_PM(1, kMtPmB, kMtPmB);
    }
#undef FGP_WMT_PM
    rc = check_launch("k_wmt_post_mean");
    if (rc != kOk) return rc;
    k_wmt_post_mean_sum<<<dim3((unsigned)Nc, (unsigned)B), kWG, 0, st>>>(work, nchunks, Nc, w, beta, out + t0, out_stride);
    rc = check_launch("k_wmt_post_mean_sum");
    if (rc != kOk) return rc;
  }
  return kOk;
}

}  // extern "C"
