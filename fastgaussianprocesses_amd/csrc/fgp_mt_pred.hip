// Multitask / derivative-informed predictions at 1 <= d <= FGP_MAX_D (8): the task-pair kernel of
// abstract_fast_gp.py:173-191 with 1 <= P <= FGP_WIDE_MT_MAX_P (16) derivative multi-index pairs, formed from the points,
//
//   K_ab(x, z) = scale sum_p cc[p] prod_j (ind[p][j] + l_j part[p][j](x, z)),
//   part = coef B_order((x_j - z_j) mod 1)  (lattice),  coef (add + omega_order(x_j XOR z_j))  (net),
//
// beside fgp_mt_parts + the torch formulation (a [N, M, P, d] parts array) and the wide kernels of fgp_wide_mt.hip
// (9 <= d <= 64: per-dimension tables in LDS, run-time loops over d).  A part has the arithmetic of k_mt_parts /
// k_wmt_parts (wmt_part, fgp_factors.h): it carries the bits fgp_mt_parts writes.
//
//   k_mt_rows        rows[g][t][i] = K_ab(xt_t, z_i)
//   k_mt_rows_zip    rows[g][t]    = K_ab(xt_t, z_t)
//   k_mt_post_mean   partial[b][t][c] = sum_{i in chunk c} K^{(g(b))}(xt_t, z_i) coeffs[b][i]; k_mt_post_mean_sum adds
//                    the chunks, then w and beta: no kernel row stored
//
// Templates on <FAM, D>: the loop over the dimensions is unrolled, no per-thread array is indexed by a run-time value.
// A thread holds the workgroup's test point (nets: as t-bit integers) and one hyper-parameter row's lengthscales and
// scale in registers (NG > 1 rows: in LDS, MtHyp); the pair's tables (16 x 8 entries of
// order | ind << 8, coef, add, and cc[16]: 2.7 KB) are a kernel argument BY VALUE, indexed by the wave-uniform p and a
// compile-time j, so they arrive through scalar loads from the argument segment: no LDS table, no device-side table
// cache, no upload.  A thread loads its training point's D coordinates once and forms the D differences once, for
// every p.  PONE: the P == 1 instance (every pair of a GP whose tasks are single partial derivatives) without the loop
// over p; it keeps the fma with cc[0] onto 0.0, so it has the generic instance's bits.
// The product runs in ascending j, the sum in ascending p, then the scale.  Every reduction is fixed-order (block_sum's
// tree, per-chunk partials, one workgroup per output): no atomics, no inter-workgroup hand-off.
//
// Register use depends on how the compiler hoists: the empty asm statements below (on a table index, on pbase, on a
// difference) and the volatile LDS pointer of MtHyp keep the tables' entries, every order's polynomial and the nets' zero
// tests from being held across the loops, and with that the scalar file from spilling to VGPR lanes and the occupancy
// from falling to one wave.  No test guards this: after a compiler change, regenerate
// profiles/r12a_kernel_resources_mt_pred.txt (tools/kernel_resources.py --grep 'k_mt_rows|k_mt_post_mean') and check
// that every instance still shows no spill and no scratch.
#include <algorithm>
#include <cstring>

#include "fgp_common.h"
#include "fgp_factors.h"
#include "fgp_runtime.h"
#include "../../include/fgp_hip.h"

namespace fgp {

constexpr int kNpP = FGP_WIDE_MT_MAX_P;   // derivative multi-index pairs
constexpr int kNpD = FGP_MAX_D;           // table stride over the dimensions
constexpr int kNpG = 4;                   // hyper-parameter rows per k_mt_rows workgroup / output rows per k_mt_post_mean one
constexpr int64_t kNpChunk = 1024;        // default chunk of training points of the mean: 4 per thread
constexpr int64_t kNpNt = 65535;          // test points per launch (grid.y)

// the pair's spec, by value: entry p * kNpD + j
struct MtPairTab {
  double coef[kNpP * kNpD];
  double add[kNpP * kNpD];
  double cc[kNpP];
  int code[kNpP * kNpD];                  // order | ind << 8
};
static_assert(sizeof(MtPairTab) <= 3072, "the tables travel in the kernel-argument segment (4 KB)");

// The test point as the pair function takes it: doubles (lattice) or t-bit integers (net).  A workgroup's test point is
// converted once, by D threads, into LDS and read from there: a thread then holds it in VGPRs, beside its training
// point, and the SGPRs stay free for the tables and the lengthscales (k_mt_rows_zip: the point is the thread's own).
template <int FAM, int D>
struct MtPoint {
  double x[D];
  unsigned long long b[D];
  __device__ __forceinline__ void load(const double* __restrict__ p, int tbits) {
#pragma unroll
    for (int j = 0; j < D; ++j) {
      if constexpr (FAM == 0) x[j] = p[j];
      else b[j] = to_bits(p[j], tbits);
    }
  }
  __device__ __forceinline__ void stage(double* xs, const double* __restrict__ p, int tbits) const {
    if (threadIdx.x < D) {
      const double v = p[threadIdx.x];
      if constexpr (FAM == 0) xs[threadIdx.x] = v;
      else xs[threadIdx.x] = __longlong_as_double((long long)to_bits(v, tbits));
    }
  }
  __device__ __forceinline__ void take(const double* xs) {
#pragma unroll
    for (int j = 0; j < D; ++j) {
      if constexpr (FAM == 0) x[j] = xs[j];
      else b[j] = (unsigned long long)__double_as_longlong(xs[j]);
    }
  }
};

// Hyper-parameter rows g0 .. g0 + NG - 1 (a row past Gk repeats row Gk - 1), staged in LDS as [NG][1 + D] (scale,
// lengthscales) by the first NG (1 + D) threads.  NG == 1: a thread takes the row into registers once.  NG > 1: a
// factor reads its lengthscale from LDS where it is used, a broadcast read at a compile-time offset (volatile: hoisted
// out of the loops the NG D values would cost 2 NG D VGPRs and the occupancy with them).  The scalar file is left to
// the tables, the constants of the parts and the loop state, which fill it at D = 8.
template <int D, int NG>
struct MtHyp {
  double lsr[NG == 1 ? D : 1];
  double scr;
  const volatile double* s;
  __device__ __forceinline__ void stage(double* lds, const double* __restrict__ hyp, int g0, int Gk) {
    if (threadIdx.x < NG * (1 + D)) {
      const int b = threadIdx.x / (1 + D), q = threadIdx.x % (1 + D);
      const int g = g0 + b < Gk ? g0 + b : Gk - 1;
      lds[threadIdx.x] = hyp[(int64_t)g * (1 + D) + q];
    }
    s = lds;
  }
  __device__ __forceinline__ void take() {
    if constexpr (NG == 1) {
      scr = s[0];
#pragma unroll
      for (int j = 0; j < D; ++j) lsr[j] = s[1 + j];
    }
  }
  __device__ __forceinline__ double ls(int b, int j) const {
    if constexpr (NG == 1) return lsr[j];
    else return s[b * (1 + D) + 1 + j];
  }
  __device__ __forceinline__ double sc(int b) const {
    if constexpr (NG == 1) return scr;
    else return s[b * (1 + D)];
  }
};

// acc[b] = sum_p cc[p] prod_j (ind + l_bj part_pj) of the pair (test point, training point zi of z [D][zs])
template <int FAM, int D, int NG, bool PONE>
__device__ __forceinline__ void mt_pair(const MtPairTab& tab, int P, int tbits, const MtPoint<FAM, D>& x,
                                        const MtHyp<D, NG>& h, const void* __restrict__ z, int64_t zs, int64_t zi,
                                        double (&acc)[NG], int pbase = 0) {
  double dl[D];
  unsigned long long dv[D];
  // (a running pointer, one stride: the D - 1 multiples j zs as loop-invariant scalars would not fit the scalar file)
  const char* zp = static_cast<const char*>(z) + zi * 8;
#pragma unroll
  for (int j = 0; j < D; ++j) {
    if constexpr (FAM == 0) {
      dl[j] = mod1(x.x[j] - *reinterpret_cast<const double*>(zp));
      dv[j] = 0ull;
    } else {
      dl[j] = 0.0;
      dv[j] = x.b[j] ^ (unsigned long long)*reinterpret_cast<const long long*>(zp);
    }
    zp += zs * 8;
  }
#pragma unroll
  for (int b = 0; b < NG; ++b) acc[b] = 0.0;
  const int Pn = PONE ? 1 : P;
  for (int p = 0; p < Pn; ++p) {
    double pr[NG];
#pragma unroll
    for (int b = 0; b < NG; ++b) pr[b] = 1.0;
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const int q = (pbase + p) * kNpD + j;
      // wmt_part in its two steps: ind, coef and add are fetched behind the polynomial (q behind an empty asm), or
      // the D entries' scalar loads are issued together and held, 5 SGPRs each, across the D polynomials
      // (P > 1: the difference behind an empty asm as well.  The polynomial of entry (p, j) is then evaluated here, for
      // its one order; left to hoist what does not depend on p, the compiler keeps every order's polynomial of every
      // dimension in VGPRs -- 256 of them at D = 8, one wave per SIMD -- and the nets' zero tests in SGPR pairs)
      double dlj = dl[j];
      unsigned long long dvj = dv[j];
      if constexpr (!PONE) {
        if constexpr (FAM == 0) asm volatile("" : "+v"(dlj));
        else asm volatile("" : "+v"(dvj));
      }
      const double base = wmt_base(FAM, tab.code[q] & 0xff, dlj, dvj, tbits);
      int q2 = q;
      asm volatile("" : "+s"(q2));
      const double part = wmt_finish(FAM, tab.coef[q2], tab.add[q2], base);
      const double one = (tab.code[q2] >> 8) ? 1.0 : 0.0;
#pragma unroll
      for (int b = 0; b < NG; ++b) pr[b] *= __builtin_fma(h.ls(b, j), part, one);
    }
    const double c = tab.cc[pbase + p];
#pragma unroll
    for (int b = 0; b < NG; ++b) acc[b] = __builtin_fma(c, pr[b], acc[b]);
  }
}

// ------------------------------------------------------------------------------------------------ kernel rows
// thread = training point i (coalesced loads of z's rows and stores), workgroup = (256 points, test point t, NG rows)
template <int FAM, int D, int NG, bool PONE>
__global__ __launch_bounds__(kWG) void k_mt_rows(const double* __restrict__ xt, int64_t N, const void* __restrict__ z,
                                                 int64_t n, int P, MtPairTab tab, int tbits,
                                                 const double* __restrict__ hyp, int Gk, double* __restrict__ rows) {
  __shared__ double xs[D], hs[NG * (1 + D)];
  const int64_t t = blockIdx.y;
  const int g0 = blockIdx.z * NG;
  MtPoint<FAM, D> x;
  x.stage(xs, xt + t * D, tbits);
  MtHyp<D, NG> h;
  h.stage(hs, hyp, g0, Gk);
  __syncthreads();
  x.take(xs);
  h.take();
  const int64_t i = (int64_t)blockIdx.x * kWG + threadIdx.x;
  if (i >= n) return;
  double acc[NG];
  mt_pair<FAM, D, NG, PONE>(tab, P, tbits, x, h, z, n, i, acc);
#pragma unroll
  for (int b = 0; b < NG; ++b)
    if (g0 + b < Gk) rows[((int64_t)(g0 + b) * N + t) * n + i] = h.sc(b) * acc[b];
}

// zip: thread = pair t, rows[g][t] = K(xt_t, z_t); workgroup = (256 pairs, NG rows); the test point is the thread's own
template <int FAM, int D, int NG>
__global__ __launch_bounds__(kWG) void k_mt_rows_zip(const double* __restrict__ xt, int64_t N,
                                                     const void* __restrict__ z, int P, MtPairTab tab, int tbits,
                                                     const double* __restrict__ hyp, int Gk, double* __restrict__ rows) {
  __shared__ double hs[NG * (1 + D)];
  const int g0 = blockIdx.y * NG;
  MtHyp<D, NG> h;
  h.stage(hs, hyp, g0, Gk);
  __syncthreads();
  h.take();
  const int64_t t = (int64_t)blockIdx.x * kWG + threadIdx.x;
  if (t >= N) return;
  MtPoint<FAM, D> x;
  x.load(xt + t * D, tbits);
  double acc[NG];
  mt_pair<FAM, D, NG, false>(tab, P, tbits, x, h, z, N, t, acc);
#pragma unroll
  for (int b = 0; b < NG; ++b)
    if (g0 + b < Gk) rows[(int64_t)(g0 + b) * N + t] = h.sc(b) * acc[b];
}

// ------------------------------------------------------------------------------------------------ posterior mean
// k_wmt_post_mean's summation contract: workgroup = (chunk c, test point t, NB output rows); a thread adds every 256th
// point of its chunk in ascending i by sum = fma(scale K, c_i, sum) -- scale K is the value k_mt_rows stores --, then
// block_sum.  NK kernel rows per workgroup: 1 when every output row shares the hyper-parameters (Gk == 1), else NB.  A
// row past B repeats row B - 1 and is not stored.  The chunk bounds depend on n and the chunk length alone.
template <int FAM, int D, int NK, int NB, bool PONE>
__global__ __launch_bounds__(kWG) void k_mt_post_mean(const double* __restrict__ xt, int64_t N,
                                                      const void* __restrict__ z, int64_t n, int P, MtPairTab tab,
                                                      int tbits, const double* __restrict__ hyp, int Gk,
                                                      const double* __restrict__ coeffs, int64_t cstride, int B,
                                                      int64_t chunk, int64_t nchunks, double* __restrict__ partial) {
  static_assert(NK == 1 || NK == NB, "one kernel row for all output rows, or one each");
  __shared__ double red[kWG / 64];
  __shared__ double xs[D], hs[NK * (1 + D)];
  const int tid = threadIdx.x;
  const int64_t t = blockIdx.y;
  const int b0 = blockIdx.z * NB;
  MtPoint<FAM, D> x;
  x.stage(xs, xt + t * D, tbits);
  MtHyp<D, NK> h;
  h.stage(hs, hyp, NK == 1 ? 0 : b0, Gk);
  __syncthreads();
  x.take(xs);
  h.take();
  double sum[NB], sc[NK];
#pragma unroll
  for (int k = 0; k < NK; ++k) sc[k] = h.sc(k);
  // where thread 0 stores row b's partial, or -1: formed here, in VGPRs, so that N, nchunks, B and the block indices
  // are not held in SGPRs across the loop for the epilogue alone
  int64_t po[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b)
    po[b] = (tid == 0 && b0 + b < B) ? ((int64_t)(b0 + b) * N + t) * nchunks + blockIdx.x : (int64_t)-1;
  const double* cb[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    sum[b] = 0.0;
    cb[b] = coeffs + (int64_t)(b0 + b < B ? b0 + b : B - 1) * cstride;
  }
  const int64_t i0 = (int64_t)blockIdx.x * chunk;
  const int64_t i1 = i0 + chunk < n ? i0 + chunk : n;
  for (int64_t i = i0 + tid; i < i1; i += kWG) {
    double acc[NK];
    // (pbase: 0 behind an empty asm, so the scalar loads of the tables stay inside this loop: hoisted above it they
    // are live beside everything else and overflow the scalar file at D >= 5)
    int pbase = 0;
    asm volatile("" : "+s"(pbase));
    mt_pair<FAM, D, NK, PONE>(tab, P, tbits, x, h, z, n, i, acc, pbase);
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const int k = NK == 1 ? 0 : b;
      sum[b] = __builtin_fma(sc[k] * acc[k], cb[b][i], sum[b]);
    }
  }
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const double v = block_sum(sum[b], red);
    if (po[b] >= 0) partial[po[b]] = v;
  }
}

// out[b][t] = beta out[b][t] + w[b] sum_c partial[b][t][c]: one workgroup per output, a lane over every kWG-th chunk in
// ascending order, then block_sum's fixed tree; w NULL: 1; beta 0 (out is not read) or 1
__global__ __launch_bounds__(kWG) void k_mt_post_mean_sum(const double* __restrict__ partial, int64_t nchunks, int64_t N,
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
static int np_dp_ok(const char* fn, int d, int P) {
  if (d < 1 || d > FGP_MAX_D)
    return set_error(kErrInvalid, "%s: d=%d outside 1..%d (d > %d: the fgp_wide_ entry point)", fn, d, FGP_MAX_D,
                     FGP_MAX_D);
  if (P < 1) return set_error(kErrInvalid, "%s: P=%d (at least 1 derivative multi-index pair)", fn, P);
  if (P > kNpP) return set_error(kErrUnsupported, "%s: P=%d above %d (the torch formulation covers more)", fn, P, kNpP);
  return kOk;
}

static int np_tables(const char* fn, int family, int d, int P, const int* order, const double* coef, const double* add,
                     const int* ind, const double* cc, int tbits, MtPairTab& tab) {
  if (family != FGP_FAMILY_LATTICE && family != FGP_FAMILY_NET) return set_error(kErrInvalid, "%s: bad family %d", fn, family);
  const bool net = family == FGP_FAMILY_NET;
  if (!order) return set_error(kErrInvalid, "%s: null pointer (order)", fn);
  if (!coef) return set_error(kErrInvalid, "%s: null pointer (coef)", fn);
  if (net && !add) return set_error(kErrInvalid, "%s: null pointer (add)", fn);
  if (!ind) return set_error(kErrInvalid, "%s: null pointer (ind)", fn);
  if (!cc) return set_error(kErrInvalid, "%s: null pointer (cc)", fn);
  if (net && (tbits < 1 || tbits > 63)) return set_error(kErrInvalid, "%s: tbits=%d outside 1..63", fn, tbits);
  std::memset(&tab, 0, sizeof(tab));
  for (int p = 0; p < kNpP; ++p)
    for (int j = 0; j < kNpD; ++j) {
      const int q = p * kNpD + j;
      if (p >= P || j >= d) {
        tab.code[q] = 1 | (1 << 8);     // (never read: a factor of exactly 1)
        continue;
      }
      const int o = order[p * d + j];
      if (o < 1 || o > (net ? 4 : 8))
        return set_error(kErrUnsupported, "%s: %s order[%d][%d]=%d outside 1..%d", fn, net ? "Walsh" : "Bernoulli", p, j, o,
                         net ? 4 : 8);
      const int one = ind[p * d + j];
      if (one != 0 && one != 1) return set_error(kErrInvalid, "%s: ind[%d][%d]=%d is not 0 or 1", fn, p, j, one);
      tab.code[q] = o | (one << 8);
      tab.coef[q] = coef[p * d + j];
      tab.add[q] = add ? add[p * d + j] : 0.0;
    }
  for (int p = 0; p < P; ++p) tab.cc[p] = cc[p];
  return kOk;
}

// the chunk of training points of fgp_mt_post_mean: 0 = the default, else a positive multiple of kWG
static int np_pm_sizes(const char* fn, int64_t N, int64_t n, int B, int64_t chunk, int64_t* chunk_out, int64_t* nchunks) {
  if (N < 0) return set_error(kErrInvalid, "%s: N=%lld is negative", fn, (long long)N);
  if (n < 1) return set_error(kErrInvalid, "%s: n=%lld (at least 1 training point)", fn, (long long)n);
  if (B < 1 || B > 65535) return set_error(kErrInvalid, "%s: B=%d outside 1..65535", fn, B);
  if (chunk < 0 || chunk % kWG != 0)
    return set_error(kErrInvalid, "%s: chunk=%lld is not 0 (default) or a positive multiple of %d", fn, (long long)chunk, kWG);
  const int64_t ch = chunk ? chunk : kNpChunk;
  const int64_t nc = (n - 1) / ch + 1;
  if (nc > 0x7fffffffll) return set_error(kErrUnsupported, "%s: n=%lld needs %lld chunks", fn, (long long)n, (long long)nc);
  *chunk_out = ch;
  *nchunks = nc;
  return kOk;
}

}  // namespace fgp

using namespace fgp;

extern "C" {

int fgp_mt_rows(int family, const double* xt, int64_t N, const void* z, int64_t n, int zip, int d, int P,
                const int* order, const double* coef, const double* add, const int* ind, const double* cc, int tbits,
                const double* hyp, int Gk, double* rows, void* stream) {
  static const char* fn = "fgp_mt_rows";
  int rc = np_dp_ok(fn, d, P);
  if (rc != kOk) return rc;
  if (N < 0) return set_error(kErrInvalid, "%s: N=%lld is negative", fn, (long long)N);
  if (n < 1) return set_error(kErrInvalid, "%s: n=%lld (at least 1 training point)", fn, (long long)n);
  if (Gk < 1 || Gk > 65535 * kNpG) return set_error(kErrInvalid, "%s: Gk=%d outside 1..%d", fn, Gk, 65535 * kNpG);
  if (!zip && N > kNpNt) return set_error(kErrInvalid, "%s: N=%lld above %lld test points a call", fn, (long long)N, (long long)kNpNt);
  if (zip && N != n) return set_error(kErrInvalid, "%s: zip needs N == n", fn);
  if (!xt) return set_error(kErrInvalid, "%s: null pointer (xt)", fn);
  if (!z) return set_error(kErrInvalid, "%s: null pointer (z)", fn);
  if (!hyp) return set_error(kErrInvalid, "%s: null pointer (hyp)", fn);
  if (!rows) return set_error(kErrInvalid, "%s: null pointer (rows)", fn);
  MtPairTab tab;
  rc = np_tables(fn, family, d, P, order, coef, add, ind, cc, tbits, tab);
  if (rc != kOk) return rc;
  if (N == 0) return kOk;
  const int64_t nb = ((zip ? N : n) + kWG - 1) / kWG;
  if (nb > 0x7fffffffll) return set_error(kErrUnsupported, "%s: n=%lld needs %lld workgroups", fn, (long long)n, (long long)nb);
  hipStream_t st = (hipStream_t)stream;
  const bool lat = family == FGP_FAMILY_LATTICE;
  const unsigned gb = Gk == 1 ? 1u : (unsigned)((Gk + kNpG - 1) / kNpG);
  rc = dispatch_range<1, FGP_MAX_D>(d, [&](auto dc) {
    constexpr int D = decltype(dc)::value;
    if (zip) {
      const dim3 grid((unsigned)nb, gb);
#define FGP_NP_ZIP(FAM, NG) k_mt_rows_zip<FAM, D, NG><<<grid, kWG, 0, st>>>(xt, N, z, P, tab, tbits, hyp, Gk, rows)
      if (lat && Gk == 1) FGP_NP_ZIP(0, 1);
      else if (lat) FGP_NP_ZIP(0, kNpG);
      else if (Gk == 1) FGP_NP_ZIP(1, 1);
      else FGP_NP_ZIP(1, kNpG);
#undef FGP_NP_ZIP
      return check_launch("k_mt_rows_zip");
    }
    const dim3 grid((unsigned)nb, (unsigned)N, gb);
#define FGP_NP_ROWS(FAM, NG, PONE) \
  k_mt_rows<FAM, D, NG, PONE><<<grid, kWG, 0, st>>>(xt, N, z, n, P, tab, tbits, hyp, Gk, rows)
#define FGP_NP_ROWS_P(FAM, NG)          \
  do {                                  \
    if (P == 1) FGP_NP_ROWS(FAM, NG, true); \
    else FGP_NP_ROWS(FAM, NG, false);   \
  } while (0)
    if (lat && Gk == 1) FGP_NP_ROWS_P(0, 1);
    else if (lat) FGP_NP_ROWS_P(0, kNpG);
    else if (Gk == 1) FGP_NP_ROWS_P(1, 1);
    else FGP_NP_ROWS_P(1, kNpG);
#undef FGP_NP_ROWS_P
#undef FGP_NP_ROWS
    return check_launch("k_mt_rows");
  });
  return rc == kNoMatch ? no_kernel(rc, fn, d) : rc;
}

int fgp_mt_post_mean_work(int64_t N, int64_t n, int B, int64_t chunk, int64_t* len) {
  static const char* fn = "fgp_mt_post_mean_work";
  int64_t ch = 0, nc = 0;
  int rc = np_pm_sizes(fn, N, n, B, chunk, &ch, &nc);
  if (rc != kOk) return rc;
  if (!len) return set_error(kErrInvalid, "%s: null pointer (len)", fn);
  *len = std::max<int64_t>(1, (int64_t)B * std::min<int64_t>(N, kNpNt) * nc);
  return kOk;
}

int fgp_mt_post_mean(int family, const double* xt, int64_t N, const void* z, int64_t n, int d, int P, const int* order,
                     const double* coef, const double* add, const int* ind, const double* cc, int tbits,
                     const double* hyp, int Gk, const double* coeffs, int64_t coeff_stride, int B, const double* w,
                     int beta, double* out, int64_t out_stride, double* work, int64_t chunk, void* stream) {
  static const char* fn = "fgp_mt_post_mean";
  int rc = np_dp_ok(fn, d, P);
  if (rc != kOk) return rc;
  int64_t ch = 0, nchunks = 0;
  rc = np_pm_sizes(fn, N, n, B, chunk, &ch, &nchunks);
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
  MtPairTab tab;
  rc = np_tables(fn, family, d, P, order, coef, add, ind, cc, tbits, tab);
  if (rc != kOk) return rc;
  if (N == 0) return kOk;
  hipStream_t st = (hipStream_t)stream;
  const bool lat = family == FGP_FAMILY_LATTICE;
  const unsigned gz = B == 1 ? 1u : (unsigned)((B + kNpG - 1) / kNpG);
  rc = dispatch_range<1, FGP_MAX_D>(d, [&](auto dc) {
    constexpr int D = decltype(dc)::value;
    // the test points in launches of at most kNpNt: a point's chunks and their order do not depend on the split
    for (int64_t t0 = 0; t0 < N; t0 += kNpNt) {
      const int64_t Nc = std::min<int64_t>(kNpNt, N - t0);
      const dim3 grid((unsigned)nchunks, (unsigned)Nc, gz);
#define FGP_NP_PM(FAM, NK, NB, PONE)                                                                                      \
  k_mt_post_mean<FAM, D, NK, NB, PONE><<<grid, kWG, 0, st>>>(xt + t0 * D, Nc, z, n, P, tab, tbits, hyp, Gk, coeffs,      \
                                                              coeff_stride, B, ch, nchunks, work)
#define FGP_NP_PM_P(FAM, NK, NB)               \
  do {                                         \
    if (P == 1) FGP_NP_PM(FAM, NK, NB, true);  \
    else FGP_NP_PM(FAM, NK, NB, false);        \
  } while (0)
      if (lat) {
        if (B == 1) FGP_NP_PM_P(0, 1, 1);
        else if (Gk == 1) FGP_NP_PM_P(0, 1, kNpG);
        else FGP_NP_PM_P(0, kNpG, kNpG);
      } else {
        if (B == 1) FGP_NP_PM_P(1, 1, 1);
        else if (Gk == 1) FGP_NP_PM_P(1, 1, kNpG);
        else FGP_NP_PM_P(1, kNpG, kNpG);
      }
#undef FGP_NP_PM_P
#undef FGP_NP_PM
      int r = check_launch("k_mt_post_mean");
      if (r != kOk) return r;
      k_mt_post_mean_sum<<<dim3((unsigned)Nc, (unsigned)B), kWG, 0, st>>>(work, nchunks, Nc, w, beta, out + t0, out_stride);
      r = check_launch("k_mt_post_mean_sum");
      if (r != kOk) return r;
    }
    return (int)kOk;
  });
  return rc == kNoMatch ? no_kernel(rc, fn, d) : rc;
}

}  // extern "C"
