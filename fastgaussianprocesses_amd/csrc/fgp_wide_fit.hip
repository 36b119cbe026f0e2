// Wide inputs (9 <= d <= 64): the device-resident MLL fit loop, fgp_wide_fit_run (include/fgp_hip.h, an addition to
// ABI 20) -- AbstractGP.fit's iteration (abstract_gp.py:241-296: loss, loss.backward(), torch.optim.Rprop.step()) for G
// independent eigen-problems as a fixed sequence of plain launches on the caller's stream:
//
//   k1        fgp_wide_k1                       k1 = scale prod_j (1 + l_j part_j)            (fgp_wide.hip)
//   lambda    fgp_fftbr / fgp_fftbr_real / fgp_fwht (stable: AbstractFastGP.ft)               (fgp_transforms.hip)
//   terms     k_wide_fit_eig  (new)             norm / logdet / d noise partials, g~ = dL/dlambda in place of lambda
//   u         fgp_ifftbr (real part) / fgp_ifftbr_real / fgp_fwht: the adjoint transform of g~
//   gradient  fgp_wide_k1_bwd                   dL/dscale, dL/dl_j                            (fgp_wide.hip)
//   step      k_wide_fit_step (new)             two-level sums, loss, histories, chain rule to the raw parameters,
//                                               Rprop (rprop_update, fgp_nll.h), the natural rows of the next k1
//
// fgp_wide_fit_desc.loss_metric GCV / CV (AbstractGP.fit's alternative losses, abstract_gp.py:242-273; the closed forms
// above loss_terms in fgp_spectral.hip): g~ needs the global sums N1 and T, so `terms` becomes two passes over lambda
// and Y -- k_wide_fit_loss_sums (the partials, lambda left in place) and k_wide_fit_loss_grad (g~ over lambda) -- ten
// launches per iteration instead of nine; the MLL sequence is untouched.
//
// No host synchronisation, no device-to-host copy, no atomics, no inter-workgroup hand-off: every kernel reads what
// the launch before it wrote.  The lattice lambda of a real even k1 is real up to rounding; its real part is taken
// (Re(1/ev) and log|ev| differ from the complex forms by O((Im/Re)^2), below one rounding), so g~ is real and its
// adjoint is Re ifftbr(g~).  Problem g's sums run over its own partials in its own order: its results do not depend
// on G or on the other problems of the launch.  No per-thread array is indexed by a run-time dimension.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "fgp_common.h"
#include "fgp_nll.h"
#include "fgp_runtime.h"
#include "../../include/fgp_hip.h"

namespace fgp {

constexpr int kWfV = 4;                         // 16-byte groups of Y (2 frequencies each) in flight per lane
constexpr int kWfBlock = kWG * 2 * kWfV;        // frequencies per k_wide_fit_eig workgroup (2048)

// ------------------------------------------------------------------------------------------------
// Eigenvalue terms of problem g = blockIdx.y over frequencies [blockIdx.x kWfBlock, +kWfBlock): with
// ev_k = sqrt(n) Re(lambda_k) + noise, r = 1 / ev_k and t_k = (w - Y_k r) r = -Y_k / ev_k^2 + w / ev_k,
//   partial[g][0][blk] = sum Y_k r          (norm term)
//   partial[g][1][blk] = sum log|ev_k|      (logdet term)
//   partial[g][2][blk] = sum t_k            (2 dL/dnoise)
//   lam[g][k]          = 1/2 sqrt(n) t_k    (g~_k = dL/dlambda_k, written over lambda_k; lattice: (g~_k, 0))
// A memory stream with a divide and a log per element: a lane issues its kWfV 16-byte loads of Y and the 1 (net) or 2
// (lattice: one complex element each) 16-byte loads of lambda per group before the arithmetic.  FAM 0: lam is
// complex128, FAM 1: float64.  n is a power of two: a lane's pair (k, k + 1) is inside the row or, at n = 1, only k.
template <int FAM>
__global__ __launch_bounds__(kWG) void k_wide_fit_eig(double* __restrict__ lam, const double* __restrict__ ysq,
                                                      const double* __restrict__ raw_noise, int64_t n, double sqrtn,
                                                      double w, int nbe, double* __restrict__ partial) {
  __shared__ double red[kWG / 64];
  const int tid = threadIdx.x;
  const int g = blockIdx.y;
  const double noise = exp(raw_noise[g]);
  const double* yrow = ysq + (int64_t)g * n;
  double* lrow = lam + (int64_t)g * n * (FAM == 0 ? 2 : 1);
  const int64_t base = (int64_t)blockIdx.x * kWfBlock + 2 * tid;
  double y0[kWfV], y1[kWfV], l0[kWfV], l1[kWfV];
#pragma unroll
  for (int v = 0; v < kWfV; ++v) {
    const int64_t k = base + (int64_t)v * 2 * kWG;
    y0[v] = y1[v] = 0.0;
    l0[v] = l1[v] = 0.0;
    if (k + 1 < n) {
      const double2 yy = *reinterpret_cast<const double2*>(yrow + k);
      y0[v] = yy.x;
      y1[v] = yy.y;
      if constexpr (FAM == 0) {
        const double2 a = *reinterpret_cast<const double2*>(lrow + 2 * k);
        const double2 b = *reinterpret_cast<const double2*>(lrow + 2 * k + 2);
        l0[v] = a.x;
        l1[v] = b.x;
      } else {
        const double2 a = *reinterpret_cast<const double2*>(lrow + k);
        l0[v] = a.x;
        l1[v] = a.y;
      }
    } else if (k < n) {
      y0[v] = yrow[k];
      l0[v] = lrow[FAM == 0 ? 2 * k : k];
    }
  }
  double s_norm = 0.0, s_logdet = 0.0, s_noise = 0.0;
  const double hs = 0.5 * sqrtn;
#pragma unroll
  for (int v = 0; v < kWfV; ++v) {
    const int64_t k = base + (int64_t)v * 2 * kWG;
    if (k >= n) continue;
    const bool pair = k + 1 < n;
    const double ev0 = sqrtn * l0[v] + noise;
    const double r0 = 1.0 / ev0;
    const double t0 = (w - y0[v] * r0) * r0;
    s_norm += y0[v] * r0;
    s_logdet += log(fabs(ev0));
    s_noise += t0;
    double t1 = 0.0;
    if (pair) {
      const double ev1 = sqrtn * l1[v] + noise;
      const double r1 = 1.0 / ev1;
      t1 = (w - y1[v] * r1) * r1;
      s_norm += y1[v] * r1;
      s_logdet += log(fabs(ev1));
      s_noise += t1;
    }
    if constexpr (FAM == 0) {
      *reinterpret_cast<double2*>(lrow + 2 * k) = make_double2(hs * t0, 0.0);
      if (pair) *reinterpret_cast<double2*>(lrow + 2 * k + 2) = make_double2(hs * t1, 0.0);
    } else {
      if (pair) *reinterpret_cast<double2*>(lrow + k) = make_double2(hs * t0, hs * t1);
      else lrow[k] = hs * t0;
    }
  }
  s_norm = block_sum(s_norm, red);
  s_logdet = block_sum(s_logdet, red);
  s_noise = block_sum(s_noise, red);
  if (tid == 0) {
    double* pg = partial + (int64_t)g * 3 * nbe + blockIdx.x;
    pg[0] = s_norm;
    pg[(int64_t)nbe] = s_logdet;
    pg[2 * (int64_t)nbe] = s_noise;
  }
}

// ------------------------------------------------------------------------------------------------
// GCV / CV.  With ev_k = sqrt(n) Re(lambda_k) + noise, lambda'_k = sqrt(n) Re(lambda_k), r = 1 / ev_k:
//   N1 = sum Y_k r^2,  S1 = sum Y_k r^3,  GCV: T = sum r, S2 = sum r^2;  CV: T = sum 1 / lambda'_k
//   GCV: D = (T / n)^2, loss = N1 / D, c1 = -2 / D, c2 = 2 N1 T / (n^2 D^2), w2_k = r^2
//   CV:  I = T / n, loss = w N1 / I^2, c1 = -2 w / I^2, c2 = 2 w N1 / (n I^3), w2_k = 1 / lambda'_k^2
//   g~_k = dL/dlambda_k = sqrt(n) (c1 Y_k r^3 + c2 w2_k),  dL/dnoise = c1 S1 (+ c2 S2, GCV)
// Partials [G][4][nbe] = (N1, T, S1, S2); the CV loop leaves row 3 unwritten and unread.
constexpr int kWfLossQ = 4;

// A lane's kWfV groups of (Y_k, Y_k+1, Re lambda_k, Re lambda_k+1), zero past the row: k_wide_fit_eig's load pattern,
// every 16-byte load issued before the arithmetic.
template <int FAM>
__device__ __forceinline__ void wide_fit_load(const double* __restrict__ yrow, const double* __restrict__ lrow,
                                              int64_t base, int64_t n, double (&y0)[kWfV], double (&y1)[kWfV],
                                              double (&l0)[kWfV], double (&l1)[kWfV]) {
#pragma unroll
  for (int v = 0; v < kWfV; ++v) {
    const int64_t k = base + (int64_t)v * 2 * kWG;
    y0[v] = y1[v] = 0.0;
    l0[v] = l1[v] = 0.0;
    if (k + 1 < n) {
      const double2 yy = *reinterpret_cast<const double2*>(yrow + k);
      y0[v] = yy.x;
      y1[v] = yy.y;
      if constexpr (FAM == 0) {
        const double2 a = *reinterpret_cast<const double2*>(lrow + 2 * k);
        const double2 b = *reinterpret_cast<const double2*>(lrow + 2 * k + 2);
        l0[v] = a.x;
        l1[v] = b.x;
      } else {
        const double2 a = *reinterpret_cast<const double2*>(lrow + k);
        l0[v] = a.x;
        l1[v] = a.y;
      }
    } else if (k < n) {
      y0[v] = yrow[k];
      l0[v] = lrow[FAM == 0 ? 2 * k : k];
    }
  }
}

// Level 2 of a two-level sum: a lane over every kWG-th partial in ascending order, then block_sum's fixed tree (the
// order k_wide_fit_step's MLL sums use).  Every thread gets the total.
__device__ __forceinline__ double wide_fit_total(const double* __restrict__ pq, int nbe, double* red) {
  double a = 0.0;
  for (int c = threadIdx.x; c < nbe; c += kWG) a += pq[c];
  return block_sum(a, red);
}

// loss, c1, c2 and the history terms of one problem from its totals: ONE sequence of operations for
// k_wide_fit_loss_grad and k_wide_fit_step, whose coefficients are therefore the same bits.
struct WideLossCoef {
  double loss, c1, c2, t1, t2;
};

template <bool CV>
__device__ __forceinline__ WideLossCoef wide_loss_coef(double N1, double T, double n, double w) {
  WideLossCoef c;
  if constexpr (CV) {
    const double I = T / n, I2 = I * I;
    c.loss = w * N1 / I2;
    c.c1 = -2.0 * w / I2;
    c.c2 = 2.0 * w * N1 / (n * I2 * I);
    c.t1 = c.t2 = NAN;
  } else {
    const double q = T / n, D = q * q;
    c.loss = N1 / D;
    c.c1 = -2.0 / D;
    c.c2 = 2.0 * N1 * T / (n * n * D * D);
    c.t1 = N1;
    c.t2 = D;
  }
  return c;
}

// Pass 1 over frequencies [blockIdx.x kWfBlock, +kWfBlock) of problem g = blockIdx.y: the partials; lambda stays.
template <int FAM, bool CV>
__global__ __launch_bounds__(kWG) void k_wide_fit_loss_sums(const double* __restrict__ lam,
                                                            const double* __restrict__ ysq,
                                                            const double* __restrict__ raw_noise, int64_t n,
                                                            double sqrtn, int nbe, double* __restrict__ partial) {
  __shared__ double red[kWG / 64];
  const int tid = threadIdx.x;
  const int g = blockIdx.y;
  const double noise = exp(raw_noise[g]);
  const double* yrow = ysq + (int64_t)g * n;
  const double* lrow = lam + (int64_t)g * n * (FAM == 0 ? 2 : 1);
  const int64_t base = (int64_t)blockIdx.x * kWfBlock + 2 * tid;
  double y0[kWfV], y1[kWfV], l0[kWfV], l1[kWfV];
  wide_fit_load<FAM>(yrow, lrow, base, n, y0, y1, l0, l1);
  double s_n1 = 0.0, s_t = 0.0, s_1 = 0.0, s_2 = 0.0;
#pragma unroll
  for (int v = 0; v < kWfV; ++v) {
    const int64_t k = base + (int64_t)v * 2 * kWG;
    if (k >= n) continue;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      if (e == 1 && k + 1 >= n) continue;
      const double lp = sqrtn * (e ? l1[v] : l0[v]), Y = e ? y1[v] : y0[v];
      const double r = 1.0 / (lp + noise);
      const double r2 = r * r, yr2 = Y * r2;
      s_n1 += yr2;
      s_1 += yr2 * r;
      if constexpr (CV) {
        s_t += 1.0 / lp;
      } else {
        s_t += r;
        s_2 += r2;
      }
    }
  }
  s_n1 = block_sum(s_n1, red);
  s_t = block_sum(s_t, red);
  s_1 = block_sum(s_1, red);
  if constexpr (!CV) s_2 = block_sum(s_2, red);
  if (tid == 0) {
    double* pg = partial + (int64_t)g * kWfLossQ * nbe + blockIdx.x;
    pg[0] = s_n1;
    pg[(int64_t)nbe] = s_t;
    pg[2 * (int64_t)nbe] = s_1;
    if constexpr (!CV) pg[3 * (int64_t)nbe] = s_2;
  }
}

// Pass 2, same geometry: every workgroup re-sums its problem's N1 and T partials in k_wide_fit_step's order (no
// coefficient launch between the passes, no hand-off), forms c1 and c2 and writes g~ over lambda (lattice: (g~, 0)).
template <int FAM, bool CV>
__global__ __launch_bounds__(kWG) void k_wide_fit_loss_grad(double* __restrict__ lam, const double* __restrict__ ysq,
                                                            const double* __restrict__ raw_noise, int64_t n,
                                                            double sqrtn, double w, int nbe,
                                                            const double* __restrict__ partial) {
  __shared__ double red[kWG / 64];
  const int tid = threadIdx.x;
  const int g = blockIdx.y;
  const double noise = exp(raw_noise[g]);
  const double* yrow = ysq + (int64_t)g * n;
  double* lrow = lam + (int64_t)g * n * (FAM == 0 ? 2 : 1);
  const int64_t base = (int64_t)blockIdx.x * kWfBlock + 2 * tid;
  double y0[kWfV], y1[kWfV], l0[kWfV], l1[kWfV];
  wide_fit_load<FAM>(yrow, lrow, base, n, y0, y1, l0, l1);
  const double* pg = partial + (int64_t)g * kWfLossQ * nbe;
  const double N1 = wide_fit_total(pg, nbe, red);
  const double T = wide_fit_total(pg + nbe, nbe, red);
  const WideLossCoef c = wide_loss_coef<CV>(N1, T, (double)n, w);
#pragma unroll
  for (int v = 0; v < kWfV; ++v) {
    const int64_t k = base + (int64_t)v * 2 * kWG;
    if (k >= n) continue;
    const bool pair = k + 1 < n;
    double gt[2] = {0.0, 0.0};
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      if (e == 1 && !pair) continue;
      const double lp = sqrtn * (e ? l1[v] : l0[v]), Y = e ? y1[v] : y0[v];
      const double r = 1.0 / (lp + noise);
      const double r2 = r * r;
      double w2 = r2;
      if constexpr (CV) {
        const double rl = 1.0 / lp;
        w2 = rl * rl;
      }
      gt[e] = sqrtn * (c.c1 * (Y * r2 * r) + c.c2 * w2);
    }
    if constexpr (FAM == 0) {
      *reinterpret_cast<double2*>(lrow + 2 * k) = make_double2(gt[0], 0.0);
      if (pair) *reinterpret_cast<double2*>(lrow + 2 * k + 2) = make_double2(gt[1], 0.0);
    } else {
      if (pair) *reinterpret_cast<double2*>(lrow + k) = make_double2(gt[0], gt[1]);
      else lrow[k] = gt[0];
    }
  }
}

// ------------------------------------------------------------------------------------------------
// The step of problem g = blockIdx.x (one workgroup per problem).  raw = [G scales, G dl lengthscales, G noises].
//   mode 0  only the natural rows of the current raw parameters (before the first k1 of a run; init: a new fit's
//           Rprop state prev = 0, step = lr)
//   mode 1  sums, loss, history rows, gradient: the evaluation without an update
//   mode 2  the same, the Rprop step of the parameters that require a gradient, and the natural rows of the new ones
// Sums: level 1 = the per-workgroup partials of k_wide_fit_eig / k_wide_k1_bwd, level 2 here, a lane over every
// kWG-th partial in ascending order, then block_sum's fixed tree.
// LOSS = FGP_LOSS_GCV / FGP_LOSS_CV: pe is k_wide_fit_loss_sums' [G][4][nbe]; the history row is (loss, N1, D) /
// (loss, NaN, NaN) as k_spec_loss_step writes it, dL/dnoise = c1 S1 (+ c2 S2, GCV); mll_const and w are not used.
struct WideFitStep {
  Fit f;
  int G, d, dl, nbe;
  double w, lr;
  const double* pe;          // [G][3][nbe]; GCV / CV: [G][4][nbe]
  const double* dscale;      // [G]      dL/dscale
  const double* dls;         // [G][d]   dL/dl_j
  double* nat_scale;         // [G]
  double* nat_ls;            // [G][d]
};

struct WideFitLoss {
  double n, cv_weight;
};

template <int LOSS>
__global__ __launch_bounds__(kWG) void k_wide_fit_step(WideFitStep s, int iter, int mode, int init, WideFitLoss x) {
  __shared__ double red[kWG / 64];
  const int tid = threadIdx.x;
  const int g = blockIdx.x;
  const int G = s.G, d = s.d, dl = s.dl;
  const Fit& f = s.f;
  const int p_scale = g, p_ls = G + g * dl, p_noise = G + G * dl + g;
  if (mode != 0) {
    constexpr bool CV = LOSS == FGP_LOSS_CV;
    constexpr int NQ = LOSS == FGP_LOSS_MLL ? 3 : kWfLossQ;
    double sums[NQ];
    WideLossCoef lc{};
    if constexpr (LOSS == FGP_LOSS_MLL) {
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const double* pq = s.pe + ((int64_t)g * 3 + q) * s.nbe;
        double a = 0.0;
        for (int c = tid; c < s.nbe; c += kWG) a += pq[c];
        sums[q] = block_sum(a, red);
      }
    } else {
      sums[3] = 0.0;
#pragma unroll
      for (int q = 0; q < (CV ? 3 : 4); ++q) sums[q] = wide_fit_total(s.pe + ((int64_t)g * NQ + q) * s.nbe, s.nbe, red);
      lc = wide_loss_coef<CV>(sums[0], sums[1], x.n, x.cv_weight);
    }
    if (tid < 2 + dl) {
      int p, rg;
      double nat, gnat;
      if (tid == 0) {
        p = p_scale;
        rg = f.scale_rg;
        nat = s.nat_scale[g];
        gnat = s.dscale[g];
      } else if (tid <= dl) {
        const int j = tid - 1;
        p = p_ls + j;
        rg = f.ls_rg;
        nat = s.nat_ls[(int64_t)g * d + j];
        if (dl == d) {
          gnat = s.dls[(int64_t)g * d + j];
        } else {                               // one lengthscale for every dimension: the sum over j, ascending
          gnat = 0.0;
          for (int jj = 0; jj < d; ++jj) gnat += s.dls[(int64_t)g * d + jj];
        }
      } else {
        p = p_noise;
        rg = f.noise_rg;
        nat = exp(f.raw[p]);
        if constexpr (LOSS == FGP_LOSS_MLL) gnat = 0.5 * sums[2];
        else if constexpr (CV) gnat = lc.c1 * sums[2];
        else gnat = lc.c1 * sums[2] + lc.c2 * sums[3];
      }
      const double graw = nat * gnat;          // exp transforms: d nat / d raw = nat
      f.raw_hist[(int64_t)iter * f.n_params + p] = f.raw[p];
      f.grad_out[p] = graw;
      if (mode == 2 && rg) rprop_update(f, p, graw);
    }
    if (tid == 0) {
      double* lh = f.loss_hist + ((int64_t)iter * G + g) * 3;
      if constexpr (LOSS == FGP_LOSS_MLL) {
        const double t2 = s.w * sums[1];
        lh[0] = 0.5 * (sums[0] + t2) + f.mll_const;
        lh[1] = sums[0];
        lh[2] = t2;
      } else {
        lh[0] = lc.loss;
        lh[1] = lc.t1;
        lh[2] = lc.t2;
      }
    }
    if (mode != 2) return;
    __syncthreads();
  } else if (init && tid < 2 + dl) {
    const int p = tid == 0 ? p_scale : (tid <= dl ? p_ls + tid - 1 : p_noise);
    f.prev[p] = 0.0;
    f.step[p] = s.lr;
  }
  if (tid == 0) s.nat_scale[g] = exp(f.raw[p_scale]);
  for (int j = tid; j < d; j += kWG) s.nat_ls[(int64_t)g * d + j] = exp(f.raw[p_ls + (dl == d ? j : 0)]);
}

// ------------------------------------------------------------------------------------------------ host side
struct WideFitPlan {
  int64_t n;
  int nbe;                                       // k_wide_fit_eig workgroups per problem
  bool lat, r2c;
  int64_t o_scale, o_ls, o_dscale, o_dls, o_a, o_b, o_w, o_pe, o_pb, o_pl, len;   // offsets into work, in doubles
};

static int64_t even(int64_t v) { return (v + 1) & ~(int64_t)1; }

static int wide_fit_plan(const char* fn, const fgp_wide_fit_desc* a, WideFitPlan& p) {
  if (!a) return set_error(kErrInvalid, "%s: null pointer: desc", fn);
  if (a->d <= FGP_MAX_D || a->d > FGP_WIDE_MAX_D)
    return set_error(kErrInvalid, "%s: d=%d outside %d..%d", fn, a->d, FGP_MAX_D + 1, FGP_WIDE_MAX_D);
  if (a->log2n < 0 || a->log2n > 24) return set_error(kErrInvalid, "%s: log2n=%d outside 0..24", fn, a->log2n);
  if (a->G < 1 || a->G > 65535) return set_error(kErrInvalid, "%s: G=%d outside 1..65535", fn, a->G);
  if (a->dl != 1 && a->dl != a->d) return set_error(kErrInvalid, "%s: dl=%d not in {1, d=%d}", fn, a->dl, a->d);
  if (a->family != FGP_FAMILY_LATTICE && a->family != FGP_FAMILY_NET)
    return set_error(kErrInvalid, "%s: bad family %d", fn, a->family);
  p.n = (int64_t)1 << a->log2n;
  if (a->parts_stride != 0 && a->parts_stride != (int64_t)a->d * p.n)
    return set_error(kErrInvalid, "%s: parts_stride=%lld is neither 0 nor d n", fn, (long long)a->parts_stride);
  if ((int64_t)a->G * (2 + a->dl) > (int64_t)1 << 30) return set_error(kErrInvalid, "%s: G=%d too large", fn, a->G);
  if (a->loss_metric != FGP_LOSS_MLL && a->loss_metric != FGP_LOSS_GCV && a->loss_metric != FGP_LOSS_CV)
    return set_error(kErrInvalid, "%s: loss_metric=%d not FGP_LOSS_MLL / _GCV / _CV", fn, a->loss_metric);
  if (a->loss_metric == FGP_LOSS_CV && !std::isfinite(a->cv_weight))
    return set_error(kErrInvalid, "%s: cv_weight is not finite", fn);
  p.lat = a->family == FGP_FAMILY_LATTICE;
  p.r2c = use_r2c(read_switches(), p.lat, a->log2n);
  p.nbe = (int)((p.n + kWfBlock - 1) / kWfBlock);
  const int64_t G = a->G, d = a->d, n = p.n;
  int64_t o = 0;
  p.o_scale = o, o += even(G);
  p.o_ls = o, o += even(G * d);
  p.o_dscale = o, o += even(G);
  p.o_dls = o, o += even(G * d);
  p.o_a = o, o += even(G * n);                          // k1, then u = dL/dk1
  p.o_b = o, o += even(G * n * (p.lat ? 2 : 1));        // lambda, then g~
  p.o_w = o, o += p.lat ? 2 * G * n : 0;                // the lattice transforms' scratch
  p.o_pe = o, o += even(G * 3 * p.nbe);
  p.o_pb = o, o += even(G * (1 + d) * ((n + kWG - 1) / kWG));
  // GCV / CV: k_wide_fit_loss_sums' partials, after everything the MLL lays out (whose length stays as it was)
  p.o_pl = o, o += a->loss_metric == FGP_LOSS_MLL ? 0 : even(G * kWfLossQ * p.nbe);
  p.len = o;
  return kOk;
}

// The two GCV / CV passes of one iteration over lambda (B) and Y, one launch each.
static int wide_fit_loss_sums(bool lat, bool cv, dim3 grid, const double* B, const double* ysq, const double* raw_noise,
                              int64_t n, double sqrtn, int nbe, double* pe, hipStream_t st) {
  if (lat) {
    if (cv) k_wide_fit_loss_sums<0, true><<<grid, kWG, 0, st>>>(B, ysq, raw_noise, n, sqrtn, nbe, pe);
    else k_wide_fit_loss_sums<0, false><<<grid, kWG, 0, st>>>(B, ysq, raw_noise, n, sqrtn, nbe, pe);
  } else {
    if (cv) k_wide_fit_loss_sums<1, true><<<grid, kWG, 0, st>>>(B, ysq, raw_noise, n, sqrtn, nbe, pe);
    else k_wide_fit_loss_sums<1, false><<<grid, kWG, 0, st>>>(B, ysq, raw_noise, n, sqrtn, nbe, pe);
  }
  return check_launch("k_wide_fit_loss_sums");
}

static int wide_fit_loss_grad(bool lat, bool cv, dim3 grid, double* B, const double* ysq, const double* raw_noise,
                              int64_t n, double sqrtn, double w, int nbe, const double* pe, hipStream_t st) {
  if (lat) {
    if (cv) k_wide_fit_loss_grad<0, true><<<grid, kWG, 0, st>>>(B, ysq, raw_noise, n, sqrtn, w, nbe, pe);
    else k_wide_fit_loss_grad<0, false><<<grid, kWG, 0, st>>>(B, ysq, raw_noise, n, sqrtn, w, nbe, pe);
  } else {
    if (cv) k_wide_fit_loss_grad<1, true><<<grid, kWG, 0, st>>>(B, ysq, raw_noise, n, sqrtn, w, nbe, pe);
    else k_wide_fit_loss_grad<1, false><<<grid, kWG, 0, st>>>(B, ysq, raw_noise, n, sqrtn, w, nbe, pe);
  }
  return check_launch("k_wide_fit_loss_grad");
}

// One iteration as stages, in the order wide_fit_run enqueues them.  fgp_wide_fit_stage (a test hook) enqueues one of
// them; wide_fit_run is the loop over the same function, so the run and the staged sequence are one piece of code.
enum WideFitStage {
  kWfsPrologue = 0,   // k_wide_fit_step in mode 0; the stage's mode is its init flag
  kWfsK1,             // fgp_wide_k1 (per problem when every problem has its own parts)
  kWfsForward,        // lambda = ft(k1)
  kWfsTerms,          // k_wide_fit_eig; GCV / CV: k_wide_fit_loss_sums
  kWfsTerms2,         // GCV / CV only: k_wide_fit_loss_grad
  kWfsAdjoint,        // u = the adjoint transform of g~
  kWfsK1Bwd,          // fgp_wide_k1_bwd
  kWfsStep,           // k_wide_fit_step in mode 1 or 2
  kWfsCount
};

// what every stage needs of the desc and the plan, formed once per run
struct WideFitCtx {
  const fgp_wide_fit_desc* a;
  const WideFitPlan* p;
  WideFitStep s;
  WideFitLoss x;
  double *nat_scale, *nat_ls, *dscale, *dls, *A, *B, *W, *pe, *pb;
  const double* raw_noise;
  double sqrtn;
};

static WideFitCtx wide_fit_ctx(const fgp_wide_fit_desc* a, const WideFitPlan& p) {
  WideFitCtx c{};
  c.a = a, c.p = &p;
  const int G = a->G, d = a->d;
  double* work = static_cast<double*>(a->work);
  c.nat_scale = work + p.o_scale, c.nat_ls = work + p.o_ls, c.dscale = work + p.o_dscale, c.dls = work + p.o_dls;
  c.A = work + p.o_a, c.B = work + p.o_b, c.W = work + p.o_w, c.pe = work + p.o_pe, c.pb = work + p.o_pb;
  WideFitStep& s = c.s;
  s.f.n_params = G * (2 + a->dl);
  s.f.raw = a->raw;
  s.f.prev = a->rprop_prev;
  s.f.step = a->rprop_step;
  s.f.grad_out = a->grad_out;
  s.f.loss_hist = a->loss_hist;
  s.f.raw_hist = a->raw_hist;
  s.f.scale_rg = a->scale_rg, s.f.ls_rg = a->ls_rg, s.f.noise_rg = a->noise_rg;
  s.f.mll_const = a->mll_const;
  s.f.eta_minus = a->eta_minus, s.f.eta_plus = a->eta_plus, s.f.step_min = a->step_min, s.f.step_max = a->step_max;
  s.G = G, s.d = d, s.dl = a->dl, s.nbe = p.nbe;
  s.w = a->logdet_weight, s.lr = a->lr;
  if (a->loss_metric != FGP_LOSS_MLL) c.pe = work + p.o_pl;
  s.pe = c.pe, s.dscale = c.dscale, s.dls = c.dls, s.nat_scale = c.nat_scale, s.nat_ls = c.nat_ls;
  c.raw_noise = a->raw + (int64_t)G * (1 + a->dl);
  c.sqrtn = std::sqrt((double)p.n);
  c.x = WideFitLoss{(double)p.n, a->cv_weight};
  return c;
}

static int wide_fit_step_launch(const WideFitCtx& c, int iter, int mode, int init, hipStream_t st) {
  const int loss = c.a->loss_metric, G = c.a->G;
  if (loss == FGP_LOSS_MLL) k_wide_fit_step<FGP_LOSS_MLL><<<G, kWG, 0, st>>>(c.s, iter, mode, init, c.x);
  else if (loss == FGP_LOSS_GCV) k_wide_fit_step<FGP_LOSS_GCV><<<G, kWG, 0, st>>>(c.s, iter, mode, init, c.x);
  else k_wide_fit_step<FGP_LOSS_CV><<<G, kWG, 0, st>>>(c.s, iter, mode, init, c.x);
  return check_launch("k_wide_fit_step");
}

// Stage `stage` of iteration `iter` (the history row the step writes).  mode: the prologue's init flag, the step's mode
// (1 or 2), otherwise unused.  The caller has validated stage and mode.
static int wide_fit_stage(const WideFitCtx& c, int iter, int stage, int mode, hipStream_t st) {
  const fgp_wide_fit_desc* a = c.a;
  const WideFitPlan& p = *c.p;
  const int G = a->G, d = a->d, m = a->log2n, loss = a->loss_metric;
  const int64_t n = p.n;
  const dim3 grid((unsigned)p.nbe, (unsigned)G);
  int rc = kOk;
  switch (stage) {
    case kWfsPrologue:
      return wide_fit_step_launch(c, 0, 0, mode, st);
    case kWfsK1:
      // per problem when every problem has its own parts: fgp_wide_k1 takes ONE parts array
      if (a->parts_stride == 0) return fgp_wide_k1(a->parts, n, d, c.nat_scale, c.nat_ls, G, c.A, st);
      for (int g = 0; g < G && rc == kOk; ++g)
        rc = fgp_wide_k1(a->parts + g * a->parts_stride, n, d, c.nat_scale + g, c.nat_ls + (int64_t)g * d, 1, c.A + g * n,
                         st);
      return rc;
    case kWfsForward:
      // lambda = ft(k1), stable (AbstractFastGP.ft)
      if (!p.lat) return fgp_fwht(c.A, n, c.B, G, m, 1, st);
      if (p.r2c) return fgp_fftbr_real(c.A, n, c.B, c.W, G, m, st);
      return fgp_fftbr(c.A, n, 1, c.B, G, m, 1, st);
    case kWfsTerms:
      if (loss == FGP_LOSS_MLL) {
        if (p.lat)
          k_wide_fit_eig<0><<<grid, kWG, 0, st>>>(c.B, a->ysq, c.raw_noise, n, c.sqrtn, a->logdet_weight, p.nbe, c.pe);
        else
          k_wide_fit_eig<1><<<grid, kWG, 0, st>>>(c.B, a->ysq, c.raw_noise, n, c.sqrtn, a->logdet_weight, p.nbe, c.pe);
        return check_launch("k_wide_fit_eig");
      }
      return wide_fit_loss_sums(p.lat, loss == FGP_LOSS_CV, grid, c.B, a->ysq, c.raw_noise, n, c.sqrtn, p.nbe, c.pe, st);
    case kWfsTerms2:
      return wide_fit_loss_grad(p.lat, loss == FGP_LOSS_CV, grid, c.B, a->ysq, c.raw_noise, n, c.sqrtn, a->cv_weight,
                                p.nbe, c.pe, st);
    case kWfsAdjoint:
      // u = dL/dk1: the adjoint transform of g~ (lattice: the real part)
      if (!p.lat) return fgp_fwht(c.B, n, c.A, G, m, 1, st);
      if (p.r2c) return fgp_ifftbr_real(c.B, n, nullptr, 0, c.A, n, c.W, G, m, st);
      return fgp_ifftbr(c.B, n, c.A, 1, c.W, G, m, 1, st);
    case kWfsK1Bwd:
      if (a->parts_stride == 0)
        return fgp_wide_k1_bwd(a->parts, n, d, c.nat_scale, c.nat_ls, G, c.A, c.dscale, c.dls, c.pb, st);
      for (int g = 0; g < G && rc == kOk; ++g)
        rc = fgp_wide_k1_bwd(a->parts + g * a->parts_stride, n, d, c.nat_scale + g, c.nat_ls + (int64_t)g * d, 1,
                             c.A + g * n, c.dscale + g, c.dls + (int64_t)g * d, c.pb, st);
      return rc;
    default:
      return wide_fit_step_launch(c, iter, mode, 0, st);
  }
}

static int wide_fit_run(const fgp_wide_fit_desc* a, const WideFitPlan& p, int iter0, int iters, int final_no_update,
                        hipStream_t st) {
  const WideFitCtx c = wide_fit_ctx(a, p);
  int rc = wide_fit_stage(c, 0, kWfsPrologue, iter0 == 0 && a->lr > 0.0, st);
  for (int it = 0; it < iters && rc == kOk; ++it) {
    const bool last = it + 1 == iters;
    for (int stage = kWfsK1; stage < kWfsCount && rc == kOk; ++stage) {
      if (stage == kWfsTerms2 && a->loss_metric == FGP_LOSS_MLL) continue;
      rc = wide_fit_stage(c, iter0 + it, stage, stage == kWfsStep ? ((last && final_no_update) ? 1 : 2) : 0, st);
    }
  }
  return rc;
}

// what fgp_wide_fit_run and fgp_wide_fit_stage validate beyond the plan: the pointers, then (after the caller's own
// iteration arguments, the order fgp_wide_fit_run has always reported them in) the alignment
static int wide_fit_check_ptrs(const char* fn, const fgp_wide_fit_desc* desc) {
  const struct {
    const void* ptr;
    const char* name;
  } ptrs[] = {{desc->parts, "parts"},           {desc->ysq, "ysq"},           {desc->raw, "raw"},
              {desc->rprop_prev, "rprop_prev"}, {desc->rprop_step, "rprop_step"}, {desc->loss_hist, "loss_hist"},
              {desc->raw_hist, "raw_hist"},     {desc->grad_out, "grad_out"}, {desc->work, "work"}};
  for (const auto& q : ptrs)
    if (!q.ptr) return set_error(kErrInvalid, "%s: null pointer: %s", fn, q.name);
  return kOk;
}

static int wide_fit_check_align(const char* fn, const fgp_wide_fit_desc* desc) {
  if (((uintptr_t)desc->ysq | (uintptr_t)desc->work) & 15)
    return set_error(kErrInvalid, "%s: ysq and work must be 16-byte aligned", fn);
  return kOk;
}

}  // namespace fgp

using namespace fgp;

extern "C" {

int fgp_wide_fit_work(const fgp_wide_fit_desc* desc, int64_t* len) {
  WideFitPlan p;
  int rc = wide_fit_plan("fgp_wide_fit_work", desc, p);
  if (rc != kOk) return rc;
  if (!len) return set_error(kErrInvalid, "fgp_wide_fit_work: null pointer: len");
  *len = p.len;
  return kOk;
}

int fgp_wide_fit_run(const fgp_wide_fit_desc* desc, int iter0, int iters, int final_no_update, void* stream) {
  WideFitPlan p;
  int rc = wide_fit_plan("fgp_wide_fit_run", desc, p);
  if (rc != kOk) return rc;
  rc = wide_fit_check_ptrs("fgp_wide_fit_run", desc);
  if (rc != kOk) return rc;
  if (iters < 0) return set_error(kErrInvalid, "fgp_wide_fit_run: iters=%d negative", iters);
  if (iter0 < 0) return set_error(kErrInvalid, "fgp_wide_fit_run: iter0=%d negative", iter0);
  rc = wide_fit_check_align("fgp_wide_fit_run", desc);
  if (rc != kOk) return rc;
  if (iters == 0) return kOk;
  return wide_fit_run(desc, p, iter0, iters, final_no_update, (hipStream_t)stream);
}

int fgp_wide_fit_work_layout(const fgp_wide_fit_desc* desc, int64_t offsets[10]) {
  WideFitPlan p;
  int rc = wide_fit_plan("fgp_wide_fit_work_layout", desc, p);
  if (rc != kOk) return rc;
  if (!offsets) return set_error(kErrInvalid, "fgp_wide_fit_work_layout: null pointer: offsets");
  const int64_t o[10] = {p.o_scale, p.o_ls, p.o_dscale, p.o_dls, p.o_a, p.o_b, p.o_w, p.o_pe, p.o_pb, p.o_pl};
  for (int i = 0; i < 10; ++i) offsets[i] = o[i];
  return kOk;
}

int fgp_wide_fit_stage(const fgp_wide_fit_desc* desc, int iter, int stage, int mode, void* stream) {
  static const char* fn = "fgp_wide_fit_stage";
  WideFitPlan p;
  int rc = wide_fit_plan(fn, desc, p);
  if (rc != kOk) return rc;
  rc = wide_fit_check_ptrs(fn, desc);
  if (rc != kOk) return rc;
  if (iter < 0) return set_error(kErrInvalid, "%s: iter=%d negative", fn, iter);
  rc = wide_fit_check_align(fn, desc);
  if (rc != kOk) return rc;
  if (stage < 0 || stage >= kWfsCount) return set_error(kErrInvalid, "%s: stage=%d outside 0..%d", fn, stage, kWfsCount - 1);
  if (stage == kWfsTerms2 && desc->loss_metric == FGP_LOSS_MLL)
    return set_error(kErrInvalid, "%s: stage=%d (the second terms pass) exists under GCV / CV only", fn, stage);
  if (stage == kWfsPrologue) {
    if (mode != 0 && mode != 1) return set_error(kErrInvalid, "%s: mode=%d of the prologue is not 0 or 1 (init)", fn, mode);
    if (mode == 1 && !(desc->lr > 0.0)) return set_error(kErrInvalid, "%s: mode=1 (init) needs lr > 0", fn);
  } else if (stage == kWfsStep) {
    if (mode != 1 && mode != 2) return set_error(kErrInvalid, "%s: mode=%d of the step is not 1 or 2", fn, mode);
  } else if (mode != 0) {
    return set_error(kErrInvalid, "%s: mode=%d of stage %d is not 0", fn, mode, stage);
  }
  const WideFitCtx c = wide_fit_ctx(desc, p);
  return wide_fit_stage(c, iter, stage, mode, (hipStream_t)stream);
}

}  // extern "C"
