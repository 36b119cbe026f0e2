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
// The step of problem g = blockIdx.x (one workgroup per problem).  raw = [G scales, G dl lengthscales, G noises].
//   mode 0  only the natural rows of the current raw parameters (before the first k1 of a run; init: a new fit's
//           Rprop state prev = 0, step = lr)
//   mode 1  sums, loss, history rows, gradient: the evaluation without an update
//   mode 2  the same, the Rprop step of the parameters that require a gradient, and the natural rows of the new ones
// Sums: level 1 = the per-workgroup partials of k_wide_fit_eig / k_wide_k1_bwd, level 2 here, a lane over every
// kWG-th partial in ascending order, then block_sum's fixed tree.
struct WideFitStep {
  Fit f;
  int G, d, dl, nbe;
  double w, lr;
  const double* pe;          // [G][3][nbe]
  const double* dscale;      // [G]      dL/dscale
  const double* dls;         // [G][d]   dL/dl_j
  double* nat_scale;         // [G]
  double* nat_ls;            // [G][d]
};

__global__ __launch_bounds__(kWG) void k_wide_fit_step(WideFitStep s, int iter, int mode, int init) {
  __shared__ double red[kWG / 64];
  const int tid = threadIdx.x;
  const int g = blockIdx.x;
  const int G = s.G, d = s.d, dl = s.dl;
  const Fit& f = s.f;
  const int p_scale = g, p_ls = G + g * dl, p_noise = G + G * dl + g;
  if (mode != 0) {
    double sums[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const double* pq = s.pe + ((int64_t)g * 3 + q) * s.nbe;
      double a = 0.0;
      for (int c = tid; c < s.nbe; c += kWG) a += pq[c];
      sums[q] = block_sum(a, red);
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
        gnat = 0.5 * sums[2];
      }
      const double graw = nat * gnat;          // exp transforms: d nat / d raw = nat
      f.raw_hist[(int64_t)iter * f.n_params + p] = f.raw[p];
      f.grad_out[p] = graw;
      if (mode == 2 && rg) rprop_update(f, p, graw);
    }
    if (tid == 0) {
      const double t2 = s.w * sums[1];
      double* lh = f.loss_hist + ((int64_t)iter * G + g) * 3;
      lh[0] = 0.5 * (sums[0] + t2) + f.mll_const;
      lh[1] = sums[0];
      lh[2] = t2;
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
  int64_t o_scale, o_ls, o_dscale, o_dls, o_a, o_b, o_w, o_pe, o_pb, len;   // offsets into work, in doubles
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
  p.len = o;
  return kOk;
}

static int wide_fit_run(const fgp_wide_fit_desc* a, const WideFitPlan& p, int iter0, int iters, int final_no_update,
                        hipStream_t st) {
  const int G = a->G, d = a->d, m = a->log2n;
  const int64_t n = p.n;
  double* work = static_cast<double*>(a->work);
  double *nat_scale = work + p.o_scale, *nat_ls = work + p.o_ls, *dscale = work + p.o_dscale, *dls = work + p.o_dls;
  double *A = work + p.o_a, *B = work + p.o_b, *W = work + p.o_w, *pe = work + p.o_pe, *pb = work + p.o_pb;
  WideFitStep s{};
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
  s.pe = pe, s.dscale = dscale, s.dls = dls, s.nat_scale = nat_scale, s.nat_ls = nat_ls;
  const double* raw_noise = a->raw + (int64_t)G * (1 + a->dl);
  const double sqrtn = std::sqrt((double)n);
  k_wide_fit_step<<<G, kWG, 0, st>>>(s, 0, 0, iter0 == 0 && a->lr > 0.0);
  int rc = check_launch("k_wide_fit_step");
  for (int it = 0; it < iters && rc == kOk; ++it) {
    // k1 (per problem when every problem has its own parts: fgp_wide_k1 takes ONE parts array)
    if (a->parts_stride == 0) {
      rc = fgp_wide_k1(a->parts, n, d, nat_scale, nat_ls, G, A, st);
    } else {
      for (int g = 0; g < G && rc == kOk; ++g)
        rc = fgp_wide_k1(a->parts + g * a->parts_stride, n, d, nat_scale + g, nat_ls + (int64_t)g * d, 1, A + g * n, st);
    }
    if (rc != kOk) break;
    // lambda = ft(k1), stable (AbstractFastGP.ft)
    if (!p.lat) rc = fgp_fwht(A, n, B, G, m, 1, st);
    else if (p.r2c) rc = fgp_fftbr_real(A, n, B, W, G, m, st);
    else rc = fgp_fftbr(A, n, 1, B, G, m, 1, st);
    if (rc != kOk) break;
    const dim3 grid((unsigned)p.nbe, (unsigned)G);
    if (p.lat) k_wide_fit_eig<0><<<grid, kWG, 0, st>>>(B, a->ysq, raw_noise, n, sqrtn, a->logdet_weight, p.nbe, pe);
    else k_wide_fit_eig<1><<<grid, kWG, 0, st>>>(B, a->ysq, raw_noise, n, sqrtn, a->logdet_weight, p.nbe, pe);
    rc = check_launch("k_wide_fit_eig");
    if (rc != kOk) break;
    // u = dL/dk1: the adjoint transform of g~ (lattice: the real part)
    if (!p.lat) rc = fgp_fwht(B, n, A, G, m, 1, st);
    else if (p.r2c) rc = fgp_ifftbr_real(B, n, nullptr, 0, A, n, W, G, m, st);
    else rc = fgp_ifftbr(B, n, A, 1, W, G, m, 1, st);
    if (rc != kOk) break;
    if (a->parts_stride == 0) {
      rc = fgp_wide_k1_bwd(a->parts, n, d, nat_scale, nat_ls, G, A, dscale, dls, pb, st);
    } else {
      for (int g = 0; g < G && rc == kOk; ++g)
        rc = fgp_wide_k1_bwd(a->parts + g * a->parts_stride, n, d, nat_scale + g, nat_ls + (int64_t)g * d, 1, A + g * n,
                             dscale + g, dls + (int64_t)g * d, pb, st);
    }
    if (rc != kOk) break;
    const bool last = it + 1 == iters;
    k_wide_fit_step<<<G, kWG, 0, st>>>(s, iter0 + it, (last && final_no_update) ? 1 : 2, 0);
    rc = check_launch("k_wide_fit_step");
  }
  return rc;
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
  const struct {
    const void* ptr;
    const char* name;
  } ptrs[] = {{desc->parts, "parts"},           {desc->ysq, "ysq"},           {desc->raw, "raw"},
              {desc->rprop_prev, "rprop_prev"}, {desc->rprop_step, "rprop_step"}, {desc->loss_hist, "loss_hist"},
              {desc->raw_hist, "raw_hist"},     {desc->grad_out, "grad_out"}, {desc->work, "work"}};
  for (const auto& q : ptrs)
    if (!q.ptr) return set_error(kErrInvalid, "fgp_wide_fit_run: null pointer: %s", q.name);
  if (iters < 0) return set_error(kErrInvalid, "fgp_wide_fit_run: iters=%d negative", iters);
  if (iter0 < 0) return set_error(kErrInvalid, "fgp_wide_fit_run: iter0=%d negative", iter0);
  if (((uintptr_t)desc->ysq | (uintptr_t)desc->work) & 15)
    return set_error(kErrInvalid, "fgp_wide_fit_run: ysq and work must be 16-byte aligned");
  if (iters == 0) return kOk;
  return wide_fit_run(desc, p, iter0, iters, final_no_update, (hipStream_t)stream);
}

}  // extern "C"
