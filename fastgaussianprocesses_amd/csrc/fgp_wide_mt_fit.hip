// Wide inputs (9 <= d <= 64), multitask / derivative-informed GPs: the device-resident fit loop (MLL; GCV / CV),
// fgp_wide_mt_fit_run (include/fgp_hip.h, an addition to ABI 20) -- AbstractGP.fit's iteration (abstract_gp.py:241-296:
// loss, loss.backward(), torch.optim.Rprop.step()) over _FastInverseLogDetCache's lams and block inverse
// (util.py:275-370) for ONE eigen-problem of T sorted tasks, as a fixed sequence of plain launches on the caller's
// stream.  With np = T (T + 1) / 2 sorted pairs (k, l), k <= l, one iteration is
//
//   k1        fgp_wide_mt_k1, one call per pair        k1_kl into A at the packed offset of (k, l)      (fgp_wide_mt.hip)
//   lambda    fgp_fftbr / fgp_fftbr_real / fgp_fwht    one batched call per sorted task k over its T - k rows
//   lams      k_wide_mt_lams (new)                     K_task[a_k, a_l] (sqrt(n_l) lam^_kl + noise [k == l]), packed
//   blocks    fgp_mt_factor / fgp_mt_solve / fgp_mt_selinv / fgp_mt_mll_grad                            (fgp_multitask.hip)
//   contract  k_wide_mt_contract (new)                 g~ = dL/dlambda over lambda; partials of the noise and K_task
//                                                      gradients, of the norm and of the logdet
//   u         fgp_ifftbr (real part) / fgp_ifftbr_real / fgp_fwht, batched per k: u = dL/dk1 over k1
//   gradient  fgp_wide_mt_k1_bwd, one call per pair    into dsl [np][1 + d]
//   step      k_wide_mt_fit_step (new, one workgroup)  second level of every sum, loss, histories, chain rule to the
//                                                      raw parameters, Rprop (rprop_update, fgp_nll.h), the natural
//                                                      scale / lengthscale row of the next k1
//
// 3 np + 2 T + 7 entry-point calls per iteration.  fgp_wide_mt_fit_desc.loss_metric GCV / CV (equal n per task) keeps
// every stage but fgp_mt_mll_grad, which k_wide_mt_loss_sums + k_wide_mt_loss_grad (new, below) replace: one call more.
// No host synchronisation, no device-to-host copy, no atomics, no
// inter-workgroup hand-off: every kernel reads what a launch before it wrote.  lam^ = lambda, or conj(lambda) where
// the pair's conj flag is set (task index a_k > a_l: util.py:280-284).  Nets: lambda and g~ are real (the generic
// loop's .to(complex128) passes the real part of the gradient back).  fgp_wide_mt_k1 / _k1_bwd take their spec by
// value (no device table, no copy), so validating every pair's spec before the first launch is all the "first use"
// there is; the transforms' twiddle tables are made on their first call as everywhere else.
//
// PARAMETER batches (fgp_wide_mt_fit_batch_desc: G > 1 problems, each with its own rows of the five parameter blocks; the work
// layout and the bit contract are stated in include/fgp_hip.h): the same stages over G problems, the launch count
// independent of G.  k1 / transforms / k1_bwd take a pair's G rows in one call (A and B are pair-major [p][G][n_k]), the
// block calls take G problems (lams .. glp problem-major [G][L]), k_wide_mt_lams / k_wide_mt_contract get the problem as
// blockIdx.z, and the one-workgroup step is split in two: k_wide_mt_fit_sums (a workgroup per problem: the evaluation
// half) and k_wide_mt_fit_bstep (element sums over the problems, loss row, histories, Rprop, natural rows) -- one call
// more.  With G <= 1 every index below reduces to the one-problem one and k_wide_mt_fit_step runs as before.
#include <cmath>
#include <cstdint>

#include "fgp_common.h"
#include "fgp_nll.h"
#include "fgp_runtime.h"
#include "../../include/fgp_hip.h"

namespace fgp {

constexpr int kWmfT = FGP_MT_MAX_TASKS;
constexpr int kWmfPairs = FGP_WIDE_MT_FIT_PAIRS;
constexpr int kWmfMaxParams = 2 + FGP_WIDE_MAX_D + kWmfT * kWmfT + kWmfT;
constexpr int kWmfMaxG = 4096;               // problems of a parameter batch, raw elements of all their rows
constexpr int kWmfMaxBatchParams = 8192;

// what the new kernels need of the problem, by value
struct WmfLay {
  int T, np;                       // sorted active tasks, pairs
  int T_all, rank, vtask_exp;
  int f_off, v_off, noise_off;     // raw offsets of the task factor, the task noise and the noise (G > 1: of row 0)
  int G;                           // problems (>= 1)
  int64_t L;                       // packed length of one problem
  int64_t n[kWmfT];                // descending
  int64_t offk[kWmfT];             // packed offset of pair (k, k); pair (k, l) at offk[k] + (l - k) n[k]
  int task[kWmfT];                 // task index a_k of sorted task k
  unsigned long long conj[(kWmfPairs + 63) / 64];   // bit p: pair p's lambda is conjugated
};

// pair index p (row-major over k <= l) -> (k, l)
__device__ __forceinline__ void wmf_pair(const WmfLay& m, int p, int& k, int& l) {
  k = 0;
  int rem = p;
  while (rem >= m.T - k) {
    rem -= m.T - k;
    ++k;
  }
  l = k + rem;
}

// K_task[a, b] = sum_r F[a, r] F[b, r] + [a == b] v_a from the raw rows (mtg_kt, fgp_multitask.hip; util.py:157-162)
// (f_off, v_off: the raw offsets of the problem's task-factor and task-noise rows)
__device__ __forceinline__ double wmf_kt(const WmfLay& m, const double* __restrict__ raw, int f_off, int v_off, int a,
                                         int b) {
  double s = 0.0;
  for (int r = 0; r < m.rank; ++r) s += raw[f_off + a * m.rank + r] * raw[f_off + b * m.rank + r];
  if (a == b) s += m.vtask_exp ? exp(raw[v_off + a]) : raw[v_off + a];
  return s;
}

// the raw offsets of problem g's noise, task-factor and task-noise rows (rows [5][G]; NULL: row 0 of every block)
struct WmfOff {
  int noise, f, v;
};
__device__ __forceinline__ WmfOff wmf_off(const WmfLay& m, const int* __restrict__ rows, int g) {
  WmfOff o;
  o.noise = m.noise_off, o.f = m.f_off, o.v = m.v_off;
  if (rows) {
    o.noise += rows[2 * m.G + g];
    o.f += rows[3 * m.G + g] * m.T_all * m.rank;
    o.v += rows[4 * m.G + g] * m.T_all;
  }
  return o;
}
// element i of sorted pair (k, l) of problem g: in the pair-major transform arrays A / B, in the problem-major packed ones
__device__ __forceinline__ int64_t wmf_epair(const WmfLay& m, int k, int l, int g, int64_t i) {
  return (int64_t)m.G * m.offk[k] + ((int64_t)(l - k) * m.G + g) * m.n[k] + i;
}
__device__ __forceinline__ int64_t wmf_eprob(const WmfLay& m, int k, int l, int g, int64_t i) {
  return (int64_t)g * m.L + m.offk[k] + (int64_t)(l - k) * m.n[k] + i;
}

template <int FAM>
__device__ __forceinline__ double2 wmf_lam(const void* __restrict__ lam, int64_t e, bool cj) {
  if constexpr (FAM == 0) {
    const double2 v = static_cast<const double2*>(lam)[e];
    return make_double2(v.x, cj ? -v.y : v.y);
  } else {
    return make_double2(static_cast<const double*>(lam)[e], 0.0);
  }
}

// ------------------------------------------------------------------------------------------------
// lams[k, l][i] = K_task[a_k, a_l] (sqrt(n_l) lam^_kl[i] + noise [k == l])  (util.py:284-298), thread = entry i of pair
// p = blockIdx.y of problem g = blockIdx.z.  lam: complex128 (FAM 0) / float64 (FAM 1), pair-major [p][G][n_k]; lams
// problem-major [G][L] (one problem: both are the packed layout).
template <int FAM>
__global__ __launch_bounds__(kWG) void k_wide_mt_lams(WmfLay m, const double* __restrict__ raw,
                                                      const int* __restrict__ rows, const void* __restrict__ lam,
                                                      double2* __restrict__ lams) {
  const int p = blockIdx.y, g = blockIdx.z;
  int k, l;
  wmf_pair(m, p, k, l);
  const int64_t i = (int64_t)blockIdx.x * kWG + threadIdx.x;
  if (i >= m.n[k]) return;
  const WmfOff o = wmf_off(m, rows, g);
  const bool cj = (m.conj[p >> 6] >> (p & 63)) & 1ull;
  const double2 v = wmf_lam<FAM>(lam, wmf_epair(m, k, l, g, i), cj);
  const double rn = sqrt((double)m.n[l]);
  double bx = rn * v.x;
  const double by = rn * v.y;
  if (k == l) bx += exp(raw[o.noise]);
  const double kt = wmf_kt(m, raw, o.f, o.v, m.task[k], m.task[l]);
  lams[wmf_eprob(m, k, l, g, i)] = make_double2(bx * kt, by * kt);
}

// ------------------------------------------------------------------------------------------------
// Pair p = blockIdx.y < np, entries [blockIdx.x kWG, +kWG): with g = dL/dlams (torch's convention dL/dRe + i dL/dIm),
//   lam[e]             = g~ = K_task sqrt(n_l) g, conjugated by the pair's flag (FAM 1: its real part)
//   part[p][0][blk]    = sum_i Re g[i]                                               (diagonal pairs: d/dnoise / K_task)
//   part[p][1][blk]    = sum_i Re(conj(g[i]) (sqrt(n_l) lam^[i] + noise [k == l]))   (dL/dK_task[a_k, a_l])
// blockIdx.y == np: part[np][0][blk] = this workgroup's share of sum_b Re(conj(y_b) z_b), part[np][1][blk] of the
// classes' logdet.  A workgroup past its pair's n_k writes nothing, and the step reads none of its partials.
// Problem g = blockIdx.z: its yz_len entries of y and z, its nmin classes of logdet, its [np + 1][2][nbx] of part.
template <int FAM>
__global__ __launch_bounds__(kWG) void k_wide_mt_contract(WmfLay m, const double* __restrict__ raw,
                                                          const int* __restrict__ rows,
                                                          const double2* __restrict__ glp, void* __restrict__ lam,
                                                          const double2* __restrict__ y, const double2* __restrict__ z,
                                                          int64_t yz_len, const double* __restrict__ logdet, int nbx,
                                                          double* __restrict__ part) {
  __shared__ double red[kWG / 64];
  const int p = blockIdx.y, g = blockIdx.z;
  y += (int64_t)g * yz_len, z += (int64_t)g * yz_len;
  logdet += (int64_t)g * m.n[m.T - 1];
  part += (int64_t)g * (m.np + 1) * 2 * nbx;
  double s0 = 0.0, s1 = 0.0;
  if (p == m.np) {
    const int64_t t0 = (int64_t)blockIdx.x * kWG + threadIdx.x, nt = (int64_t)nbx * kWG;
    for (int64_t e = t0; e < yz_len; e += nt) {
      const double2 yv = y[e], zv = z[e];
      s0 = __builtin_fma(yv.x, zv.x, __builtin_fma(yv.y, zv.y, s0));
    }
    for (int64_t j = t0; j < m.n[m.T - 1]; j += nt) s1 += logdet[j];
  } else {
    int k, l;
    wmf_pair(m, p, k, l);
    if ((int64_t)blockIdx.x * kWG >= m.n[k]) return;
    const int64_t i = (int64_t)blockIdx.x * kWG + threadIdx.x;
    if (i < m.n[k]) {
      const WmfOff o = wmf_off(m, rows, g);
      const int64_t e = wmf_epair(m, k, l, g, i);
      const bool cj = (m.conj[p >> 6] >> (p & 63)) & 1ull;
      const double2 v = wmf_lam<FAM>(lam, e, cj);
      const double2 gv = glp[wmf_eprob(m, k, l, g, i)];
      const double rn = sqrt((double)m.n[l]);
      double bx = rn * v.x;
      const double by = rn * v.y;
      if (k == l) bx += exp(raw[o.noise]);
      const double f = wmf_kt(m, raw, o.f, o.v, m.task[k], m.task[l]) * rn;
      s0 = gv.x;
      s1 = __builtin_fma(gv.x, bx, gv.y * by);
      if constexpr (FAM == 0) static_cast<double2*>(lam)[e] = make_double2(f * gv.x, cj ? -(f * gv.y) : f * gv.y);
      else static_cast<double*>(lam)[e] = f * gv.x;
    }
  }
  s0 = block_sum(s0, red);
  s1 = block_sum(s1, red);
  if (threadIdx.x == 0) {
    part[((int64_t)p * 2 + 0) * nbx + blockIdx.x] = s0;
    part[((int64_t)p * 2 + 1) * nbx + blockIdx.x] = s1;
  }
}

// ------------------------------------------------------------------------------------------------
// GCV / CV (fgp_wide_mt_fit_desc.loss_metric; util.py:371-394, abstract_gp.py:242-273; the closed forms of T tasks of
// EQUAL n above k_mt_spec_iter, fgp_spectral.hip).  With equal n every frequency class j < n has one row per task, so the
// selected inverse zinv IS the dense A_j = Lambda_j^-1 (upper triangle, packed as the lams) and z [B][T n] its solutions.
//   GCV  N = sum_b sum_j |z_bj|^2, Tr = sum_j Re tr A_j, D = (Tr / (T n))^2, loss = N / D
//   CV   N_t = sum_b sum_j |z_bjt|^2, S_t = n I_t = sum_j Re A_j[t, t], loss = w n^2 sum_t N_t / S_t^2
// Both gradients are one form.  With S_rt = sum_b z_r conj(z_t) (per class),
//   W[r, c] = sum_t ( c2_t A_rt conj(A_ct) - c1_t (S_rt conj(A_ct) + A_rt S_tc) ),      dL = Re tr(W dLambda)
//   GCV  c1_t = 1 / D, c2_t = 2 N / (D Tr) for every t      (dN = -2 Re(u^H dLambda z), u = A z;  dTr = -Re tr(A^2 dLambda))
//   CV   c1_t = w n^2 / S_t^2, c2_t = 2 c1_t N_t / S_t      (u = A e_t z_t;  dS_t = -(A e_t)^H dLambda (A e_t))
// and glp takes fgp_mt_mll_grad's convention: Re W[r, r] on the diagonal, 2 W[r, c] on a coupling entry r < c.
// The sums are global, so the stage is two kernels: k_wide_mt_loss_sums writes per-workgroup partials
//   pl [NT][2][nbx] = (N, Tr) (GCV, NT = 1) or (N_t, S_t) per task (CV, NT = T),
// k_wide_mt_loss_grad re-forms the totals in every workgroup (wmf_total: the same order everywhere, so the same bits)
// and writes W.  A thread per frequency; the T x T block is never held in registers or LDS: A and z are re-read from
// global memory (L1 / L2: a wavefront's reads of one entry are contiguous), T (2 B + 3) complex products per entry.
// FAM 1 (nets): A is real (k_wide_mt_lams writes zero imaginary parts and the factor keeps them), its imaginary parts
// are not read and their products are dropped -- the bits of the complex form on a zero imaginary part.
constexpr int kWmfLossQ = 2;

struct WmfCoef {
  double loss, c1, c2, D;
};

// GCV: (N, Tr) -> loss, c1, c2, D.  CV: (N_t, S_t) -> task t's term of the loss, c1_t, c2_t.  tn = T n, wn2 = w n^2
// (exact: n is a power of two).
__device__ __forceinline__ WmfCoef wmf_loss_coef(bool cv, double N, double S, double tn, double wn2) {
  WmfCoef c;
  if (cv) {
    c.D = S * S;
    c.c1 = wn2 / c.D;
    c.loss = c.c1 * N;
    c.c2 = 2.0 * c.loss / S;
  } else {
    const double q = S / tn;
    c.D = q * q;
    c.loss = N / c.D;
    c.c1 = 1.0 / c.D;
    c.c2 = 2.0 * N / (c.D * S);
  }
  return c;
}

// the second level of one row of partials: a lane over every kWG-th partial in ascending order, then block_sum
__device__ __forceinline__ double wmf_total(const double* __restrict__ row, int cnt, double* red) {
  double a = 0.0;
  for (int c = threadIdx.x; c < cnt; c += kWG) a += row[c];
  return block_sum(a, red);
}

// A[r][t] of class j from the packed upper triangle (Z offset by j)
template <int FAM>
__device__ __forceinline__ double2 wmf_ainv(const WmfLay& m, const double2* __restrict__ Z, int r, int t) {
  const int lo = r <= t ? r : t, hi = r <= t ? t : r;
  const int64_t e = m.offk[lo] + (int64_t)(hi - lo) * m.n[0];
  if constexpr (FAM == 1) return make_double2(Z[e].x, 0.0);
  const double2 v = Z[e];
  return make_double2(v.x, r <= t ? v.y : -v.y);
}
template <int FAM>
__device__ __forceinline__ double2 wmf_a_mulc_a(double2 a, double2 b) {      // a conj(b)
  if constexpr (FAM == 1) return make_double2(a.x * b.x, 0.0);
  return cmulc(a, b);
}
template <int FAM>
__device__ __forceinline__ double2 wmf_s_mulc_a(double2 s, double2 a) {      // s conj(a)
  if constexpr (FAM == 1) return make_double2(s.x * a.x, s.y * a.x);
  return cmulc(s, a);
}
template <int FAM>
__device__ __forceinline__ double2 wmf_a_mul_s(double2 a, double2 s) {       // a s
  if constexpr (FAM == 1) return make_double2(a.x * s.x, a.x * s.y);
  return cmul(a, s);
}

// blockIdx.x: kWG frequencies; CV: blockIdx.y = task t.  Per thread B ascending (GCV: the tasks ascending inside), then
// block_sum.
template <bool CV>
__global__ __launch_bounds__(kWG) void k_wide_mt_loss_sums(WmfLay m, int B, const double2* __restrict__ zinv,
                                                           const double2* __restrict__ z, int nbx,
                                                           double* __restrict__ pl) {
  __shared__ double red[kWG / 64];
  const int64_t n = m.n[0], j = (int64_t)blockIdx.x * kWG + threadIdx.x;
  const int t0 = CV ? (int)blockIdx.y : 0, t1 = CV ? t0 + 1 : m.T;
  double s0 = 0.0, s1 = 0.0;
  if (j < n) {
    for (int b = 0; b < B; ++b)
      for (int t = t0; t < t1; ++t) {
        const double2 zv = z[((int64_t)b * m.T + t) * n + j];
        s0 = __builtin_fma(zv.x, zv.x, __builtin_fma(zv.y, zv.y, s0));
      }
    for (int t = t0; t < t1; ++t) s1 += zinv[m.offk[t] + j].x;
  }
  s0 = block_sum(s0, red);
  s1 = block_sum(s1, red);
  if (threadIdx.x == 0) {
    pl[((int64_t)t0 * kWmfLossQ + 0) * nbx + blockIdx.x] = s0;
    pl[((int64_t)t0 * kWmfLossQ + 1) * nbx + blockIdx.x] = s1;
  }
}

template <int FAM, bool CV>
__global__ __launch_bounds__(kWG) void k_wide_mt_loss_grad(WmfLay m, int B, double cv_weight,
                                                           const double2* __restrict__ zinv,
                                                           const double2* __restrict__ z, int nbx,
                                                           const double* __restrict__ pl, double2* __restrict__ glp) {
  __shared__ double red[kWG / 64];
  __shared__ double c1s[kWmfT], c2s[kWmfT];
  const int T = m.T;
  const int64_t n = m.n[0], j = (int64_t)blockIdx.x * kWG + threadIdx.x;
  const double tn = (double)T * (double)n, wn2 = cv_weight * (double)n * (double)n;
  for (int t = 0; t < (CV ? T : 1); ++t) {
    const double N = wmf_total(pl + ((int64_t)t * kWmfLossQ + 0) * nbx, nbx, red);
    const double S = wmf_total(pl + ((int64_t)t * kWmfLossQ + 1) * nbx, nbx, red);
    const WmfCoef c = wmf_loss_coef(CV, N, S, tn, wn2);
    if (threadIdx.x == 0) c1s[t] = c.c1, c2s[t] = c.c2;
  }
  __syncthreads();
  if (j >= n) return;
  const double2* Z = zinv + j;
  const double2* zj = z + j;
  for (int r = 0; r < T; ++r)
    for (int c = r; c < T; ++c) {
      double wx = 0.0, wy = 0.0;
      for (int t = 0; t < T; ++t) {
        const double2 art = wmf_ainv<FAM>(m, Z, r, t), act = wmf_ainv<FAM>(m, Z, c, t);
        double2 srt = make_double2(0.0, 0.0), stc = make_double2(0.0, 0.0);
        for (int b = 0; b < B; ++b) {
          const double2* zb = zj + (int64_t)b * T * n;
          const double2 zr = zb[(int64_t)r * n], zt = zb[(int64_t)t * n], zc = zb[(int64_t)c * n];
          srt += cmulc(zr, zt);
          stc += cmulc(zt, zc);
        }
        const double2 e1 = wmf_a_mulc_a<FAM>(art, act);
        double2 e2 = wmf_s_mulc_a<FAM>(srt, act);
        e2 += wmf_a_mul_s<FAM>(art, stc);
        const double c1 = c1s[CV ? t : 0], c2 = c2s[CV ? t : 0];
        wx = __builtin_fma(-c1, e2.x, __builtin_fma(c2, e1.x, wx));
        wy = __builtin_fma(-c1, e2.y, __builtin_fma(c2, e1.y, wy));
      }
      glp[m.offk[r] + (int64_t)(c - r) * n + j] = r == c ? make_double2(wx, 0.0) : make_double2(2.0 * wx, 2.0 * wy);
    }
}

// ------------------------------------------------------------------------------------------------
// The step, one workgroup.  raw = [scale, dl lengthscales, noise, task factor T_all x rank, task noise T_all].
//   mode 0  the natural scale / lengthscale row of the current raw parameters, the constant gradient rows of
//           fgp_mt_mll_grad (gn [B] = 1/2, gl = 1/2 w) and the cleared info flag, before the first k1 of a run
//           (init: a new fit's Rprop state prev = 0, step = lr)
//   mode 1  sums, loss, history rows, gradient: the evaluation without an update
//   mode 2  the same, the Rprop step of the blocks that require a gradient, and the natural row of the new parameters
// Sums: level 1 = the per-workgroup partials of k_wide_mt_contract / the per-pair totals of fgp_wide_mt_k1_bwd, level 2
// here -- a lane over every kWG-th partial in ascending order, then block_sum's fixed tree; the pairs in ascending order.
struct WmfStep {
  Fit f;
  WmfLay lay;
  int d, dl, B, nbx;
  int rg_factor, rg_vtask;
  double w, lr;
  const double* part;        // [np + 1][2][nbx]
  const double* dsl;         // [np][1 + d]   dL/dscale, dL/dl_j of every pair
  double* nat;               // [1 + d]       natural scale, lengthscales
  double* gn;                // [B], then gl [1]
  int* info;
  int loss;                  // FGP_LOSS_MLL / _GCV / _CV
  double cv_weight;
  const double* pl;          // GCV / CV: k_wide_mt_loss_sums' partials [NT][2][nbx]
};

// The second level of one problem's sums (the evaluation half of the step, shared by k_wide_mt_fit_step and
// k_wide_mt_fit_sums): tot[2 p + q] of part [np + 1][2][nbx] -- a lane over every kWG-th partial ascending, then
// block_sum; only the first ceil(n_k / kWG) partials of a pair, and of q = 0 the diagonal pairs only -- and dsum[0 .. d]
// = the sum over the pairs, ascending, of dscale / dls[j] (pair p's at ds + p ds_pair and dlp + j + p ds_pair).  Ends with a
// barrier.
__device__ __forceinline__ void wmf_second_level(const WmfLay& m, int d, int nbx, const double* __restrict__ part,
                                                 const double* __restrict__ ds, const double* __restrict__ dlp,
                                                 int64_t ds_pair, double* red, double* tot, double* dsum) {
  const int tid = threadIdx.x, np = m.np;
  for (int p = 0; p <= np; ++p) {
    int k = 0, l = 0;
    int64_t cnt = nbx;
    if (p < np) {
      wmf_pair(m, p, k, l);
      cnt = (m.n[k] + kWG - 1) / kWG;
    }
    for (int q = 0; q < 2; ++q) {
      if (p < np && q == 0 && k != l) continue;        // Re g sums: the diagonal pairs only
      const double* pq = part + ((int64_t)p * 2 + q) * nbx;
      double a = 0.0;
      for (int64_t c = tid; c < cnt; c += kWG) a += pq[c];
      a = block_sum(a, red);
      if (tid == 0) tot[2 * p + q] = a;
    }
  }
  if (tid <= d) {
    double a = 0.0;
    for (int p = 0; p < np; ++p) a += (tid == 0 ? ds : dlp + (tid - 1))[(int64_t)p * ds_pair];
    dsum[tid] = a;
  }
  __syncthreads();
}

// One problem's raw gradient of its own parameter x, x in one problem's order [scale, dl lengthscales, noise, task factor
// T_all x rank, task noise T_all]; o: the raw offsets of the problem's noise, factor and task-noise rows; nat_s, nat_l: its
// natural scale and lengthscales.
__device__ __forceinline__ double wmf_raw_grad(const WmfLay& m, int d, int dl, int x, const double* __restrict__ raw,
                                               const WmfOff& o, double nat_s, const double* __restrict__ nat_l,
                                               const double* tot, const double* dsum) {
  const int noise1 = 1 + dl, f1 = noise1 + 1, v1 = f1 + m.T_all * m.rank;
  double gs = 0.0;
  if (x == 0) {
    gs = nat_s * dsum[0];                                              // exp transforms: d nat / d raw = nat
  } else if (x < noise1) {
    const int j = x - 1;
    if (dl == d) {
      gs = nat_l[j] * dsum[1 + j];
    } else {                                                            // one lengthscale: the sum over j, ascending
      double a = 0.0;
      for (int jj = 0; jj < d; ++jj) a += dsum[1 + jj];
      gs = nat_l[0] * a;
    }
  } else if (x == noise1) {
    double a = 0.0;
    for (int k = 0, p = 0; k < m.T; p += m.T - k, ++k) a += wmf_kt(m, raw, o.f, o.v, m.task[k], m.task[k]) * tot[2 * p];
    gs = exp(raw[o.noise]) * a;
  } else if (x < v1) {
    // K_task[a, b] = sum_r F[a, r] F[b, r] + [a == b] v_a:  dF[c, r] += g_ab (F[b, r] [a == c] + F[a, r] [b == c])
    const int u = x - f1, c = u / m.rank, r = u - c * m.rank;
    for (int k = 0, p = 0; k < m.T; ++k) {
      const int a = m.task[k];
      for (int l = k; l < m.T; ++l, ++p) {
        const int b = m.task[l];
        const double gv = tot[2 * p + 1];
        if (a == c) gs += gv * raw[o.f + b * m.rank + r];
        if (b == c) gs += gv * raw[o.f + a * m.rank + r];
      }
    }
  } else {
    const int c = x - v1;
    for (int k = 0, p = 0; k < m.T; p += m.T - k, ++k)
      if (m.task[k] == c) gs += m.vtask_exp ? tot[2 * p + 1] * exp(raw[o.v + c]) : tot[2 * p + 1];
  }
  return gs;
}

__global__ __launch_bounds__(kWG) void k_wide_mt_fit_step(WmfStep s, int iter, int mode, int init) {
  __shared__ double red[kWG / 64];
  __shared__ double tot[2 * (kWmfPairs + 1)];     // [p][0 / 1]: the second-level sums of part
  __shared__ double dsum[1 + FGP_WIDE_MAX_D];     // sum over the pairs of dsl
  __shared__ double grad[kWmfMaxParams];
  const int tid = threadIdx.x;
  const Fit& f = s.f;
  const WmfLay& m = s.lay;
  const int d = s.d, dl = s.dl, np = m.np, n_params = f.n_params;
  if (mode != 0) {
    wmf_second_level(m, d, s.nbx, s.part, s.dsl, s.dsl + 1, 1 + d, red, tot, dsum);
    // the raw gradient of every parameter, before any parameter moves (the task-factor rows read one another)
    const WmfOff o = wmf_off(m, nullptr, 0);
    for (int x = tid; x < n_params; x += kWG) grad[x] = wmf_raw_grad(m, d, dl, x, f.raw, o, s.nat[0], s.nat + 1, tot, dsum);
    if (s.loss != FGP_LOSS_MLL) {
      // GCV / CV: the second level of the loss sums in k_wide_mt_loss_grad's order; the row (loss, N, D) or
      // (loss, NaN, NaN); tot[2 np], tot[2 np + 1], mll_const and w are unread
      const bool cv = s.loss == FGP_LOSS_CV;
      const double nn = (double)m.n[0], tn = (double)m.T * nn, wn2 = s.cv_weight * nn * nn;
      double loss = 0.0, t1 = nan(""), t2 = nan("");
      for (int t = 0; t < (cv ? m.T : 1); ++t) {
        const double N = wmf_total(s.pl + ((int64_t)t * kWmfLossQ + 0) * s.nbx, s.nbx, red);
        const double S = wmf_total(s.pl + ((int64_t)t * kWmfLossQ + 1) * s.nbx, s.nbx, red);
        const WmfCoef c = wmf_loss_coef(cv, N, S, tn, wn2);
        loss += c.loss;                                                     // the tasks in ascending order
        if (!cv) t1 = N, t2 = c.D;
      }
      if (tid == 0) {
        double* lh = f.loss_hist + (int64_t)iter * 3;
        lh[0] = loss;
        lh[1] = t1;
        lh[2] = t2;
      }
    } else if (tid == 0) {
      double* lh = f.loss_hist + (int64_t)iter * 3;
      const double t1 = tot[2 * np], t2 = s.w * tot[2 * np + 1];
      lh[0] = 0.5 * (t1 + t2) + f.mll_const;
      lh[1] = t1;
      lh[2] = t2;
    }
    __syncthreads();
    for (int x = tid; x < n_params; x += kWG) {
      const double gp = grad[x];
      f.raw_hist[(int64_t)iter * n_params + x] = f.raw[x];
      f.grad_out[x] = gp;
      int rg;
      if (x == 0) rg = f.scale_rg;
      else if (x < m.noise_off) rg = f.ls_rg;
      else if (x == m.noise_off) rg = f.noise_rg;
      else if (x < m.v_off) rg = s.rg_factor;
      else rg = s.rg_vtask;
      if (mode == 2 && rg) rprop_update(f, x, gp);
    }
    if (mode != 2) return;
    __syncthreads();
  } else {
    if (init)
      for (int x = tid; x < n_params; x += kWG) {
        f.prev[x] = 0.0;
        f.step[x] = s.lr;
      }
    for (int b = tid; b <= s.B; b += kWG) s.gn[b] = b < s.B ? 0.5 : 0.5 * s.w;
    if (tid == 0) s.info[0] = 0;
  }
  if (tid == 0) s.nat[0] = exp(f.raw[0]);
  for (int j = tid; j < d; j += kWG) s.nat[1 + j] = exp(f.raw[1 + (dl == d ? j : 0)]);
}

// ------------------------------------------------------------------------------------------------ G > 1 problems
// The evaluation half of the step for problem g = blockIdx.x: sums[g] = (norm_g, logdet_g, the problem's raw-space
// contribution to each of its own P1 = 2 + dl + T_all rank + T_all parameters), by wmf_second_level and wmf_raw_grad --
// the sums, the order and the expressions of k_wide_mt_fit_step on this problem alone.  LDS: 8 (4 + 2 (np + 1) + 1 + 64)
// <= 2.7 KB, static.
struct WmfSums {
  WmfLay lay;
  int d, dl, nbx;
  const double* raw;
  const int* rows;           // [5][G]
  const double* part;        // [G][np + 1][2][nbx]
  const double* dsl;         // per pair dscale [G], then dls [G][d]
  const double* nat;         // scale [G], then lengthscales [G][d]
  double* sums;              // [G][2 + P1]
};

__global__ __launch_bounds__(kWG) void k_wide_mt_fit_sums(WmfSums s) {
  __shared__ double red[kWG / 64];
  __shared__ double tot[2 * (kWmfPairs + 1)];
  __shared__ double dsum[1 + FGP_WIDE_MAX_D];
  const WmfLay& m = s.lay;
  const int g = blockIdx.x, G = m.G, d = s.d, dl = s.dl, np = m.np;
  const int P1 = 2 + dl + m.T_all * m.rank + m.T_all;
  wmf_second_level(m, d, s.nbx, s.part + (int64_t)g * (np + 1) * 2 * s.nbx, s.dsl + g, s.dsl + G + (int64_t)g * d,
                   (int64_t)G * (1 + d), red, tot, dsum);
  const WmfOff o = wmf_off(m, s.rows, g);
  double* out = s.sums + (int64_t)g * (2 + P1);
  for (int x = threadIdx.x; x < P1; x += kWG)
    out[2 + x] = wmf_raw_grad(m, d, dl, x, s.raw, o, s.nat[g], s.nat + G + (int64_t)g * d, tot, dsum);
  if (threadIdx.x == 0) out[0] = tot[2 * np], out[1] = tot[2 * np + 1];
}

// The step over G problems, one workgroup of kWmfStepWG threads, a thread per raw element (strided).  Modes as
// k_wide_mt_fit_step.  Element x of row r of block q gets the sum of sums[g][its column] over the problems g with
// rows[q][g] == r, g ascending from 0.0 (k_mtg_step's order, fgp_multitask.hip); thread 0 adds the loss terms, g
// ascending.  The gradients come from sums alone, so an element is read, stepped and written by its own thread and no
// gradient is staged: no LDS.  The natural rows of the new parameters are gathered after a barrier.
constexpr int kWmfStepWG = 1024;
struct WmfBStep {
  Fit f;
  int G, d, dl, T_all, rank;
  int nrows[5];
  int rg_factor, rg_vtask;
  double w, lr;
  const int* rows;           // [5][G]
  const double* sums;        // [G][2 + P1]
  double* nat;               // scale [G], then lengthscales [G][d]
  double* gn;                // [G] = 1/2, then gl [G] = 1/2 w
  int* info;
};

__global__ __launch_bounds__(kWmfStepWG) void k_wide_mt_fit_bstep(WmfBStep s, int iter, int mode, int init) {
  const int tid = threadIdx.x;
  const Fit& f = s.f;
  const int G = s.G, d = s.d, dl = s.dl, n_params = f.n_params;
  if (mode != 0) {
    const int wid[5] = {1, dl, 1, s.T_all * s.rank, s.T_all};
    const int col0[5] = {0, 1, 1 + dl, 2 + dl, 2 + dl + s.T_all * s.rank};     // a block's first column of P1
    const int rgs[5] = {f.scale_rg, f.ls_rg, f.noise_rg, s.rg_factor, s.rg_vtask};
    const int S = 2 + col0[4] + s.T_all;
    for (int x = tid; x < n_params; x += kWmfStepWG) {
      int q = 0, base = 0;
      while (q < 4 && x >= base + s.nrows[q] * wid[q]) base += s.nrows[q] * wid[q], ++q;
      const int r = (x - base) / wid[q], c = 2 + col0[q] + (x - base) - r * wid[q];
      const int* rq = s.rows ? s.rows + (int64_t)q * G : nullptr;
      double gp = 0.0;
      for (int g = 0; g < G; ++g)
        if ((rq ? rq[g] : 0) == r) gp += s.sums[(int64_t)g * S + c];
      f.raw_hist[(int64_t)iter * n_params + x] = f.raw[x];
      f.grad_out[x] = gp;
      if (mode == 2 && rgs[q]) rprop_update(f, x, gp);
    }
    if (tid == 0) {
      double t1 = 0.0, ld = 0.0;
      for (int g = 0; g < G; ++g) t1 += s.sums[(int64_t)g * S], ld += s.sums[(int64_t)g * S + 1];
      const double t2 = s.w * ld;
      double* lh = f.loss_hist + (int64_t)iter * 3;
      lh[0] = 0.5 * (t1 + t2) + f.mll_const;
      lh[1] = t1;
      lh[2] = t2;
    }
    if (mode != 2) return;
    __syncthreads();
  } else {
    if (init)
      for (int x = tid; x < n_params; x += kWmfStepWG) {
        f.prev[x] = 0.0;
        f.step[x] = s.lr;
      }
    for (int b = tid; b < 2 * G; b += kWmfStepWG) s.gn[b] = b < G ? 0.5 : 0.5 * s.w;
    if (tid == 0) s.info[0] = 0;
  }
  for (int g = tid; g < G; g += kWmfStepWG) s.nat[g] = exp(f.raw[s.rows ? s.rows[g] : 0]);
  for (int e = tid; e < G * d; e += kWmfStepWG) {
    const int g = e / d, j = e - g * d;
    s.nat[G + e] = exp(f.raw[s.nrows[0] + (s.rows ? s.rows[G + g] : 0) * dl + (dl == d ? j : 0)]);
  }
}

// ------------------------------------------------------------------------------------------------ host side
struct WmfPlan {
  WmfLay lay;
  bool lat;
  int nbx;
  int n_params;
  int64_t L, rn;                                   // packed length, R nmin
  int log2n[kWmfT];
  // byte offsets into work
  size_t o_nat, o_gn, o_info, o_dsl, o_a, o_b, o_w, o_lams, o_fac, o_zinv, o_glp, o_z, o_ld, o_part, o_pb, bytes;
  size_t o_pl, pl_bytes;                           // GCV / CV: k_wide_mt_loss_sums' partials, after pb (MLL: empty)
  int G, P1;                                       // problems (>= 1), one problem's parameters
  int nrows[5];                                    // rows per parameter block (>= 1)
  const int* rows;                                 // G > 1: device [5][G] (may be NULL: row 0), else NULL
  size_t o_sums, sums_bytes;                       // G > 1: the per-problem totals [G][2 + P1], after pl (else empty)
};

static size_t wmf_align(size_t b) { return (b + 255) & ~(size_t)255; }

// bt: the batch descriptor whose `one` is a, or NULL (one problem)
static int wmf_plan(const char* fn, const fgp_wide_mt_fit_desc* a, WmfPlan& p,
                    const fgp_wide_mt_fit_batch_desc* bt = nullptr) {
  if (!a) return set_error(kErrInvalid, "%s: null pointer: desc", fn);
  static const int kNoRows[5] = {0, 0, 0, 0, 0};
  const int G_in = bt ? bt->G : 0;
  const int* nrows_in = bt ? bt->nrows : kNoRows;
  if (a->d <= FGP_MAX_D || a->d > FGP_WIDE_MAX_D)
    return set_error(kErrInvalid, "%s: d=%d outside %d..%d", fn, a->d, FGP_MAX_D + 1, FGP_WIDE_MAX_D);
  if (a->family != FGP_FAMILY_LATTICE && a->family != FGP_FAMILY_NET)
    return set_error(kErrInvalid, "%s: bad family %d", fn, a->family);
  const int T = a->layout.T;
  if (T < 1 || T > FGP_MT_MAX_TASKS)
    return set_error(kErrInvalid, "%s: T=%d (layout.T) outside 1..%d", fn, T, FGP_MT_MAX_TASKS);
  p = WmfPlan{};
  WmfLay& m = p.lay;
  m.T = T;
  m.np = T * (T + 1) / 2;
  int64_t L = 0, rn = 0;
  for (int k = 0; k < T; ++k) {
    const int64_t nk = a->layout.n[k];
    if (nk < 1 || (nk & (nk - 1)) || nk > ((int64_t)1 << kMaxLog2N))
      return set_error(kErrInvalid, "%s: n[%d]=%lld is not a power of two in 1..2^%d", fn, k, (long long)nk, kMaxLog2N);
    if (k > 0 && nk > a->layout.n[k - 1])
      return set_error(kErrInvalid, "%s: n[%d]=%lld above n[%d]: the tasks are not sorted by n descending", fn, k,
                       (long long)nk, k - 1);
    m.n[k] = nk;
    m.offk[k] = L;
    L += nk * (T - k);
    rn += nk;
    int lg = 0;
    while (((int64_t)1 << lg) < nk) ++lg;
    p.log2n[k] = lg;
  }
  if (rn / m.n[T - 1] > FGP_MT_MAX_ROWS)
    return set_error(kErrUnsupported, "%s: n spread too wide (%lld block rows)", fn, (long long)(rn / m.n[T - 1]));
  const int loss = a->loss_metric;
  if (loss != FGP_LOSS_MLL && loss != FGP_LOSS_GCV && loss != FGP_LOSS_CV)
    return set_error(kErrInvalid, "%s: loss_metric=%d not FGP_LOSS_MLL / _GCV / _CV", fn, loss);
  if (loss == FGP_LOSS_CV && !std::isfinite(a->cv_weight)) return set_error(kErrInvalid, "%s: cv_weight is not finite", fn);
  if (loss != FGP_LOSS_MLL && m.n[T - 1] != m.n[0])
    return set_error(kErrUnsupported, "%s: loss_metric=%d needs the same n in every task (n[0]=%lld, n[%d]=%lld)", fn, loss,
                     (long long)m.n[0], T - 1, (long long)m.n[T - 1]);
  if (loss == FGP_LOSS_CV && T == 1)
    return set_error(kErrUnsupported, "%s: loss_metric=FGP_LOSS_CV with T=1 (one task's inv_diag is another function)", fn);
  if (a->B < 1) return set_error(kErrInvalid, "%s: B=%d (at least one data vector)", fn, a->B);
  if (a->dl != 1 && a->dl != a->d) return set_error(kErrInvalid, "%s: dl=%d not in {1, d=%d}", fn, a->dl, a->d);
  if (a->rank < 0 || a->rank > FGP_MT_MAX_TASKS)
    return set_error(kErrInvalid, "%s: rank=%d outside 0..%d", fn, a->rank, FGP_MT_MAX_TASKS);
  if (a->T_all < T || a->T_all > FGP_MT_MAX_TASKS)
    return set_error(kErrInvalid, "%s: T_all=%d outside T=%d..%d", fn, a->T_all, T, FGP_MT_MAX_TASKS);
  for (int k = 0; k < T; ++k) {
    if (a->task[k] < 0 || a->task[k] >= a->T_all)
      return set_error(kErrInvalid, "%s: task[%d]=%d outside 0..T_all-1", fn, k, a->task[k]);
    m.task[k] = a->task[k];
  }
  for (int q = 0; q < m.np; ++q) {
    if (a->pair[q].P < 1) return set_error(kErrInvalid, "%s: pair[%d].P=%d (at least 1 multi-index pair)", fn, q, a->pair[q].P);
    if (a->pair[q].P > FGP_WIDE_MT_MAX_P)
      return set_error(kErrUnsupported, "%s: pair[%d].P=%d above %d (the generic loop covers more)", fn, q, a->pair[q].P,
                       FGP_WIDE_MT_MAX_P);
    if (a->pair[q].conj) m.conj[q >> 6] |= 1ull << (q & 63);
  }
  // parameter batches: G problems (0 = 1), nrows[q] rows of block q (0 = 1)
  if (G_in < 0) return set_error(kErrInvalid, "%s: G=%d negative", fn, G_in);
  p.G = G_in > 1 ? G_in : 1;
  p.rows = p.G > 1 ? bt->rows : nullptr;
  const int wid[5] = {1, a->dl, 1, a->T_all * a->rank, a->T_all};
  p.P1 = 0;
  int64_t npar = 0;
  for (int q = 0; q < 5; ++q) {
    if (nrows_in[q] < 0) return set_error(kErrInvalid, "%s: nrows[%d]=%d negative", fn, q, nrows_in[q]);
    p.nrows[q] = nrows_in[q] > 1 ? nrows_in[q] : 1;
    if (p.G == 1 && p.nrows[q] > 1)
      return set_error(kErrInvalid, "%s: nrows[%d]=%d rows for G=%d (one problem has one row per block)", fn, q,
                       nrows_in[q], G_in);
    p.P1 += wid[q];
    npar += (int64_t)p.nrows[q] * wid[q];
  }
  if (p.G > 1) {
    if (a->B != 1)
      return set_error(kErrUnsupported, "%s: B=%d with G=%d (a parameter batch has one data vector per problem)", fn, a->B,
                       G_in);
    if (loss != FGP_LOSS_MLL)
      return set_error(kErrUnsupported, "%s: loss_metric=%d with G=%d (a parameter batch fits the MLL)", fn, loss, G_in);
    if (p.G > kWmfMaxG) return set_error(kErrUnsupported, "%s: G=%d problems above %d", fn, G_in, kWmfMaxG);
    if (npar > kWmfMaxBatchParams)
      return set_error(kErrUnsupported, "%s: n_params=%lld (sum of nrows x width) above %d", fn, (long long)npar,
                       kWmfMaxBatchParams);
  }
  m.G = p.G;
  m.L = L;
  m.T_all = a->T_all;
  m.rank = a->rank;
  m.vtask_exp = a->vtask_exp != 0;
  m.noise_off = p.nrows[0] + p.nrows[1] * a->dl;
  m.f_off = m.noise_off + p.nrows[2];
  m.v_off = m.f_off + p.nrows[3] * a->T_all * a->rank;
  p.n_params = (int)npar;
  p.lat = a->family == FGP_FAMILY_LATTICE;
  p.L = L;
  p.rn = rn;
  p.nbx = (int)((m.n[0] + kWG - 1) / kWG);
  // every array G-fold (include/fgp_hip.h); G = 1: what one problem always had
  const size_t G = (size_t)p.G, B = (size_t)a->B, d = (size_t)a->d, np = (size_t)m.np, GL = G * (size_t)L;
  size_t o = 0;
  p.o_nat = o, o += wmf_align(8 * G * (1 + d));
  p.o_gn = o, o += wmf_align(8 * (G * B + G));
  p.o_info = o, o += 256;
  p.o_dsl = o, o += wmf_align(8 * np * G * (1 + d));
  p.o_a = o, o += wmf_align(8 * GL);                                     // k1, then u = dL/dk1
  p.o_b = o, o += wmf_align((p.lat ? 16 : 8) * GL);                      // lambda, then g~
  p.o_w = o, o += p.lat ? wmf_align(16 * GL) : 0;                        // the lattice transforms' scratch
  p.o_lams = o, o += wmf_align(16 * GL);
  p.o_fac = o, o += wmf_align(16 * GL);
  p.o_zinv = o, o += wmf_align(16 * GL);
  p.o_glp = o, o += wmf_align(16 * GL);
  p.o_z = o, o += wmf_align(16 * G * B * (size_t)rn);
  p.o_ld = o, o += wmf_align(8 * G * (size_t)m.n[T - 1]);
  p.o_part = o, o += wmf_align(8 * G * (np + 1) * 2 * (size_t)p.nbx);
  p.o_pb = o, o += wmf_align(8 * G * (1 + d) * (size_t)p.nbx);           // fgp_wide_mt_k1_bwd's partials
  p.pl_bytes = loss == FGP_LOSS_MLL ? 0 : 8 * (size_t)kWmfLossQ * (loss == FGP_LOSS_CV ? (size_t)T : 1) * (size_t)p.nbx;
  p.o_pl = o, o += wmf_align(p.pl_bytes);
  p.sums_bytes = p.G > 1 ? 8 * G * (size_t)(2 + p.P1) : 0;
  p.o_sums = o, o += wmf_align(p.sums_bytes);
  p.bytes = o;
  return kOk;
}

// One iteration as stages, in the order wmf_run enqueues them.  fgp_wide_mt_fit_stage (a test hook) enqueues one of them;
// wmf_run is the loop over the same function, so the run and the staged sequence are one piece of code.
enum WmfStage {
  kWmsPrologue = 0,   // k_wide_mt_fit_step in mode 0; the stage's mode is its init flag
  kWmsK1,             // fgp_wide_mt_k1 of every pair
  kWmsForward,        // lambda = ft(k1), one batched call per sorted task
  kWmsLams,           // k_wide_mt_lams
  kWmsBlocks,         // fgp_mt_factor, fgp_mt_solve, fgp_mt_selinv, fgp_mt_mll_grad (GCV / CV: the loss sums and gradient)
  kWmsContract,       // k_wide_mt_contract
  kWmsAdjoint,        // u = the adjoint transforms of g~
  kWmsK1Bwd,          // fgp_wide_mt_k1_bwd of every pair
  kWmsStep,           // k_wide_mt_fit_step in mode 1 or 2
  kWmsCount
};

// what every stage needs of the desc and the plan, formed once per run
struct WmfCtx {
  const fgp_wide_mt_fit_desc* a;
  const WmfPlan* p;
  WmfStep s;
  WmfSums bs;                                      // G > 1: the totals kernel's and the step's arguments
  WmfBStep bt;
  Switches sw;
  double *nat, *gn, *dsl, *A, *logdet, *part, *pb, *pl, *sums;
  int* info;
  char* Bf;
  void* W;
  double2 *lams, *fac, *zinv, *glp, *z;
  const double2* y;
  size_t esz;                                      // bytes of a lambda element
};

static WmfCtx wmf_ctx(const fgp_wide_mt_fit_desc* a, const WmfPlan& p) {
  WmfCtx c{};
  c.a = a, c.p = &p;
  char* w = static_cast<char*>(a->work);
  c.nat = reinterpret_cast<double*>(w + p.o_nat);
  c.gn = reinterpret_cast<double*>(w + p.o_gn);
  c.info = reinterpret_cast<int*>(w + p.o_info);
  c.dsl = reinterpret_cast<double*>(w + p.o_dsl);
  c.A = reinterpret_cast<double*>(w + p.o_a);
  c.Bf = w + p.o_b;
  c.W = p.lat ? static_cast<void*>(w + p.o_w) : nullptr;
  c.lams = reinterpret_cast<double2*>(w + p.o_lams);
  c.fac = reinterpret_cast<double2*>(w + p.o_fac);
  c.zinv = reinterpret_cast<double2*>(w + p.o_zinv);
  c.glp = reinterpret_cast<double2*>(w + p.o_glp);
  c.z = reinterpret_cast<double2*>(w + p.o_z);
  c.logdet = reinterpret_cast<double*>(w + p.o_ld);
  c.part = reinterpret_cast<double*>(w + p.o_part);
  c.pb = reinterpret_cast<double*>(w + p.o_pb);
  c.pl = reinterpret_cast<double*>(w + p.o_pl);
  c.esz = p.lat ? 16 : 8;
  WmfStep& s = c.s;
  s.f.n_params = p.n_params;
  s.f.raw = a->raw;
  s.f.prev = a->rprop_prev;
  s.f.step = a->rprop_step;
  s.f.grad_out = a->grad_out;
  s.f.loss_hist = a->loss_hist;
  s.f.raw_hist = a->raw_hist;
  s.f.scale_rg = a->rg_scale, s.f.ls_rg = a->rg_ls, s.f.noise_rg = a->rg_noise;
  s.f.mll_const = a->mll_const;
  s.f.eta_minus = a->eta_minus, s.f.eta_plus = a->eta_plus, s.f.step_min = a->step_min, s.f.step_max = a->step_max;
  s.lay = p.lay;
  s.d = a->d, s.dl = a->dl, s.B = a->B, s.nbx = p.nbx;
  s.rg_factor = a->rg_factor, s.rg_vtask = a->rg_vtask;
  s.w = a->logdet_weight, s.lr = a->lr;
  s.part = c.part, s.dsl = c.dsl, s.nat = c.nat, s.gn = c.gn, s.info = c.info;
  s.loss = a->loss_metric, s.cv_weight = a->cv_weight, s.pl = c.pl;
  c.sums = reinterpret_cast<double*>(w + p.o_sums);
  if (p.G > 1) {
    WmfSums& bs = c.bs;
    bs.lay = p.lay;
    bs.d = a->d, bs.dl = a->dl, bs.nbx = p.nbx;
    bs.raw = a->raw, bs.rows = p.rows, bs.part = c.part, bs.dsl = c.dsl, bs.nat = c.nat, bs.sums = c.sums;
    WmfBStep& bt = c.bt;
    bt.f = s.f;
    bt.G = p.G, bt.d = a->d, bt.dl = a->dl, bt.T_all = a->T_all, bt.rank = a->rank;
    for (int q = 0; q < 5; ++q) bt.nrows[q] = p.nrows[q];
    bt.rg_factor = a->rg_factor, bt.rg_vtask = a->rg_vtask;
    bt.w = a->logdet_weight, bt.lr = a->lr;
    bt.rows = p.rows, bt.sums = c.sums, bt.nat = c.nat, bt.gn = c.gn, bt.info = c.info;
  }
  c.sw = read_switches();
  c.y = static_cast<const double2*>(a->y);
  return c;
}

// GCV / CV: dL/dlams from the selected inverse and the solutions, in place of fgp_mt_mll_grad -- two launches, the sums'
// reduction between them
template <int FAM, bool CV>
static int wmf_loss_stage(const WmfCtx& c, hipStream_t st) {
  const fgp_wide_mt_fit_desc* a = c.a;
  const WmfPlan& p = *c.p;
  const dim3 gs((unsigned)p.nbx, CV ? (unsigned)p.lay.T : 1u);
  k_wide_mt_loss_sums<CV><<<gs, kWG, 0, st>>>(p.lay, a->B, c.zinv, c.z, p.nbx, c.pl);
  int rc = check_launch("k_wide_mt_loss_sums");
  if (rc != kOk) return rc;
  k_wide_mt_loss_grad<FAM, CV><<<(unsigned)p.nbx, kWG, 0, st>>>(p.lay, a->B, a->cv_weight, c.zinv, c.z, p.nbx, c.pl, c.glp);
  return check_launch("k_wide_mt_loss_grad");
}

// Stage `stage` of iteration `iter` (the history row the step writes).  mode: the prologue's init flag, the step's mode
// (1 or 2), otherwise unused.  The caller has validated stage and mode.
static int wmf_stage(const WmfCtx& c, int iter, int stage, int mode, hipStream_t st) {
  const fgp_wide_mt_fit_desc* a = c.a;
  const WmfPlan& p = *c.p;
  const WmfLay& m = p.lay;
  const int T = m.T, np = m.np, d = a->d, G = p.G;
  const fgp_mt_layout* lay = &a->layout;
  double *nat = c.nat, *A = c.A;
  const int* rows = p.rows;
  const int64_t nvec = (int64_t)G * a->B;          // data vectors: B of one problem, or one of each of G
  int rc = kOk;
  switch (stage) {
    case kWmsPrologue:
      if (G > 1) {
        k_wide_mt_fit_bstep<<<1, kWmfStepWG, 0, st>>>(c.bt, 0, 0, mode);
        return check_launch("k_wide_mt_fit_bstep");
      }
      k_wide_mt_fit_step<<<1, kWG, 0, st>>>(c.s, 0, 0, mode);
      return check_launch("k_wide_mt_fit_step");
    case kWmsK1:
      // k1 of every pair into A, the pair's G rows together (pair-major: G offk[k] + (l - k) G n_k; one problem: the
      // pair's packed offset): the pairs that share k lie contiguously
      for (int k = 0, q = 0; k < T && rc == kOk; ++k)
        for (int l = k; l < T && rc == kOk; ++l, ++q)
          rc = fgp_wide_mt_k1(a->pair[q].parts, m.n[k], d, a->pair[q].P, a->pair[q].ind, a->pair[q].cc, nat, nat + G, G,
                              A + (int64_t)G * (m.offk[k] + (int64_t)(l - k) * m.n[k]), st);
      return rc;
    case kWmsForward:
      // lambda = ft(k1), stable (AbstractFastGP.ft), the (T - k) G rows of sorted task k in one call
      for (int k = 0; k < T && rc == kOk; ++k) {
        const int64_t n = m.n[k], nr = (int64_t)(T - k) * G;
        const int lg = p.log2n[k];
        double* in = A + (int64_t)G * m.offk[k];
        void* out = c.Bf + c.esz * (size_t)G * (size_t)m.offk[k];
        if (!p.lat) rc = fgp_fwht(in, n, static_cast<double*>(out), nr, lg, 1, st);
        else if (use_r2c(c.sw, true, lg)) rc = fgp_fftbr_real(in, n, out, c.W, nr, lg, st);
        else rc = fgp_fftbr(in, n, 1, out, nr, lg, 1, st);
      }
      return rc;
    case kWmsLams: {
      const dim3 gl((unsigned)p.nbx, (unsigned)np, (unsigned)G);
      if (p.lat) k_wide_mt_lams<0><<<gl, kWG, 0, st>>>(m, a->raw, rows, c.Bf, c.lams);
      else k_wide_mt_lams<1><<<gl, kWG, 0, st>>>(m, a->raw, rows, c.Bf, c.lams);
      return check_launch("k_wide_mt_lams");
    }
    case kWmsBlocks:
      // the structured factor, the solves of the B vectors, the selected inverse and dL/dlams (fgp_multitask.hip); a
      // non-positive pivot sets info and counts as log|pivot|, as in the generic loop and MtGeneralEngine
      rc = fgp_mt_factor(lay, c.lams, G, c.fac, c.logdet, c.info, st);
      if (rc == kOk) rc = fgp_mt_solve(lay, c.fac, G, c.y, p.rn, nvec, c.z, st);
      if (rc == kOk) rc = fgp_mt_selinv(lay, c.fac, G, c.zinv, st);
      if (rc != kOk) return rc;
      if (a->loss_metric == FGP_LOSS_MLL) return fgp_mt_mll_grad(lay, c.zinv, c.z, c.gn, c.gn + nvec, nvec, G, c.glp, st);
      if (a->loss_metric == FGP_LOSS_CV) return p.lat ? wmf_loss_stage<0, true>(c, st) : wmf_loss_stage<1, true>(c, st);
      return p.lat ? wmf_loss_stage<0, false>(c, st) : wmf_loss_stage<1, false>(c, st);
    case kWmsContract: {
      const dim3 gc((unsigned)p.nbx, (unsigned)np + 1, (unsigned)G);
      if (p.lat)
        k_wide_mt_contract<0><<<gc, kWG, 0, st>>>(m, a->raw, rows, c.glp, c.Bf, c.y, c.z, (int64_t)a->B * p.rn, c.logdet,
                                                  p.nbx, c.part);
      else
        k_wide_mt_contract<1><<<gc, kWG, 0, st>>>(m, a->raw, rows, c.glp, c.Bf, c.y, c.z, (int64_t)a->B * p.rn, c.logdet,
                                                  p.nbx, c.part);
      return check_launch("k_wide_mt_contract");
    }
    case kWmsAdjoint:
      // u = dL/dk1: the adjoint transform of g~ (lattice: the real part), batched as the forward
      for (int k = 0; k < T && rc == kOk; ++k) {
        const int64_t n = m.n[k], nr = (int64_t)(T - k) * G;
        const int lg = p.log2n[k];
        double* out = A + (int64_t)G * m.offk[k];
        void* in = c.Bf + c.esz * (size_t)G * (size_t)m.offk[k];
        if (!p.lat) rc = fgp_fwht(static_cast<const double*>(in), n, out, nr, lg, 1, st);
        else if (use_r2c(c.sw, true, lg)) rc = fgp_ifftbr_real(in, n, nullptr, 0, out, n, c.W, nr, lg, st);
        else rc = fgp_ifftbr(in, n, out, 1, c.W, nr, lg, 1, st);
      }
      return rc;
    case kWmsK1Bwd:
      // pair q's dscale [G], then dls [G][d]
      for (int k = 0, q = 0; k < T && rc == kOk; ++k)
        for (int l = k; l < T && rc == kOk; ++l, ++q)
          rc = fgp_wide_mt_k1_bwd(a->pair[q].parts, m.n[k], d, a->pair[q].P, a->pair[q].ind, a->pair[q].cc, nat, nat + G, G,
                                  A + (int64_t)G * (m.offk[k] + (int64_t)(l - k) * m.n[k]),
                                  c.dsl + (int64_t)q * G * (1 + d), c.dsl + (int64_t)q * G * (1 + d) + G, c.pb, st);
      return rc;
    default:
      if (G > 1) {
        k_wide_mt_fit_sums<<<(unsigned)G, kWG, 0, st>>>(c.bs);
        rc = check_launch("k_wide_mt_fit_sums");
        if (rc != kOk) return rc;
        k_wide_mt_fit_bstep<<<1, kWmfStepWG, 0, st>>>(c.bt, iter, mode, 0);
        return check_launch("k_wide_mt_fit_bstep");
      }
      k_wide_mt_fit_step<<<1, kWG, 0, st>>>(c.s, iter, mode, 0);
      return check_launch("k_wide_mt_fit_step");
  }
}

static int wmf_run(const fgp_wide_mt_fit_desc* a, const WmfPlan& p, int iter0, int iters, int final_no_update,
                   hipStream_t st) {
  const WmfCtx c = wmf_ctx(a, p);
  int rc = wmf_stage(c, 0, kWmsPrologue, iter0 == 0 && a->lr > 0.0, st);
  for (int it = 0; it < iters && rc == kOk; ++it) {
    const bool last = it + 1 == iters;
    for (int stage = kWmsK1; stage < kWmsCount && rc == kOk; ++stage)
      rc = wmf_stage(c, iter0 + it, stage, stage == kWmsStep ? ((last && final_no_update) ? 1 : 2) : 0, st);
  }
  return rc;
}

// what fgp_wide_mt_fit_run and fgp_wide_mt_fit_stage validate beyond the plan
static int wmf_check(const char* fn, const fgp_wide_mt_fit_desc* desc, const WmfPlan& p) {
  const struct {
    const void* ptr;
    const char* name;
  } ptrs[] = {{desc->y, "y"},
              {desc->raw, "raw"},
              {desc->rprop_prev, "rprop_prev"},
              {desc->rprop_step, "rprop_step"},
              {desc->loss_hist, "loss_hist"},
              {desc->raw_hist, "raw_hist"},
              {desc->grad_out, "grad_out"},
              {desc->work, "work"}};
  for (const auto& q : ptrs)
    if (!q.ptr) return set_error(kErrInvalid, "%s: null pointer: %s", fn, q.name);
  for (int q = 0; q < p.lay.np; ++q) {
    const fgp_wide_mt_pair& pr = desc->pair[q];
    if (!pr.parts) return set_error(kErrInvalid, "%s: null pointer: pair[%d].parts", fn, q);
    if (!pr.ind) return set_error(kErrInvalid, "%s: null pointer: pair[%d].ind", fn, q);
    if (!pr.cc) return set_error(kErrInvalid, "%s: null pointer: pair[%d].cc", fn, q);
    // every pair's spec is checked here, before the first launch (fgp_wide_mt_k1 takes it by value: nothing to upload)
    for (int e = 0; e < pr.P * desc->d; ++e)
      if (pr.ind[e] != 0 && pr.ind[e] != 1)
        return set_error(kErrInvalid, "%s: pair[%d].ind[%d][%d]=%d is not 0 or 1", fn, q, e / desc->d, e % desc->d, pr.ind[e]);
  }
  return kOk;
}

// The entry points, for one problem (bt NULL) and for a batch descriptor (a = &bt->one)
static int wmf_api_work(const char* fn, const fgp_wide_mt_fit_desc* a, const fgp_wide_mt_fit_batch_desc* bt, int64_t* bytes) {
  WmfPlan p;
  int rc = wmf_plan(fn, a, p, bt);
  if (rc != kOk) return rc;
  if (!bytes) return set_error(kErrInvalid, "%s: null pointer: bytes", fn);
  *bytes = (int64_t)p.bytes;
  return kOk;
}

static int wmf_api_run(const char* fn, const fgp_wide_mt_fit_desc* desc, const fgp_wide_mt_fit_batch_desc* bt, int iter0,
                       int iters, int final_no_update, void* stream) {
  WmfPlan p;
  int rc = wmf_plan(fn, desc, p, bt);
  if (rc != kOk) return rc;
  rc = wmf_check(fn, desc, p);
  if (rc != kOk) return rc;
  if (iters < 0) return set_error(kErrInvalid, "%s: iters=%d negative", fn, iters);
  if (iter0 < 0) return set_error(kErrInvalid, "%s: iter0=%d negative", fn, iter0);
  if (((uintptr_t)desc->y | (uintptr_t)desc->work) & 15)
    return set_error(kErrInvalid, "%s: y and work must be 16-byte aligned", fn);
  if (iters == 0) return kOk;
  return wmf_run(desc, p, iter0, iters, final_no_update, (hipStream_t)stream);
}

static int wmf_api_work_layout(const char* fn, const fgp_wide_mt_fit_desc* a, const fgp_wide_mt_fit_batch_desc* bt,
                               int64_t offsets[15]) {
  WmfPlan p;
  int rc = wmf_plan(fn, a, p, bt);
  if (rc != kOk) return rc;
  if (!offsets) return set_error(kErrInvalid, "%s: null pointer: offsets", fn);
  const size_t o[15] = {p.o_nat,  p.o_gn,   p.o_info, p.o_dsl, p.o_a,  p.o_b,    p.o_w, p.o_lams,
                        p.o_fac, p.o_zinv, p.o_glp,  p.o_z,   p.o_ld, p.o_part, p.o_pb};
  for (int i = 0; i < 15; ++i) offsets[i] = (int64_t)o[i];
  return kOk;
}

static int wmf_api_stage(const char* fn, const fgp_wide_mt_fit_desc* desc, const fgp_wide_mt_fit_batch_desc* bt, int iter,
                         int stage, int mode, void* stream) {
  WmfPlan p;
  int rc = wmf_plan(fn, desc, p, bt);
  if (rc != kOk) return rc;
  rc = wmf_check(fn, desc, p);
  if (rc != kOk) return rc;
  if (((uintptr_t)desc->y | (uintptr_t)desc->work) & 15)
    return set_error(kErrInvalid, "%s: y and work must be 16-byte aligned", fn);
  if (iter < 0) return set_error(kErrInvalid, "%s: iter=%d negative", fn, iter);
  if (stage < 0 || stage >= kWmsCount) return set_error(kErrInvalid, "%s: stage=%d outside 0..%d", fn, stage, kWmsCount - 1);
  if (stage == kWmsPrologue) {
    if (mode != 0 && mode != 1) return set_error(kErrInvalid, "%s: mode=%d of the prologue is not 0 or 1 (init)", fn, mode);
    if (mode == 1 && !(desc->lr > 0.0)) return set_error(kErrInvalid, "%s: mode=1 (init) needs lr > 0", fn);
  } else if (stage == kWmsStep) {
    if (mode != 1 && mode != 2) return set_error(kErrInvalid, "%s: mode=%d of the step is not 1 or 2", fn, mode);
  } else if (mode != 0) {
    return set_error(kErrInvalid, "%s: mode=%d of stage %d is not 0", fn, mode, stage);
  }
  const WmfCtx c = wmf_ctx(desc, p);
  return wmf_stage(c, iter, stage, mode, (hipStream_t)stream);
}

}  // namespace fgp

using namespace fgp;

extern "C" {

int fgp_wide_mt_fit_work(const fgp_wide_mt_fit_desc* desc, int64_t* bytes) {
  return wmf_api_work("fgp_wide_mt_fit_work", desc, nullptr, bytes);
}

int fgp_wide_mt_fit_run(const fgp_wide_mt_fit_desc* desc, int iter0, int iters, int final_no_update, void* stream) {
  return wmf_api_run("fgp_wide_mt_fit_run", desc, nullptr, iter0, iters, final_no_update, stream);
}

int fgp_wide_mt_fit_work_layout(const fgp_wide_mt_fit_desc* desc, int64_t offsets[15]) {
  return wmf_api_work_layout("fgp_wide_mt_fit_work_layout", desc, nullptr, offsets);
}

int fgp_wide_mt_fit_loss_layout(const fgp_wide_mt_fit_desc* desc, int64_t offsets[2]) {
  WmfPlan p;
  int rc = wmf_plan("fgp_wide_mt_fit_loss_layout", desc, p);
  if (rc != kOk) return rc;
  if (!offsets) return set_error(kErrInvalid, "fgp_wide_mt_fit_loss_layout: null pointer: offsets");
  offsets[0] = (int64_t)p.o_pl;
  offsets[1] = (int64_t)p.pl_bytes;
  return kOk;
}

int fgp_wide_mt_fit_stage(const fgp_wide_mt_fit_desc* desc, int iter, int stage, int mode, void* stream) {
  return wmf_api_stage("fgp_wide_mt_fit_stage", desc, nullptr, iter, stage, mode, stream);
}

// ---- the batch descriptor's counterparts
#define WMF_BATCH_ONE(fn)                                                        \
  if (!desc) return set_error(kErrInvalid, "%s: null pointer: desc", fn);       \
  const fgp_wide_mt_fit_desc* one = &desc->one

int fgp_wide_mt_fit_batch_work(const fgp_wide_mt_fit_batch_desc* desc, int64_t* bytes) {
  WMF_BATCH_ONE("fgp_wide_mt_fit_batch_work");
  return wmf_api_work("fgp_wide_mt_fit_batch_work", one, desc, bytes);
}

int fgp_wide_mt_fit_batch_run(const fgp_wide_mt_fit_batch_desc* desc, int iter0, int iters, int final_no_update,
                              void* stream) {
  WMF_BATCH_ONE("fgp_wide_mt_fit_batch_run");
  return wmf_api_run("fgp_wide_mt_fit_batch_run", one, desc, iter0, iters, final_no_update, stream);
}

int fgp_wide_mt_fit_batch_work_layout(const fgp_wide_mt_fit_batch_desc* desc, int64_t offsets[15]) {
  WMF_BATCH_ONE("fgp_wide_mt_fit_batch_work_layout");
  return wmf_api_work_layout("fgp_wide_mt_fit_batch_work_layout", one, desc, offsets);
}

int fgp_wide_mt_fit_batch_stage(const fgp_wide_mt_fit_batch_desc* desc, int iter, int stage, int mode, void* stream) {
  WMF_BATCH_ONE("fgp_wide_mt_fit_batch_stage");
  return wmf_api_stage("fgp_wide_mt_fit_batch_stage", one, desc, iter, stage, mode, stream);
}

int fgp_wide_mt_fit_batch_layout(const fgp_wide_mt_fit_batch_desc* desc, int64_t offsets[2]) {
  WMF_BATCH_ONE("fgp_wide_mt_fit_batch_layout");
  WmfPlan p;
  int rc = wmf_plan("fgp_wide_mt_fit_batch_layout", one, p, desc);
  if (rc != kOk) return rc;
  if (!offsets) return set_error(kErrInvalid, "fgp_wide_mt_fit_batch_layout: null pointer: offsets");
  offsets[0] = (int64_t)p.o_sums;
  offsets[1] = (int64_t)p.sums_bytes;
  return kOk;
}
#undef WMF_BATCH_ONE

}  // extern "C"
