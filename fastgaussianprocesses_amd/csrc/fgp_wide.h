// Wide inputs (9 <= d <= FGP_WIDE_MAX_D): the per-dimension table and the argument checks shared by the wide kernels
// of fgp_wide.hip and the wide row pass of the posterior variance's quadratic form (fgp_predict.hip).
#pragma once

#include "fgp_runtime.h"
#include "../../include/fgp_hip.h"

namespace fgp {

constexpr int kWD = FGP_WIDE_MAX_D;   // per-dimension table length

struct WideSpec {
  int order[kWD];
  double coef[kWD];
};

inline int wide_d_ok(const char* fn, int d) {
  if (d <= FGP_MAX_D || d > FGP_WIDE_MAX_D)
    return set_error(kErrInvalid, "%s: d=%d outside %d..%d (d <= %d: the entry point without _wide)", fn, d,
                     FGP_MAX_D + 1, FGP_WIDE_MAX_D, FGP_MAX_D);
  return kOk;
}

// Lattice: Bernoulli order 2 alpha and coefficient per dimension.  Net: Walsh order per dimension (1..4; order =
// NULL or 0 entries: 1), coefficients unused.
inline int wide_spec(const char* fn, int family, int d, const int* order, const double* coef, WideSpec& spec) {
  if (family != FGP_FAMILY_LATTICE && family != FGP_FAMILY_NET) return set_error(kErrInvalid, "%s: bad family %d", fn, family);
  const bool lat = family == FGP_FAMILY_LATTICE;
  if (lat && (!order || !coef)) return set_error(kErrInvalid, "%s: null pointer", fn);
  for (int j = 0; j < kWD; ++j) {
    if (lat) {
      spec.order[j] = j < d ? order[j] : 0;
      spec.coef[j] = j < d ? coef[j] : 0.0;
      if (j < d && (order[j] < 2 || order[j] > 8 || (order[j] & 1)))
        return set_error(kErrUnsupported, "%s: Bernoulli order %d unsupported", fn, order[j]);
    } else {
      spec.order[j] = (order && j < d && order[j] > 0) ? order[j] : 1;
      spec.coef[j] = 0.0;
      if (spec.order[j] > 4) return set_error(kErrUnsupported, "%s: Walsh order %d unsupported", fn, spec.order[j]);
    }
  }
  return kOk;
}

}  // namespace fgp
