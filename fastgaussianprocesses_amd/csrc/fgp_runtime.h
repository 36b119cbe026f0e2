// Host-side runtime shared by the fgp C-ABI entry points: error reporting, per-device twiddle tables, the
// run-time-int -> template-argument dispatcher, the kernel residency query and the A/B environment switches.
// Internal header (not part of the public C-ABI in include/fgp_hip.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace fgp {

constexpr int kMaxLog2N = 24;   // largest supported transform length 2^24

// Split of a length-2^m transform (m > 12) into N1 x N2 with N2 = 2^m2 rows-length, N1 = 2^m1.
inline int split_m2(int m) { return m - 4 < 12 ? m - 4 : 12; }

struct Tables {
  double2* tw4096 = nullptr;             // exp(-2 pi i k / 4096), k < 4096
  double2* twm[kMaxLog2N + 1] = {};      // for m > 12: exp(-2 pi i k / 2^m), k < 2^split_m2(m)
};

// Returns the (lazily initialised, stream-synchronised) tables of the current device.
const Tables* get_tables(hipStream_t stream);

int set_error(int code, const char* fmt, ...);

// Adjoint column pass of a [batch, 2^m] transform (m > 12), stable, unscaled: FFT (conj twiddle)
// when fft, else WHT columns.  Defined in fgp_transforms.hip; used by the fused backward.
int cols_adjoint_launch(bool fft, int m, const void* in, void* out, int64_t batch, const Tables* tb,
                        hipStream_t st);
int check_launch(const char* what);

enum Status : int {
  kOk = 0,
  kErrInvalid = -1,
  kErrUnsupported = -2,
  kErrHip = -3,
};

// ---------------------------------------------------------------- run-time int -> template argument
// dispatch_range<Lo, Hi>(v, fn) / dispatch_list<V...>(v, fn): fn(std::integral_constant<int, V>{}) for the V of
// the set that equals v, returning fn's status; kNoMatch (never a Status) when v is outside the set.
constexpr int kNoMatch = -1000;
template <int... Vs, typename Fn>
int dispatch_list(int v, Fn&& fn) {
  int rc = kNoMatch;
  (void)((v == Vs && ((rc = fn(std::integral_constant<int, Vs>{})), true)) || ...);
  return rc;
}
template <int Lo, int Hi, typename Fn>
int dispatch_range(int v, Fn&& fn) {
  if constexpr (Lo > Hi) return kNoMatch;
  else return v == Lo ? fn(std::integral_constant<int, Lo>{}) : dispatch_range<Lo + 1, Hi>(v, fn);
}
// rc of a dispatch whose callers validate v first: kNoMatch becomes kErrInvalid
int no_kernel(int rc, const char* what, int v);

// ---------------------------------------------------------------- residency and the dynamic-LDS limit
// Workgroups of `kernel` (block threads, dyn_lds bytes of dynamic LDS) resident at once on the current device:
// workgroups per CU x CUs, 0 when the query fails.  Queried once per (device, kernel, dyn_lds) and remembered,
// so a later launch inside a stream capture makes no query.  lds_limit > 0: raise_lds_limit first.
int64_t resident_workgroups(const void* kernel, int block, size_t dyn_lds, int lds_limit);
// Raises the kernel's dynamic-LDS limit above the 64 KB default, once per (device, kernel).
void raise_lds_limit(const void* kernel, int lds_limit);

// ---------------------------------------------------------------- A/B environment switches
// The library-global inputs of a launch sequence that come from the environment, parsed into the values the code
// branches on.  Read once per C-ABI call (read_switches: never cached, callers may change the environment
// between calls) and handed down; its bytes (zeroed padding) are part of the fit-graph key.
struct Switches {
  int spec_tile;        // FGP_SPEC_TILE: 0 = the per-wave kernel only, else 1
  int spec_slice_nb;    // FGP_SPEC_SLICE_NB: k blocks of the problem-slice tile kernel (>= 1), 0 = unset
  int spec_persist;     // FGP_SPEC_PERSIST: 1 = every iteration in one persistent k_spec_tile launch
  int spec_step_many;   // FGP_SPEC_STEP_MANY: 0 = the serial step of one loss over many problems, else 1
  int r2c;              // FGP_R2C: 0 = full-length lattice kernels, 1 = half-length (R2C), 2 (default) = R2C / real-even
};
Switches read_switches();
// lattices with n >= 2^17 take the half-length (R2C) kernels and their workspace layout
inline bool use_r2c(const Switches& sw, bool lattice, int log2n) { return lattice && log2n >= 17 && sw.r2c != 0; }

}  // namespace fgp
