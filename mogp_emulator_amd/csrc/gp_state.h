// GPState: what the engine knows on the host about one emulator -- hyper-parameters, priors, the last log-posterior and which of the
// device buffers hold something usable for them.  Host-only (no HIP), so that tests/c/gp_state_check.cpp can sweep the transitions.
#pragma once
#include <stdexcept>
#include <string>
#include <vector>

#include "hostmath.h"

namespace mogp {

struct GPState {
  std::vector<double> data;      // n_data: corr_raw (NC), log sigma^2, [log nugget]
  std::vector<double> meanp;     // n_mean
  bool has_data = false;
  int nug_type = NUG_ADAPTIVE;
  double nug_size = 0.;          // adaptive: jitter found by the last fit; fixed: the constant
  Priors pri;
  double logpost = 0.;
  bool logpost_stale = false;    // the priors changed since `logpost` was computed (the factorisation itself is still valid)
  bool factored = false;         // A holds L (and y) for `data`
  bool linv = false, kinv = false;
  bool alpha = false;            // dAlpha holds K^-1 t (and the rows that go with it) for this factor
  double nugget_used = 0.;       // value actually added to the diagonal in the last factorisation
  // nugget="pivot": the factor in A, alpha, L^-1, K^-1 and this emulator's copy of the inputs are in pivoted order
  bool permuted = false;
  bool kinv_split = false;       // rank < n: Kinv was formed without the rows of L^-1 of the skipped pivots (kept in w2)
  int rank = 0;                  // pivots accepted by the last pivoted factorisation (n = full rank)
  std::vector<double> beta;      // analytic mean coefficients (q), GaussianProcess.py:669-670
  std::vector<double> LA;        // q x q lower Cholesky factor of A = H^T K^-1 H + B^-1
  // informative mean priors beta ~ N(b, B) of the analytic mean (Priors.py:423-581); empty = weak
  std::vector<double> mp_b, mp_Binv, mp_Binvb;
  double mp_logdetB = 0.;

  // The transitions of the cached state.  alpha, L^-1 and K^-1 belong to the factor: each is built from it on demand (Engine::ensure_alpha,
  // ensure_linv, ensure_kinv -- an objective-only evaluation builds none of them), is only read where `factored` holds, and goes with it.
  void drop_factor() { factored = linv = kinv = alpha = false; }   // A no longer holds a usable factor (nor the buffers what was built from it)
  void unfit() { has_data = false; drop_factor(); }        // hyper-parameters, nugget or mean priors changed: fit again
  // outcome of a fit: a good one keeps what was built from its factor since, a failed one has no factor to keep anything for
  void set_fit(bool ok) {
    has_data = ok;
    if (ok) factored = true;
    else drop_factor();
  }
  void priors_changed() { logpost_stale = true; }          // `logpost` was computed with the old priors; the factor is still valid
  // the buffers now hold what was built from the current factor (a logic error without one)
  void have_alpha() { need_factor("alpha"); alpha = true; }
  void have_linv() { need_factor("L^-1"); linv = true; kinv = false; }      // (the triangular inversion uses the K^-1 buffer as scratch)
  void have_kinv(bool split) { need_factor("K^-1"); if (!linv) throw std::logic_error("GPState: K^-1 without L^-1"); kinv = true; kinv_split = split; }

 private:
  void need_factor(const char* what) const {
    if (!factored) throw std::logic_error(std::string("GPState: ") + what + " without a factor");
  }
};

}  // namespace mogp
