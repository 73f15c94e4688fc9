// The active-learning entries of the C ABI, for DenseGP_GPU and MultiOutputGP_GPU: the posterior cross covariance of two point sets and the
// ALC design criterion (Engine::predict_cov, Engine::alc)
#include "capi_internal.h"

using namespace mogp;
using namespace mogp::capi;

namespace {

void check_fit(const mogp_densegp* h) {
  const GPState& g = h->eng->gp[h->idx];
  if (!(g.has_data && g.factored)) throw std::runtime_error("Hyperparameters have not been fit for this Gaussian Process");
}
// what needs no engine: the refusals of a whole model, before any part runs
void check_model(const char* who, const mogp_mogp* h, int D) {
  check_D(D, h->eng);
  const std::string p = std::string(who) + ": ";
  if (h->eng->analytic) throw std::runtime_error(p + "not available with analytic_mean=True (the covariance gains a term of the mean coefficients)");
  if (h->nug_type0 == NUG_PIVOT) throw std::runtime_error(p + "not available with nugget=\"pivot\" (a pivoted, possibly rank-deficient factor)");
}

}  // namespace

extern "C" {

int mogp_densegp_predict_cov(mogp_densegp* h, const double* X1, int m1, const double* X2, int m2, int D, int max_slots, double* cov_out) {
  return on_engine_device(h, [&] {
    check_D(D, h->eng);
    check_fit(h);
    h->eng->predict_cov({h->idx}, X1, m1, X2, m2, max_slots, cov_out);
  });
}
int mogp_densegp_alc(mogp_densegp* h, const double* candidates, int m_c, const double* reference, int m_r, int D, const double* weights,
                     const double* noise, int max_slots, int max_points, double* reduction_out, double* cand_var_out, double* ref_var_out,
                     int* degenerate_out) {
  return on_engine_device(h, [&] {
    check_D(D, h->eng);
    check_fit(h);
    h->eng->alc({h->idx}, candidates, m_c, reference, m_r, weights, noise, max_slots, max_points, reduction_out, cand_var_out, ref_var_out,
                degenerate_out);
  });
}
// every part: its fitted emulators in one Engine::predict_cov, the rows of the others NaN
int mogp_mogp_predict_cov(mogp_mogp* h, const double* X1, int m1, const double* X2, int m2, int D, int max_slots, double* cov_out) {
  return guarded([&] {
    check_model("predict_cov", h, D);
    if (!X1 || !cov_out) throw std::runtime_error("predict_cov: null buffer");
    if (m1 < 1 || (X2 && m2 < 1)) throw std::runtime_error("predict_cov: at least one point is needed in each set");
    const size_t mm = (size_t)m1 * (size_t)(X2 ? m2 : m1);
    for_parts(h, [&](mogp_part& p, int) {
      Engine* e = p.eng.get();
      const std::vector<int> ids = fitted_ids(e);
      with_rows(e->B, ids, {Rows::out(cov_out + (size_t)p.lo * mm, mm, true)},
                [&](const std::vector<Rows>& a) { e->predict_cov(ids, X1, m1, X2, m2, max_slots, a[0].d()); });
    });
  });
}
// every part: its fitted emulators in one Engine::alc, the rows of the others NaN and degenerate = 0
int mogp_mogp_alc(mogp_mogp* h, const double* candidates, int m_c, const double* reference, int m_r, int D, const double* weights,
                  const double* noise, int max_slots, int max_points, double* reduction_out, double* cand_var_out, double* ref_var_out,
                  int* degenerate_out) {
  return guarded([&] {
    check_model("alc_criterion", h, D);
    if (!candidates || !reference || !weights || !reduction_out || !cand_var_out || !ref_var_out || !degenerate_out)
      throw std::runtime_error("alc_criterion: null buffer");
    if (m_c < 1 || m_r < 1) throw std::runtime_error("alc_criterion: at least one point is needed in each set");
    const size_t mc = (size_t)m_c, mr = (size_t)m_r;
    for_parts(h, [&](mogp_part& p, int) {
      Engine* e = p.eng.get();
      const size_t lo = (size_t)p.lo;
      const std::vector<int> ids = fitted_ids(e);
      with_rows(e->B, ids,
                {Rows::in(noise ? noise + lo : nullptr, 1), Rows::out(reduction_out + lo * mc, mc, true), Rows::out(cand_var_out + lo * mc, mc, true),
                 Rows::out(ref_var_out + lo * mr, mr, true), Rows::out(degenerate_out + lo * mc, mc, true)},
                [&](const std::vector<Rows>& a) {
                  e->alc(ids, candidates, m_c, reference, m_r, weights, a[0].d(), max_slots, max_points, a[1].d(), a[2].d(), a[3].d(), a[4].i());
                });
    });
  });
}

}  // extern "C"
