// The active-learning entries of the C ABI, for DenseGP_GPU and MultiOutputGP_GPU: the posterior cross covariance of two point sets and the
// ALC design criterion, one pick at a time or in greedy batches (predict_cov, alc, alc_batch / AlcBatch of analysis.h)
#include "analysis.h"
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
    predict_cov(*h->eng, {h->idx}, X1, m1, X2, m2, max_slots, cov_out);
  });
}
int mogp_densegp_alc(mogp_densegp* h, const double* candidates, int m_c, const double* reference, int m_r, int D, const double* weights,
                     const double* noise, int max_slots, int max_points, double* reduction_out, double* cand_var_out, double* ref_var_out,
                     int* degenerate_out) {
  return on_engine_device(h, [&] {
    check_D(D, h->eng);
    check_fit(h);
    alc(*h->eng, {h->idx}, candidates, m_c, reference, m_r, weights, noise, max_slots, max_points, reduction_out, cand_var_out, ref_var_out,
                degenerate_out);
  });
}
// every part: its fitted emulators in one predict_cov, the rows of the others NaN
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
                [&](const std::vector<Rows>& a) { predict_cov(*e, ids, X1, m1, X2, m2, max_slots, a[0].d()); });
    });
  });
}
// every part: its fitted emulators in one alc, the rows of the others NaN and degenerate = 0
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
                  alc(*e, ids, candidates, m_c, reference, m_r, weights, a[0].d(), max_slots, max_points, a[1].d(), a[2].d(), a[3].d(), a[4].i());
                });
    });
  });
}

int mogp_densegp_alc_batch(mogp_densegp* h, const double* candidates, int m, int n_forced, const double* reference, int m_r, int D,
                           const double* weights, const double* noise, int n_points, int max_slots, int* picks_out, double* pick_red_out,
                           double* red_out, int* deg_out, double* cand_var_out, double* ref_var_out, double* ref_var_after_out, double* iv_out) {
  return on_engine_device(h, [&] {
    check_D(D, h->eng);
    check_fit(h);
    alc_batch(*h->eng, {h->idx}, candidates, m, n_forced, reference, m_r, weights, noise, n_points, max_slots,
                      {picks_out, pick_red_out, red_out, deg_out, cand_var_out, ref_var_out, ref_var_after_out, iv_out});
  });
}

// select_total = 0: every part runs its fitted emulators through alc_batch.  select_total = 1: one AlcBatch per part stays
// open over the steps; per step every part downloads its score rows, this layer sums red_e / IV_e over the fitted emulators of ALL parts in
// ascending emulator order (IV_e: the integrated variance before the step, from the same rows) and takes the arg-max -- ties to the lowest
// index, a masked candidate never, a NaN never --, and every part applies that pick.  The sum depends on the rows alone, not on the parts.
int mogp_mogp_alc_batch(mogp_mogp* h, const double* candidates, int m, int n_forced, const double* reference, int m_r, int D,
                        const double* weights, const double* noise, int n_points, int select_total, int max_slots, int* picks_out,
                        double* pick_red_out, double* red_out, int* deg_out, double* cand_var_out, double* ref_var_out,
                        double* ref_var_after_out, double* iv_out, int* total_picks_out) {
  return guarded([&] {
    check_model("alc_batch", h, D);
    if (!candidates || !reference || !weights || !picks_out || !pick_red_out || !cand_var_out || !ref_var_out || !ref_var_after_out || !iv_out ||
        (select_total && !total_picks_out))
      throw std::runtime_error("alc_batch: null buffer");
    if (m < 1 || m_r < 1) throw std::runtime_error("alc_batch: at least one point is needed in each set");
    if (n_forced < 0 || n_forced > m) throw std::runtime_error("alc_batch: the pending points are a prefix of the candidates");
    if (n_points < 1) throw std::runtime_error("alc_batch: n_points must be at least 1");
    if (n_points > m - n_forced) throw std::runtime_error("alc_batch: n_points must not exceed the number of candidates");
    const int T = n_forced + n_points;
    const size_t M = (size_t)m, mr = (size_t)m_r, TM = (size_t)T * M;
    // the rows of one part in the caller's arrays (picks: the caller presets the rows of emulators that are not fit)
    const auto part_rows = [&](size_t lo) {
      return std::vector<Rows>{Rows::in(noise ? noise + lo : nullptr, 1),
                               Rows::out(picks_out + lo * T, (size_t)T, false),
                               Rows::out(pick_red_out + lo * T, (size_t)T, true),
                               Rows::out(red_out ? red_out + lo * TM : nullptr, TM, true),
                               Rows::out(deg_out ? deg_out + lo * TM : nullptr, TM, true),
                               Rows::out(cand_var_out + lo * M, M, true),
                               Rows::out(ref_var_out + lo * mr, mr, true),
                               Rows::out(ref_var_after_out + lo * mr, mr, true),
                               Rows::out(iv_out + lo * (T + 1), (size_t)T + 1, true)};
    };
    const auto as_out = [](const std::vector<Rows>& a) {
      return AlcBatchOut{a[1].i(), a[2].d(), a[3].d(), a[4].i(), a[5].d(), a[6].d(), a[7].d(), a[8].d()};
    };
    if (!select_total) {
      for_parts(h, [&](mogp_part& p, int) {
        Engine* e = p.eng.get();
        const std::vector<int> ids = fitted_ids(e);
        with_rows(e->B, ids, part_rows((size_t)p.lo), [&](const std::vector<Rows>& a) {
          alc_batch(*e, ids, candidates, m, n_forced, reference, m_r, weights, a[0].d(), n_points, max_slots, as_out(a));
        });
      });
      return;
    }
    // compact rows of every part's fitted emulators, kept on the host for the whole call
    struct PartRun {
      std::vector<int> ids, picks, deg, row_deg;
      std::vector<double> tau, pick_red, red, cand_var, ref_var, ref_var_after, iv, row_red, iv_now;
      std::unique_ptr<AlcBatch> run;
    };
    const int np = (int)h->parts.size();
    std::vector<PartRun> pr((size_t)np);
    // every part is closed on its own device, whatever happens
    struct CloseRuns {
      mogp_mogp* h;
      std::vector<PartRun>& pr;
      ~CloseRuns() {
        for (size_t k = 0; k < pr.size(); ++k) {
          if (!pr[k].run) continue;
          try {
            DeviceGuard g(h->parts[k].device);
            pr[k].run.reset();
          } catch (...) {
            pr[k].run.reset();
          }
        }
      }
    } close_runs{h, pr};
    for_parts(h, [&](mogp_part& p, int k) {
      Engine* e = p.eng.get();
      PartRun& r = pr[(size_t)k];
      r.ids = fitted_ids(e);
      const size_t nf = r.ids.size();
      if (nf == 0) return;
      std::vector<double> nz(nf);
      if (noise)
        for (size_t s = 0; s < nf; ++s) nz[s] = noise[(size_t)p.lo + r.ids[s]];
      alc_batch_check(*e, r.ids, candidates, m, n_forced, reference, m_r, weights, noise ? nz.data() : nullptr, n_points, 0, r.tau);
      alc_batch_slots(*e, (long)nf, m, m_r, T, 0, true);
      r.picks.assign(nf * T, -1), r.pick_red.assign(nf * T, 0.), r.cand_var.resize(nf * M), r.ref_var.resize(nf * mr);
      r.ref_var_after.resize(nf * mr), r.iv.resize(nf * (T + 1)), r.row_red.resize(nf * M), r.row_deg.resize(nf * M), r.iv_now.resize(nf);
      if (red_out) r.red.resize(nf * TM);
      if (deg_out) r.deg.resize(nf * TM);
      r.run.reset(new AlcBatch(*e, r.ids, r.tau.data(), candidates, m, n_forced, reference, m_r, weights, n_points,
                                       {r.picks.data(), r.pick_red.data(), red_out ? r.red.data() : nullptr, deg_out ? r.deg.data() : nullptr,
                                        r.cand_var.data(), r.ref_var.data(), r.ref_var_after.data(), r.iv.data()}));
      for (size_t s = 0; s < nf; ++s) {
        double a = 0.;
        for (size_t j = 0; j < mr; ++j) a += weights[j] * r.ref_var[s * mr + j];
        r.iv_now[s] = a;
      }
    });
    std::vector<char> masked(M, 0);
    std::vector<double> score(M);
    for (int t = 0; t < T; ++t) {
      for_parts(h, [&](mogp_part&, int k) {
        PartRun& r = pr[(size_t)k];
        if (r.run) r.run->scores_to_host(t, r.row_red.data(), r.row_deg.data());
      });
      int pick = -1;
      if (t < n_forced) {
        pick = t;
      } else {
        std::fill(score.begin(), score.end(), 0.);
        for (int k = 0; k < np; ++k) {       // parts hold ascending blocks of emulators
          const PartRun& r = pr[(size_t)k];
          for (size_t s = 0; s < r.ids.size(); ++s) {
            if (!(r.iv_now[s] > 0.)) continue;          // nothing left to reduce for this emulator
            for (size_t i = 0; i < M; ++i) score[i] += r.row_red[s * M + i] / r.iv_now[s];
          }
        }
        double best = 0.;
        for (size_t i = 0; i < M; ++i)
          if (!masked[i] && score[i] > best) {
            best = score[i];
            pick = (int)i;
          }
      }
      total_picks_out[t] = pick;
      if (pick < 0) {                      // the batch has stopped: the later steps pick nothing either
        for (int u = t + 1; u < T; ++u) total_picks_out[u] = -1;
        break;
      }
      masked[(size_t)pick] = 1;
      for (int k = 0; k < np; ++k) {
        PartRun& r = pr[(size_t)k];
        for (size_t s = 0; s < r.ids.size(); ++s) r.iv_now[s] -= r.row_red[s * M + pick];
      }
      for_parts(h, [&](mogp_part&, int k) {
        PartRun& r = pr[(size_t)k];
        if (r.run) r.run->apply(t, pick);
      });
    }
    for_parts(h, [&](mogp_part& p, int k) {
      PartRun& r = pr[(size_t)k];
      Engine* e = p.eng.get();
      if (r.run) {
        r.run->finish();
        r.run.reset();
      }
      with_rows(e->B, r.ids, part_rows((size_t)p.lo), [&](const std::vector<Rows>& a) {
        const size_t nf = r.ids.size();
        std::memcpy(a[1].p, r.picks.data(), nf * T * sizeof(int));
        std::memcpy(a[2].p, r.pick_red.data(), nf * T * sizeof(double));
        if (a[3].p) std::memcpy(a[3].p, r.red.data(), nf * TM * sizeof(double));
        if (a[4].p) std::memcpy(a[4].p, r.deg.data(), nf * TM * sizeof(int));
        std::memcpy(a[5].p, r.cand_var.data(), nf * M * sizeof(double));
        std::memcpy(a[6].p, r.ref_var.data(), nf * mr * sizeof(double));
        std::memcpy(a[7].p, r.ref_var_after.data(), nf * mr * sizeof(double));
        std::memcpy(a[8].p, r.iv.data(), nf * (T + 1) * sizeof(double));
      });
    });
  });
}

}  // extern "C"
