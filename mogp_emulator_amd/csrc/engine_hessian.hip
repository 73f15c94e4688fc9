// Engine::hessian and its steps.  A member, unlike the analyses of analysis.h: it moves emulators to other thetas with eval, launches the
// gradient into the engine's own buffers and reads alpha and the targets.  The host algebra is hessian_assemble (hostmath.h), the sizing
// rules are plain arithmetic in predict_plan.h.
#include "engine_internal.h"

#include <cmath>
#include <limits>

namespace mogp {

// ---------------------------------------------------------------------------------------------
// Hessian of the negative log-posterior at per-emulator thetas (kernels_hess.hip, DESIGN.md section 3 "Hessian"): H holds one ld x ld
// row-major block per entry of ids, its leading n_theta x n_theta block filled (both triangles, exactly symmetric) and the rest of it
// NaN (an emulator narrower than ld), all of it NaN where the factorisation fails (ok = 0).  An emulator already fit at exactly theta is not evaluated again; one that was fit elsewhere is put back
// at its own theta afterwards, so its cached state is what it was.  The planes M_p are scratch of this call, taken per group of
// emulators within the prediction's chunk budget and freed before it returns.
// ---------------------------------------------------------------------------------------------

// the device scratch of one group of m emulators; `drained` comes last, so that the stream is drained before the buffers go when the
// group is left through an exception
struct Engine::HessianScratch {
  DevBuf<double> dXs, dMp, dTp, dTo, dPp, dPo, dV, dU, dZv;
  SyncOnUnwind drained;
  HessianScratch(size_t m, int NPh, int D, int TG, int PGR, hipStream_t st)
      : dXs(m * NPh * D), dMp(m * D * ((size_t)NPh * NPh)), dTp(m * TG * ((D + 1) * (D + 2))), dTo(m * ((D + 1) * (D + 2))), dPp(m * PGR * D * D),
        dPo(m * D * D), dV(m * D * NPh), dU(m * D * NPh), dZv(m * NPh), drained{st} {}
};

// the host copies of a group's sums (kept from one group to the next)
struct Engine::HessianSums {
  std::vector<double> go, To, Po, V, U, Zv;
};

// Brings the emulators of ids to their thetas: fine[k] = 1 where emulator ids[k] holds a factor at thetas[k] afterwards -- it was there
// already, or it was evaluated there --, before[k] = the theta a fitted emulator was moved away from (empty: nothing to put back).
// Every block of H is set to NaN on the way.
void Engine::hessian_move_to(const std::vector<int>& ids, const std::vector<const double*>& thetas, double* H, int ld, std::vector<int>& fine,
                             std::vector<std::vector<double>>& before) {
  const int nb = (int)ids.size();
  const double nan = std::numeric_limits<double>::quiet_NaN();
  std::vector<int> ev_ids, ev_pos;
  std::vector<const double*> ev_th;
  for (int k = 0; k < nb; ++k) {
    const int i = ids[k];
    const GPState& g = gp[i];
    const int P = n_theta(i);
    if (P > ld) throw std::runtime_error("logpost_hessian: the result buffer passed was too small");
    std::fill(H + (size_t)k * ld * ld, H + (size_t)(k + 1) * ld * ld, nan);
    const bool fit = g.has_data && g.factored;
    if (fit && !g.logpost_stale && std::equal(g.data.begin(), g.data.end(), thetas[k])) {
      fine[k] = 1;
      continue;
    }
    if (fit) before[k] = g.data;
    ev_ids.push_back(i);
    ev_pos.push_back(k);
    ev_th.push_back(thetas[k]);
  }
  if (!ev_ids.empty()) {
    std::vector<double> f(ev_ids.size());
    std::vector<int> okv(ev_ids.size());
    eval(ev_ids, ev_th, false, f.data(), nullptr, 0, okv.data());
    for (size_t e = 0; e < ev_ids.size(); ++e) fine[ev_pos[e]] = okv[e];
  }
}

// back to where the emulators were
void Engine::hessian_put_back(const std::vector<int>& ids, const std::vector<std::vector<double>>& before) {
  std::vector<int> rb_ids;
  std::vector<const double*> rb_th;
  for (size_t k = 0; k < ids.size(); ++k)
    if (!before[k].empty()) {
      rb_ids.push_back(ids[k]);
      rb_th.push_back(before[k].data());
    }
  if (!rb_ids.empty()) {
    std::vector<double> f(rb_ids.size());
    std::vector<int> okv(rb_ids.size());
    eval(rb_ids, rb_th, false, f.data(), nullptr, 0, okv.data());
  }
}

// the device sums of the emulators of grp (K^-1 is there): the gradient's, then scale, planes, trace, pair and vectors; six downloads,
// ONE synchronisation
void Engine::hessian_group_sums(const std::vector<int>& grp, HessianScratch& d, HessianSums& h) {
  const size_t m = grp.size();
  const int NPh = hess_np(n), TS = (D + 1) * (D + 2);
  upload_idx(grp);
  BatchView v = view((int)m);
  launch_grad(v, dGradPartial, dGradOut, stream);
  launch_hess_scale(v, d.dXs, stream);
  launch_hess_planes(v, d.dXs, d.dMp, stream);
  launch_hess_trace(v, d.dMp, d.dTp, d.dTo, stream);
  launch_hess_pair(v, d.dXs, d.dPp, d.dPo, stream);
  launch_hess_vectors(v, d.dMp, d.dV, d.dU, d.dZv, stream);
  h.To.resize(m * TS); h.Po.resize(m * D * D); h.V.resize(m * D * NPh); h.U.resize(m * D * NPh); h.Zv.resize(m * NPh);
  HIPCK(hipMemcpyAsync(h.go.data(), dGradOut, h.go.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
  HIPCK(hipMemcpyAsync(h.To.data(), d.dTo, h.To.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
  HIPCK(hipMemcpyAsync(h.Po.data(), d.dPo, h.Po.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
  HIPCK(hipMemcpyAsync(h.V.data(), d.dV, h.V.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
  HIPCK(hipMemcpyAsync(h.U.data(), d.dU, h.U.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
  HIPCK(hipMemcpyAsync(h.Zv.data(), d.dZv, h.Zv.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
  HIPCK(hipStreamSynchronize(stream));
  HIPCK(hipGetLastError());
}

void Engine::hessian(const std::vector<int>& ids, const std::vector<const double*>& thetas, double* H, int ld, int* ok) {
  const int nb = (int)ids.size();
  if (nb == 0) return;
  if (analytic) throw std::runtime_error("logpost_hessian: not available with analytic_mean=True (the mean coefficients are integrated out of theta)");
  if (n_mean() > 0) throw std::runtime_error("logpost_hessian: not available for a mean function with parameters in theta");
  if (kernel_type == 2) throw std::runtime_error("logpost_hessian: not available for the ProductMat52 kernel");
  for (int i : ids)
    if (gp[i].nug_type == NUG_PIVOT)
      throw std::runtime_error("logpost_hessian: not available with nugget=\"pivot\" (a pivoted, possibly rank-deficient factor)");
  std::vector<std::vector<double>> before(nb);      // theta of the emulators that have to be put back
  std::vector<int> fine(nb, 0);
  hessian_move_to(ids, thetas, H, ld, fine, before);
  std::vector<int> good, gpos;
  for (int k = 0; k < nb; ++k)
    if (fine[k]) {
      good.push_back(ids[k]);
      gpos.push_back(k);
    }
  if (!good.empty()) {
    ensure_alpha(good);
    ensure_kinv(good, true);
    const int NPh = hess_np(n), NQ = D + 3, TQ = D + 2, TS = (D + 1) * TQ, TG = hess_trace_groups(n), PGR = hess_pair_groups(n);
    const size_t gsz = hessian_group_size(ks_budget_bytes(), hessian_scratch_bytes(NPh, D, TG, PGR), good.size());
    HessianSums h;
    h.go.resize((size_t)B * NQ);
    std::vector<double> al(n), tt(n), dpr(NC + 2), Fd((size_t)TQ * TQ);
    for (size_t g0 = 0; g0 < good.size(); g0 += gsz) {
      const std::vector<int> grp(good.begin() + g0, good.begin() + std::min(good.size(), g0 + gsz));
      HessianScratch dev(grp.size(), NPh, D, TG, PGR, stream);      // (lives to the end of the iteration, as the planes always did)
      hessian_group_sums(grp, dev, h);
      for (size_t s = 0; s < grp.size(); ++s) {
        const int i = grp[s], k = gpos[g0 + s];
        const GPState& g = gp[i];
        HIPCK(hipMemcpy(al.data(), dAlpha + (size_t)i * RA * LD, n * sizeof(double), hipMemcpyDeviceToHost));
        HIPCK(hipMemcpy(tt.data(), dT + (size_t)i * n, n * sizeof(double), hipMemcpyDeviceToHost));
        const int P = n_theta(i);
        std::vector<double> Hm((size_t)P * P, 0.);
        g.pri.d2logpdtheta2(g.data, NC, g.nug_type, dpr.data());
        if (!hessian_assemble(n, D, NC, uniform(), g.nug_type == NUG_FIT, g.nugget_used, h.go.data() + (size_t)i * NQ, h.To.data() + s * TS,
                              h.Po.data() + s * D * D, h.V.data() + s * D * NPh, h.U.data() + s * D * NPh, NPh, h.Zv.data() + s * NPh, al.data(),
                              tt.data(), dpr.data(), Fd.data(), Hm.data())) {
          fine[k] = 0;
          continue;
        }
        for (int r = 0; r < P; ++r)
          for (int c = r; c < P; ++c) H[((size_t)k * ld + r) * ld + c] = H[((size_t)k * ld + c) * ld + r] = Hm[(size_t)r * P + c];
      }
    }
  }
  hessian_put_back(ids, before);
  if (ok)
    for (int k = 0; k < nb; ++k) ok[k] = fine[k];
}

}  // namespace mogp
