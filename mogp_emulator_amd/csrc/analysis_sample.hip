// Joint posterior draws (analysis.h has the contract, kernels_sample.hip the kernels, sample_plan of predict_plan.h the sizing).  Per pass of
// `slots` emulators:
//   1. sample_build: Sigma* and mu* with predict_full_cov's own launches; Sigma* stays on the device, mu* gets its mean-function terms on
//      the host and goes up again;
//   2. sample_factor: Sigma~ gathered into the ScratchFactor (sample_gather_kernel as the fill of its factor, L^-1 not formed), then
//      the jitter ladder on the host over the slots that failed -- they alone are gathered again, from the resident Sigma* --, then
//      sample_polish_kernel: the factor's diagonal from its finished rows with the correctly rounded square root;
//   3. sample_draws: per chunk of draws z uploaded or generated, z_out and Y = mu + L z downloaded; NaN rows where Sigma~ never factorised.
// The ScratchFactor and every buffer are scratch of the call.
#include "analysis.h"
#include "engine_internal.h"

#include <cmath>
#include <limits>

namespace mogp {

namespace {

// the buffers of a pass, sized for `slots` emulators and `draws` draws per chunk; the guards come last, so that both streams are drained
// before the buffers go when the call is left through an exception
struct SamplePass {
  int m, MP;
  long slots, zrows;
  DevBuf<double> dC, dDots, dMu, dShift, dZ, dY;
  DevBuf<int> dSrc;
  DevBuf<unsigned> dStreams;
  std::vector<int> good;             // per slot of the pass: Sigma~ factorised
  SyncOnUnwind drained_main, drained_sub;
  SamplePass(int m_, long slots_, long draws, int R, hipStream_t main_stream, hipStream_t sub_stream)
      : m(m_), MP((int)sample_mp(m_)), slots(slots_), zrows(sample_draw_rows(draws)), dC((size_t)slots_ * m_ * m_), dDots((size_t)slots_ * R * m_),
        dMu((size_t)slots_ * m_), dShift((size_t)slots_), dZ((size_t)slots_ * zrows * MP), dY((size_t)slots_ * zrows * m_), dSrc((size_t)slots_),
        dStreams((size_t)slots_), good((size_t)slots_, 0), drained_main{main_stream}, drained_sub{sub_stream} {}
};

// 1. Sigma* (p.dC) and mu* (mean_out, p.dMu) of the emulators of grp
void sample_build(Engine& eng, const std::vector<int>& grp, const double* Xs, const double* dXq, int m, SamplePass& p, double* mean_out) {
  hipStream_t stream = eng.stream;
  const int nb = (int)grp.size();
  eng.ensure_alpha(grp);
  eng.ensure_linv(grp);
  eng.upload_idx(grp);
  std::vector<double> dots((size_t)nb * eng.R * m);
  {
    DevBuf<double> dKf((size_t)nb * p.MP * eng.LD), dV((size_t)nb * eng.NP * p.MP);
    SyncOnUnwind drained{stream};
    eng.fullcov_launches(nb, dXq, m, p.MP, dKf, dV, p.dC, p.dDots);
    HIPCK(hipMemcpyAsync(dots.data(), p.dDots, dots.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
    HIPCK(hipStreamSynchronize(stream));
    HIPCK(hipGetLastError());
  }
  eng.fullcov_host_means(grp, Xs, m, dots.data(), mean_out, nullptr);
  HIPCK(hipMemcpyAsync(p.dMu, mean_out, (size_t)nb * m * sizeof(double), hipMemcpyHostToDevice, stream));
  HIPCK(hipStreamSynchronize(stream));        // the ScratchFactor reads Sigma* and mu* on its own stream
}

// 2. Sigma~ = L L^T in the slots 0 .. grp.size() - 1 of the ScratchFactor, the ladder over those that fail
void sample_factor(const Engine& eng, ScratchFactor& sub, const std::vector<int>& grp, bool include_nugget, double jitter, SamplePass& p,
                   double* jitter_used, int* ok) {
  const long cnt = (long)grp.size();
  const int m = p.m;
  hipStream_t st = sub.stream();
  std::vector<int> src((size_t)p.slots, -1), list((size_t)cnt), info;
  std::vector<double> shift((size_t)p.slots, 0.), nug((size_t)cnt), diag((size_t)m);
  for (long k = 0; k < cnt; ++k) {
    src[k] = list[k] = (int)k;
    nug[k] = include_nugget ? eng.nugget_size(grp[k]) : 0.;
    shift[k] = nug[k] + jitter;
    jitter_used[k] = jitter;
  }
  HIPCK(hipMemcpyAsync(p.dSrc, src.data(), src.size() * sizeof(int), hipMemcpyHostToDevice, st));
  const CovFill fill = [&](const BatchView& sv) {
    HIPCK(hipMemcpyAsync(p.dShift, shift.data(), shift.size() * sizeof(double), hipMemcpyHostToDevice, st));
    launch_sample_gather(sv, p.dC, p.dSrc, p.dShift, m, st);
  };
  auto failed_of = [&](const std::vector<int>& tried) {
    std::vector<int> f;
    for (int k : tried)
      if (info[k] != 0) f.push_back(k);
    return f;
  };
  sub.factor(fill, info, &list, false);
  std::vector<int> failed = failed_of(list);
  std::vector<double> mean_diag((size_t)cnt, 0.);
  for (int t = 0; t < SAMPLE_LADDER_RUNGS && !failed.empty(); ++t) {
    for (int k : failed) {
      if (t == 0) {       // the mean diagonal of Sigma*, read when the ladder first needs it
        HIPCK(hipMemcpy2D(diag.data(), sizeof(double), p.dC + (size_t)k * m * m, ((size_t)m + 1) * sizeof(double), sizeof(double), (size_t)m,
                          hipMemcpyDeviceToHost));
        double s = 0.;
        for (int j = 0; j < m; ++j) s += diag[j];
        mean_diag[k] = s / m;
      }
      const double delta = sample_ladder_delta(t, mean_diag[k]);
      jitter_used[k] = jitter + delta;
      shift[k] = nug[k] + jitter_used[k];
    }
    sub.factor(fill, info, &failed, false);
    failed = failed_of(failed);
  }
  // (src and shift on the device are those of every slot's last gather; a slot that never factorised is left alone by the kernel's test)
  launch_sample_polish(sub.factor_buffer(), sub.NP, (int)cnt, p.dC, p.dSrc, p.dShift, m, st);
  for (long k = 0; k < cnt; ++k) p.good[k] = 1;
  for (int k : failed) p.good[k] = 0;
  for (long k = 0; k < cnt; ++k) ok[k] = p.good[k];
}

// 3. the draws of the emulators [e0, e0 + cnt) of the call (slots 0 .. cnt - 1), chunk by chunk
void sample_draws(ScratchFactor& sub, long e0, long cnt, int m, int S, int Sc, unsigned long long seed, const double* z_in, bool z_per_emulator,
                  SamplePass& p, double* samples, double* z_out) {
  hipStream_t st = sub.stream();
  const size_t row = (size_t)m * sizeof(double), zpitch = (size_t)p.MP * sizeof(double), mm = (size_t)m;
  for (int s0 = 0; s0 < S; s0 += Sc) {
    const int sc = std::min(Sc, S - s0);
    if (z_in) {
      for (long k = 0; k < cnt; ++k) {
        const double* zsrc = z_in + ((z_per_emulator ? (size_t)(e0 + k) * S : 0) + s0) * mm;
        HIPCK(hipMemcpy2DAsync(p.dZ + (size_t)k * p.zrows * p.MP, zpitch, zsrc, row, row, sc, hipMemcpyHostToDevice, st));
      }
    } else {
      launch_sample_normals(p.dZ, (int)cnt, p.zrows, p.MP, m, sc, s0, seed, p.dStreams, st);
    }
    launch_sample_apply(sub.factor_buffer(), sub.NP, p.dZ, p.zrows, p.MP, p.dMu, m, sc, (int)cnt, p.dY, p.zrows, st);
    for (long k = 0; k < cnt; ++k) {
      const size_t o = ((size_t)(e0 + k) * S + s0) * mm;
      if (z_out) HIPCK(hipMemcpy2DAsync(z_out + o, row, p.dZ + (size_t)k * p.zrows * p.MP, zpitch, row, sc, hipMemcpyDeviceToHost, st));
      HIPCK(hipMemcpyAsync(samples + o, p.dY + (size_t)k * p.zrows * mm, (size_t)sc * row, hipMemcpyDeviceToHost, st));
    }
    HIPCK(hipStreamSynchronize(st));          // the next chunk overwrites Z and Y
    HIPCK(hipGetLastError());
  }
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (long k = 0; k < cnt; ++k)
    if (!p.good[k]) std::fill(samples + (size_t)(e0 + k) * S * mm, samples + (size_t)(e0 + k + 1) * S * mm, nan);
}

}  // namespace

void sample_posterior(Engine& eng, const std::vector<int>& ids, const unsigned* streams, const double* Xs, int m, int S, unsigned long long seed,
                      const double* z_in, bool z_per_emulator, bool include_nugget, double jitter, int max_slots, int max_draws,
                      double* samples, double* mean_out, double* z_out, double* jitter_used, int* ok) {
  const long E = (long)ids.size();
  if (E == 0) return;
  hipStream_t stream = eng.stream;
  const int D = eng.D, R = eng.R;
  eng.require_plain_fit("sample_posterior", ids, "its covariance term is finished on the host");
  if (!streams || !Xs || !samples || !mean_out || !jitter_used || !ok) throw std::runtime_error("sample_posterior: null buffer");
  if (m < 1) throw std::runtime_error("sample_posterior: at least one query point is needed");
  if (S < 1) throw std::runtime_error("sample_posterior: at least one draw is needed (n_draws = " + std::to_string(S) + ")");
  if (!(jitter >= 0.) || !std::isfinite(jitter)) throw std::runtime_error("sample_posterior: jitter must be a finite number that is not negative");
  if (max_slots < 0 || max_draws < 0) throw std::runtime_error("sample_posterior: max_slots and max_draws must not be negative");
  require_finite(Xs, (size_t)m * D, "sample_posterior: the query points must be finite");
  if (z_in) require_finite(z_in, (size_t)(z_per_emulator ? E : 1) * S * m, "sample_posterior: z must be finite");

  const SamplePlan plan = sample_plan(E, m, S, eng.LD, eng.NP, R, eng.free_bytes_or_twice_budget(),max_slots, max_draws);
  const long slots = plan.slots;
  const int Sc = (int)plan.draws;

  ScratchFactor sub(m, slots);
  DevBuf<double> dXq((size_t)m * D);
  SamplePass p(m, slots, Sc, R, stream, sub.stream());
  HIPCK(hipMemcpyAsync(dXq, Xs, (size_t)m * D * sizeof(double), hipMemcpyHostToDevice, stream));
  HIPCK(hipMemsetAsync(p.dZ, 0, (size_t)slots * p.zrows * p.MP * sizeof(double), sub.stream()));      // columns >= m and rows >= Sc: exact zeros
  for (long e0 = 0; e0 < E; e0 += slots) {
    const long cnt = std::min(slots, E - e0);
    const std::vector<int> grp(ids.begin() + e0, ids.begin() + e0 + cnt);
    sample_build(eng, grp, Xs, dXq, m, p, mean_out + (size_t)e0 * m);
    HIPCK(hipMemcpyAsync(p.dStreams, streams + e0, (size_t)cnt * sizeof(unsigned), hipMemcpyHostToDevice, sub.stream()));
    sample_factor(eng, sub, grp, include_nugget, jitter, p, jitter_used + e0, ok + e0);
    sample_draws(sub, e0, cnt, m, S, Sc, seed, z_in, z_per_emulator, p, samples, z_out);
  }
}

}  // namespace mogp
