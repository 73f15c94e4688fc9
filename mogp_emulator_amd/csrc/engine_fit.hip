// Engine: the multi-start MAP fit -- the L-BFGS slot pool, the replica engine and its cache; ScratchFactor
#include "engine_internal.h"

#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <memory>
#include <mutex>

namespace mogp {

// ---------------------------------------------------------------------------------------------
// Multi-start MAP fit (fitting.hpp:61-128, fitting.py:219-266).  Every optimiser "round" is ONE batched device evaluation
// (objective + gradient) of every run that needs one; every run is its own L-BFGS (memory 10) with an Armijo/curvature
// line search and advances independently of the others (slot pool, run_pool below).  Optimiser trajectory parity with
// dlib / scipy is unpinned; the end-point objective is what the tests compare.
// ---------------------------------------------------------------------------------------------
namespace {
struct Lbfgs {
  int np = 0;
  std::vector<double> x, g, d, xt, gt;   // current point/gradient, direction, trial point/gradient
  double f = 0., ft = 0., step = 1., slope = 0.;
  std::vector<std::vector<double>> S, Y;
  std::vector<double> rho;
  int iter = 0, ls_iter = 0;
  enum { NEED_F0, LINESEARCH, DONE, FAILED } state = NEED_F0;
  double step_lo = 0., step_hi = 0.;      // bracketing for the curvature condition

  void direction() {
    d = g;
    const int h = (int)S.size();
    std::vector<double> al(h);
    for (int i = h - 1; i >= 0; --i) {
      double a = 0.;
      for (int k = 0; k < np; ++k) a += S[i][k] * d[k];
      a *= rho[i];
      al[i] = a;
      for (int k = 0; k < np; ++k) d[k] -= a * Y[i][k];
    }
    if (h > 0) {
      double yy = 0., sy = 0.;
      for (int k = 0; k < np; ++k) { yy += Y[h - 1][k] * Y[h - 1][k]; sy += S[h - 1][k] * Y[h - 1][k]; }
      const double gam = sy / yy;
      for (int k = 0; k < np; ++k) d[k] *= gam;
    }
    for (int i = 0; i < h; ++i) {
      double b = 0.;
      for (int k = 0; k < np; ++k) b += Y[i][k] * d[k];
      b *= rho[i];
      for (int k = 0; k < np; ++k) d[k] += S[i][k] * (al[i] - b);
    }
    for (int k = 0; k < np; ++k) d[k] = -d[k];
    slope = 0.;
    for (int k = 0; k < np; ++k) slope += g[k] * d[k];
    if (!(slope < 0.)) {   // not a descent direction: restart from steepest descent
      S.clear(); Y.clear(); rho.clear();
      for (int k = 0; k < np; ++k) d[k] = -g[k];
      slope = 0.;
      for (int k = 0; k < np; ++k) slope -= g[k] * g[k];
    }
  }
  void trial() {
    for (int k = 0; k < np; ++k) xt[k] = x[k] + step * d[k];
  }
};
}  // namespace

// the replica engine kept between multi-start fits, one per device (never destroyed at exit: the HIP runtime may be gone by then);
// the slots of different devices are independent, so the parts of a multi-part model on different GPUs do not evict each other's
static std::unique_ptr<Engine>& replica_cache(int device) {
  static std::map<int, std::unique_ptr<Engine>>* p = new std::map<int, std::unique_ptr<Engine>>();
  return (*p)[device];
}
static std::mutex& replica_cache_mutex() {
  static std::mutex* m = new std::mutex();
  return *m;
}

// The optimiser runs of a multi-start fit as a SLOT POOL (round 6).  `slots` are emulators of THIS engine; a slot
// carries one L-BFGS run at a time.  Every round is ONE batched objective (+ gradient) evaluation of the slots whose run needs one; a run
// that ends (converged, out of iterations, failed) hands its slot to the next pending run IN THE SAME ROUND -- `next(pos, x0, tag)` fills
// the slot (and, on a replica engine, gives it the targets and priors of the run's emulator), `done(tag, f, x)` receives the end point
// (f = +inf and x empty for a failed run) -- so every evaluation is full until the queue drains.  The reference runs one optimiser per
// emulator with no coupling at all (mogp_gpu/src/fitting.hpp:122-127 OpenMP over emulators; fitting.py:333-335 Pool.starmap); rounds 1-5
// ran fixed passes of starts in lock-step, each ending on its slowest run (64 x 15 starts: 71 % of the raw fit+gradient rate).
// A run's trajectory depends on its own evaluations only, and those are bit-identical whatever the batch they are part of (one-launch
// Cholesky), so the end points do not depend on the schedule.
void Engine::run_pool(const std::vector<int>& slots, const std::function<bool(int, std::vector<double>&, int&)>& next,
                      const std::function<void(int, double, const std::vector<double>&)>& done) {
  const FitOptions& opt = fit_options();
  const int ns = (int)slots.size();
  std::vector<Lbfgs> st(ns);
  std::vector<int> tag(ns, -1), evals(ns, 0);
  std::vector<char> live(ns, 0);
  const int eval_cap = opt.max_iter * 25;
  auto start_run = [&](int pos) {
    std::vector<double> x0;
    int t = -1;
    if (!next(pos, x0, t)) {
      live[pos] = 0;
      return;
    }
    Lbfgs s;
    s.np = n_theta(slots[pos]);
    if ((int)x0.size() != s.np) throw std::runtime_error("fit_map: starting point of the wrong length");
    s.g.resize(s.np); s.d.resize(s.np); s.gt.resize(s.np);
    s.x = x0;
    s.xt = s.x;
    st[pos] = std::move(s);
    tag[pos] = t;
    evals[pos] = 0;
    live[pos] = 1;
    g_lb_runs += 1;
  };
  auto finish_run = [&](int pos) {
    const Lbfgs& s = st[pos];
    const bool good = !(s.state == Lbfgs::FAILED || s.state == Lbfgs::NEED_F0) && std::isfinite(s.f);
    done(tag[pos], good ? s.f : std::numeric_limits<double>::infinity(), good ? s.x : std::vector<double>());
    start_run(pos);
  };
  for (int pos = 0; pos < ns; ++pos) start_run(pos);
  const double c1 = 1e-4, c2 = 0.9;      // Armijo / weak curvature
  static const int lazy_env = [] { const char* e = getenv("MOGP_LAZY_GRAD"); return e ? atoi(e) : -1; }();
  const bool lazy_grad = lazy_env < 0 ? n >= 512 : lazy_env != 0;
  for (;;) {
    std::vector<int> act, actid;
    std::vector<const double*> th;
    for (int pos = 0; pos < ns; ++pos)
      if (live[pos]) {
        act.push_back(pos);
        actid.push_back(slots[pos]);
        th.push_back(st[pos].xt.data());
      }
    if (act.empty()) break;
    g_pool_rounds += 1;
    g_pool_slot_rounds += (long long)act.size();
    int maxnp = 0;
    for (int pos : act) maxnp = std::max(maxnp, st[pos].np);
    std::vector<double> fv(act.size()), gv(act.size() * (size_t)maxnp);
    std::vector<int> okv(act.size());
    if (lazy_grad) {
      // The objective of every active run first; the gradient (L^-1, K^-1, the fused reduction: 2/3 of an evaluation) only
      // where the optimiser will look at it -- a trial point that fails the sufficient-decrease test is shortened without.
      // 8 - 14 % of the trial points of the benchmark fits fail it: 64 emulators x 15 starts of n = 2000, 10 / 100
      // iterations: 2.58 -> 2.34 s / 8.11 -> 7.42 s, same optima.  The second synchronisation per round costs small
      // problems more than it saves (n = 200, 15 starts: 0.045 -> 0.051 s), so it is used from n = 512 (MOGP_LAZY_GRAD=0 / 1).
      // The objective-only evaluation does not solve alpha either: grad_current does, under the triangular inversion, for the points
      // that passed -- the others never needed it.
      eval(actid, th, false, fv.data(), nullptr, 0, okv.data());
      std::vector<int> gids, gpos;
      for (size_t q = 0; q < act.size(); ++q) {
        const Lbfgs& s = st[act[q]];
        if (!okv[q]) continue;
        if (s.state == Lbfgs::NEED_F0 || fv[q] <= s.f + c1 * s.step * s.slope) {
          gids.push_back(actid[q]);
          gpos.push_back((int)q);
        }
      }
      if (!gids.empty()) {
        g_grad_evals += (long long)gids.size();
        std::vector<double> tmp(gids.size() * (size_t)maxnp);
        grad_current(gids, tmp.data(), maxnp);
        for (size_t k = 0; k < gids.size(); ++k) std::memcpy(gv.data() + (size_t)gpos[k] * maxnp, tmp.data() + k * maxnp, sizeof(double) * maxnp);
      }
    } else {
      eval(actid, th, true, fv.data(), gv.data(), maxnp, okv.data());
    }
    for (size_t q = 0; q < act.size(); ++q) {
      const int pos = act[q];
      Lbfgs& s = st[pos];
      const bool ok = okv[q] != 0;
      const double* gq = gv.data() + q * maxnp;
      bool gfinite = ok;
      evals[pos] += 1;
      // (a trial point that fails the sufficient-decrease test is judged by its objective alone)
      const bool armijo_fail = s.state == Lbfgs::LINESEARCH && ok && !(fv[q] <= s.f + c1 * s.step * s.slope);
      if (ok && !armijo_fail) for (int k = 0; k < s.np; ++k) gfinite = gfinite && std::isfinite(gq[k]);
      if (s.state == Lbfgs::NEED_F0) {
        if (!gfinite) { s.state = Lbfgs::FAILED; finish_run(pos); continue; }
        s.f = fv[q];
        s.g.assign(gq, gq + s.np);
        s.direction();
        double gn = 0.;
        for (int k = 0; k < s.np; ++k) gn += s.g[k] * s.g[k];
        gn = std::sqrt(gn);
        if (gn <= opt.gtol) { s.state = Lbfgs::DONE; finish_run(pos); continue; }
        s.step = std::min(1.0, 1.0 / gn);
        s.step_lo = 0.; s.step_hi = 0.; s.ls_iter = 0;
        s.trial();
        s.state = Lbfgs::LINESEARCH;
        continue;
      }
      // line search step: Armijo (1e-4) + weak curvature (0.9) by bisection/expansion
      bool accept = false;
      if (!gfinite || !(fv[q] <= s.f + c1 * s.step * s.slope)) {
        s.step_hi = s.step;
        s.step = 0.5 * (s.step_lo + s.step_hi);
        g_ls_short += 1;
      } else {
        double st_slope = 0.;
        for (int k = 0; k < s.np; ++k) st_slope += gq[k] * s.d[k];
        if (st_slope < c2 * s.slope && s.ls_iter < 10) {
          s.step_lo = s.step;
          s.step = (s.step_hi > 0.) ? 0.5 * (s.step_lo + s.step_hi) : 2.0 * s.step;
          g_ls_long += 1;
        } else {
          accept = true;
        }
      }
      s.ls_iter++;
      if (!accept) {
        if (s.ls_iter > 40 || s.step < 1e-20 || evals[pos] >= eval_cap) {
          // could not make progress along d: take what we have
          s.state = Lbfgs::DONE;
          finish_run(pos);
          continue;
        }
        s.trial();
        continue;
      }
      // accept xt
      std::vector<double> sv(s.np), yv(s.np);
      double sy = 0., yy = 0.;
      for (int k = 0; k < s.np; ++k) {
        sv[k] = s.xt[k] - s.x[k];
        yv[k] = gq[k] - s.g[k];
        sy += sv[k] * yv[k];
        yy += yv[k] * yv[k];
      }
      const double fold = s.f;
      s.x = s.xt;
      s.f = fv[q];
      s.g.assign(gq, gq + s.np);
      if (sy > 1e-10 * yy && yy > 0.) {
        s.S.push_back(sv); s.Y.push_back(yv); s.rho.push_back(1.0 / sy);
        if (s.S.size() > 10) { s.S.erase(s.S.begin()); s.Y.erase(s.Y.begin()); s.rho.erase(s.rho.begin()); }
      }
      s.iter++;
      g_lb_iters += 1;
      double gmax = 0.;
      for (int k = 0; k < s.np; ++k) gmax = std::max(gmax, std::fabs(s.g[k]));
      if (std::fabs(fold - s.f) <= opt.ftol * std::max(1.0, std::fabs(s.f)) || gmax <= opt.gtol || s.iter >= opt.max_iter || evals[pos] >= eval_cap) {
        s.state = Lbfgs::DONE;
        finish_run(pos);
        continue;
      }
      s.direction();
      s.step = 1.0; s.step_lo = 0.; s.step_hi = 0.; s.ls_iter = 0;
      s.trial();
    }
  }
}

// Slot `slot` of this (replica) engine becomes a copy of emulator `i` of `src`: targets (host + device, with the fixed-mean
// subtraction of the constructor), nugget type / size, hyper-parameter and mean priors; no hyper-parameters, no factor.
void Engine::retarget(int slot, const Engine& src, int i) {
  std::copy(src.hT.begin() + (size_t)i * n, src.hT.begin() + (size_t)(i + 1) * n, hT.begin() + (size_t)slot * n);
  std::vector<double> res(hT.begin() + (size_t)slot * n, hT.begin() + (size_t)(slot + 1) * n);
  if (!analytic && mean.n_params() == 0 && mean.kind == 1)
    for (auto& x : res) x -= mean.value;
  HIPCK(hipMemcpyAsync(dT + (size_t)slot * n, res.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice, stream));
  // the fresh state below is not permuted, so the slot's inputs have to be in training order again: the next run's kernels read
  // dXp[slot] whatever its nugget type.  (The pool hands out runs between evaluations, after the synchronisation of `stream` that
  // every side stream has joined: nothing in flight still reads the slot.)
  if (dXp && gp[slot].permuted) {
    restore_order(slot);
    g_inputs_restored += 1;
  }
  HIPCK(hipStreamSynchronize(stream));          // `res` is a temporary
  const GPState& s = src.gp[i];
  GPState d;
  d.nug_type = s.nug_type;
  d.nug_size = s.nug_size;
  d.pri = s.pri;
  d.mp_b = s.mp_b; d.mp_Binv = s.mp_Binv; d.mp_Binvb = s.mp_Binvb; d.mp_logdetB = s.mp_logdetB;
  d.data.assign(s.data.size(), 0.);
  d.meanp.assign(n_mean(), 0.);
  d.beta.assign(q, 0.);
  w2.erase(slot);
  gp[slot] = std::move(d);
}

ScratchFactor::ScratchFactor(int rows_, long slots_) : ScratchFactor(rows_, slots_, std::vector<double>((size_t)slots_ * rows_, 0.0)) {}

// (the engine never reads its inputs: its covariance build is replaced by the caller's fill)
ScratchFactor::ScratchFactor(int rows_, long slots_, const std::vector<double>& zeros)
    : rows(rows_), slots((int)slots_), eng(zeros.data(), rows_, 1, zeros.data(), (int)slots_, 0, MeanFunc(), 0, NUG_FIXED, 0.0) {
  NP = eng.NP;
  MS = eng.MS;
  if (NP != scratch_np(rows)) throw std::runtime_error("ScratchFactor: unexpected layout of the engine");
}

void ScratchFactor::factor(const CovFill& fill, std::vector<int>& info, const std::vector<int>* only, bool want_linv) {
  std::vector<int> ids;
  if (only) {
    ids = *only;
  } else {
    ids.resize(slots);
    for (int i = 0; i < slots; ++i) ids[i] = i;
  }
  if (ids.empty()) return;
  for (int i : ids) {
    if (i < 0 || i >= slots) throw std::runtime_error("ScratchFactor: slot out of range");
    eng.gp[i].nugget_used = eng.gp[i].nug_size;
  }
  eng.factorize_blocked(ids, info, false, &fill);
  std::vector<int> ok;
  for (int i : ids) {
    GPState& g = eng.gp[i];
    g.unfit();
    g.factored = info[i] == 0;
    if (g.factored) ok.push_back(i);
  }
  if (want_linv && !ok.empty()) eng.ensure_linv(ok);
}

void ScratchFactor::logdet_and_solve(const std::vector<int>& okslots) {
  if (okslots.empty()) return;
  eng.upload_idx(okslots);
  const BatchView sv = eng.view((int)okslots.size());
  launch_logdet(sv, eng.dInfo, eng.dRes, eng.stream);
  launch_alpha_from_linv(sv, eng.stream);
}

// The inputs of a cached replica engine taken by a fit with other inputs of the same shape: everything the engine derived from X
// is rebuilt -- the host and device copies, the analytic mean's design matrix H(X), and every slot's copy in pivot order (put back
// into training order: the slots' states are replaced by retarget before a run, and a state that is not permuted reads that copy).
void Engine::reset_inputs(const std::vector<double>& X) {
  hX = X;
  HIPCK(hipMemcpy(dX, hX.data(), hX.size() * sizeof(double), hipMemcpyHostToDevice));
  if (R > 1) {
    std::vector<double> dummy(q, 0.);
    mean.mean_deriv(hX.data(), n, D, dummy.data(), q, hH.data());
    HIPCK(hipMemcpy(dH, hH.data(), hH.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  if (dXp) {
    for (int i = 0; i < B; ++i) {
      if (gp[i].permuted) g_inputs_restored += 1;
      restore_order(i);
    }
    HIPCK(hipStreamSynchronize(stream));
  }
}

// The replica engine of the LAST multi-start fit (or mixture prediction) of the process is kept (one engine per device) and taken again
// when the next caller has the same shape (n, D, slots, kernel, mean function, device): its 3 x slots matrices are tens of GB, and on SOME
// boxes fresh allocations of that size cost 0.9 - 1.5 s per fit (bench.py run behind the GPU test suite on the same box: fit_GP_MAP 3.1
// instead of 2.15 s, every call with 256 slots; on a fresh box 2.13 s from the first call; writing 200 GB from another process beforehand
// did not reproduce it -- profiles/r06_fitmap_context_and_grad_chain.txt).  A caller of another shape frees it.  MOGP_REPLICA_CACHE=0:
// every caller builds and frees its own.
ReplicaLease::ReplicaLease(const Engine& src, long slots, const std::vector<double>& targets, int nug_type, double nug_size) {
  static const bool on = [] { const char* e = getenv("MOGP_REPLICA_CACHE"); return !e || atoi(e) != 0; }();
  cache_on = on;
  {
    std::lock_guard<std::mutex> lk(replica_cache_mutex());
    int dev = -1;
    (void)hipGetDevice(&dev);
    std::unique_ptr<Engine>& slot = replica_cache(dev);
    if (slot && cache_on && slot->n == src.n && slot->D == src.D && slot->B == (int)slots && slot->kernel_type == src.kernel_type &&
        slot->analytic == src.analytic && slot->testing_size == src.testing_size && slot->device_id() == dev &&
        slot->mean.kind == src.mean.kind && slot->mean.value == src.mean.value && slot->mean.dims == src.mean.dims &&
        slot->mean.powers == src.mean.powers) {
      rep = std::move(slot);
      rep->reset_inputs(src.hX);
      g_rep_reused += 1;
    } else {
      slot.reset();                                   // (frees the old one BEFORE the new one is allocated)
    }
  }
  if (!rep)
    rep.reset(new Engine(src.hX.data(), src.n, src.D, targets.data(), (int)slots, src.testing_size, src.mean, src.kernel_type, nug_type, nug_size,
                         src.analytic));
}

// hand the engine back to the cache when the scope is left normally (an exception destroys it)
ReplicaLease::~ReplicaLease() {
  if (!cache_on || !rep || std::uncaught_exceptions() > 0) return;
  const int dev = rep->device_id();
  std::lock_guard<std::mutex> lk(replica_cache_mutex());
  replica_cache(dev) = std::move(rep);
}

// Multi-start MAP fit (fitting.hpp:61-128, fitting.py:219-266): n_tries L-BFGS runs per emulator, the best end point wins.
// All (emulator, start) runs go through ONE slot pool (run_pool).  The runs are independent, so as many of them as pay run
// CONCURRENTLY on a replica engine whose slots take the targets and priors of whatever run they are handed (retarget): small
// problems, whose batches do not fill the GPU, then cost about one start instead of n_tries, and large ones keep every batched
// evaluation full until the queue of runs drains.  MOGP_PARALLEL_STARTS=0: no replica engine -- the slots are this engine's own
// emulators, each working through its own starts one after the other (still without waiting for its neighbours).
Engine::Starts Engine::draw_starts(std::mt19937_64& rng, const std::vector<std::pair<const Engine*, int>>& emus, int n_tries,
                                   const double* theta0, int theta0_len) {
  const int ne = (int)emus.size();
  // starting points: start 0 = theta0 if given, everything else drawn from the priors (Priors.py:394-418)
  Starts x0(n_tries, std::vector<std::vector<double>>(ne));
  for (int s = 0; s < n_tries; ++s)
    for (int e = 0; e < ne; ++e) {
      const Engine& g = *emus[e].first;
      const int i = emus[e].second;
      std::vector<double>& x = x0[s][e];
      x.assign(g.n_theta(i), 0.);
      if (s == 0 && theta0_len > 0) x.assign(theta0, theta0 + theta0_len);
      else g.gp[i].pri.sample(rng, g.NC, g.gp[i].nug_type, x.data() + g.n_mean());
    }
  return x0;
}

void Engine::fit_map(const std::vector<int>& ids, int n_tries, const double* theta0, int theta0_len) {
  if (ids.empty()) return;
  if (n_tries < 1) throw std::runtime_error("number of attempts must be positive");
  for (int i : ids)
    if (theta0_len > 0 && theta0_len != n_theta(i)) throw std::runtime_error("length of theta0 must equal n_params of GP.");
  std::vector<std::pair<const Engine*, int>> emus;
  for (int i : ids) emus.emplace_back(this, i);
  fit_map_from(ids, draw_starts(rng, emus, n_tries, theta0, theta0_len));
}

void Engine::fit_map_from(const std::vector<int>& ids, const Starts& x0) {
  if (ids.empty()) return;
  const int n_tries = (int)x0.size();
  if (n_tries < 1) throw std::runtime_error("number of attempts must be positive");
  const int ne = (int)ids.size();
  for (const auto& row : x0)
    if ((int)row.size() != ne) throw std::runtime_error("fit_map: one starting point per emulator and start is needed");
  std::vector<double> best_f(ne, std::numeric_limits<double>::infinity());
  std::vector<int> best_s(ne, -1);
  std::vector<std::vector<double>> best_x(ne);
  // run tag = s * ne + e; of equal end points the one of the earlier start wins, whatever order the runs finish in
  auto done = [&](int tag, double f, const std::vector<double>& x) {
    const int e = tag % ne, s = tag / ne;
    if (!x.empty() && std::isfinite(f) && (f < best_f[e] || (f == best_f[e] && s < best_s[e]))) {
      best_f[e] = f;
      best_s[e] = s;
      best_x[e] = x;
    }
  };
  // how many replica slots: what fits beside this engine (A, L^-1, K^-1 per slot plus the small per-emulator buffers), what pays
  // (replicas beyond what fills the device buy nothing and their buffers are fresh allocations: 64 x 15 starts of n = 2000 as ONE batch
  // of 960 replicas took 3.7 - 5.8 s, capped at 256 2.44 s, 128: 2.52 s -- round 2), MOGP_START_REPLICAS overrides the cap
  static const bool parallel_starts = [] { const char* e = getenv("MOGP_PARALLEL_STARTS"); return !e || e[0] != '0'; }();
  const long total = (long)ne * n_tries;
  long slots_n = ne;
  if (parallel_starts && n_tries > 1) {
    long fit = total;
    double free_b = 0.;
    if (free_device_bytes(free_b)) fit = slots_in_half_of(free_b, replica_slot_bytes(MS, LD));
    static const long replica_cap = [] { const char* e = getenv("MOGP_START_REPLICAS"); return e ? atol(e) : 0L; }();
    const long cap = replica_cap > 0 ? replica_cap : std::max<long>(ne, replica_slot_bound(NP, TILE));
    slots_n = std::min(total, std::min(fit, cap));
    if (slots_n > 8) slots_n -= slots_n % 8;      // (batches that are multiples of 8 give every XCD whole emulators)
  }
  if (slots_n <= ne || !parallel_starts || n_tries == 1) {
    // no replicas: slot e IS emulator ids[e] and works through its own starts
    std::vector<int> nexts(ne, 0);
    run_pool(ids,
             [&](int pos, std::vector<double>& x, int& tag) {
               if (nexts[pos] >= n_tries) return false;
               const int s = nexts[pos]++;
               x = x0[s][pos];
               tag = s * ne + pos;
               return true;
             },
             done);
  } else {
    // ONE replica engine of slots_n slots; the queue of runs in start-major order (all emulators' start 0 first)
    std::vector<double> targets((size_t)slots_n * n);
    for (long k = 0; k < slots_n; ++k) {
      const int e = (int)(k % ne);
      std::copy(hT.begin() + (size_t)ids[e] * n, hT.begin() + (size_t)(ids[e] + 1) * n, targets.begin() + (size_t)k * n);
    }
    const auto tc0 = std::chrono::steady_clock::now();
    // (the cached replica engine of the device where its shape matches, else a new one: ReplicaLease, above)
    ReplicaLease rep(*this, slots_n, targets, gp[ids[0]].nug_type, gp[ids[0]].nug_size);
    g_rep_build_us += std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - tc0).count();
    std::vector<int> holds(slots_n, -1);          // which emulator (index into ids) a slot's targets and priors belong to
    std::vector<int> rslots(slots_n);
    for (long k = 0; k < slots_n; ++k) rslots[k] = (int)k;
    long next_run = 0;
    Engine* self = this;
    const auto tp0 = std::chrono::steady_clock::now();
    struct PoolTimer {
      std::chrono::steady_clock::time_point t0;
      ~PoolTimer() { g_rep_pool_us += std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count(); }
    } pool_timer{tp0};
    rep->run_pool(rslots,
                  [&](int pos, std::vector<double>& x, int& tag) {
                    if (next_run >= total) return false;
                    const long r = next_run++;
                    const int s = (int)(r / ne), e = (int)(r % ne);
                    if (holds[pos] != e) {
                      const auto tr0 = std::chrono::steady_clock::now();
                      rep->retarget(pos, *self, ids[e]);
                      g_retarget_us += std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - tr0).count();
                      g_retargets += 1;
                      holds[pos] = e;
                    }
                    x = x0[s][e];
                    tag = (int)r;
                    return true;
                  },
                  done);
  }
  // refit at the best point of every emulator (fitting.hpp:115-117); failures -> "not fit" (:111-113)
  std::vector<int> fin;
  std::vector<const double*> th;
  for (int e = 0; e < ne; ++e) {
    if (best_x[e].empty()) {
      gp[ids[e]].set_fit(false);
    } else {
      fin.push_back(ids[e]);
      th.push_back(best_x[e].data());
    }
  }
  if (!fin.empty()) {
    std::vector<double> fv(fin.size());
    std::vector<int> okv(fin.size());
    eval(fin, th, false, fv.data(), nullptr, 0, okv.data());
  }
}

}  // namespace mogp
