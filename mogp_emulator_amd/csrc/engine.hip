#include "engine_internal.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <mutex>

namespace mogp {

void hip_check(hipError_t e, const char* what) {
  if (e != hipSuccess) throw std::runtime_error(std::string("HIP error in ") + what + ": " + hipGetErrorString(e));
}

FitOptions& fit_options() {
  static FitOptions o;
  return o;
}
ScheduleOverride& schedule_override() {
  static ScheduleOverride o;
  return o;
}

// ---------------------------------------------------------------------------------------------
// profiling registry (bench.py): HIP events on the launch stream around tagged kernels
// ---------------------------------------------------------------------------------------------
namespace {
struct ProfRec {
  std::vector<std::pair<Event, Event>> ev;
  double flops = 0., bytes = 0., ms_done = 0.;
  long long launches = 0;
  Event pending;
};
bool g_prof_on = false;
// (never destroyed: events that are still registered at exit must not be handed back to a runtime that is shutting down)
std::map<std::string, ProfRec>& g_prof = *new std::map<std::string, ProfRec>();
std::mutex g_prof_mu;
}  // namespace

void prof_begin(const char* tag, hipStream_t s) {
  if (!g_prof_on) return;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  ProfRec& r = g_prof[tag];
  Event e = try_make_timing_event();
  if (!e) return;
  hipEventRecord(e, s);
  r.pending = std::move(e);
}
void prof_end(const char* tag, hipStream_t s, double flops, double bytes) {
  if (!g_prof_on) return;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  ProfRec& r = g_prof[tag];
  if (!r.pending) return;
  Event e = try_make_timing_event();
  if (!e) return;
  hipEventRecord(e, s);
  r.ev.emplace_back(std::move(r.pending), std::move(e));
  r.flops += flops;
  r.bytes += bytes;
  r.launches += 1;
}
void prof_enable(bool on) { g_prof_on = on; }
long long prof_counter(const char* name) {
  const std::string s(name ? name : "");
  if (s == "backsolve_timeouts") return g_bs_timeouts.load();
  if (s == "alpha_solves") return g_alpha_solves.load();      // emulators whose alpha was solved (with the evaluation or when first read)
  if (s == "mchol_aborts") return g_mc_aborts.load();          // one-launch factorisations repeated with a multi-launch schedule
  if (s == "objective_evals") return g_obj_evals.load();      // emulator objective evaluations (with or without gradient)
  if (s == "gradient_evals") return g_grad_evals.load();      // of which with gradient
  // optimiser statistics of fit_GP_MAP: runs started, accepted L-BFGS steps, line-search trial points that were shortened
  // (sufficient decrease failed) / lengthened (curvature condition failed)
  if (s == "lbfgs_runs") return g_lb_runs.load();
  if (s == "lbfgs_iterations") return g_lb_iters.load();
  if (s == "linesearch_shortened") return g_ls_short.load();
  if (s == "linesearch_lengthened") return g_ls_long.load();
  // slot pool of fit_GP_MAP: batched optimiser rounds, and the sum over rounds of the slots that took part (/ rounds = mean batch)
  if (s == "pool_rounds") return g_pool_rounds.load();
  if (s == "pool_slot_rounds") return g_pool_slot_rounds.load();
  if (s == "replica_engine_build_us") return g_rep_build_us.load();      // host time spent constructing replica engines (allocations)
  if (s == "retarget_us") return g_retarget_us.load();                   // host time inside Engine::retarget (slot takes another emulator's targets)
  if (s == "retargets") return g_retargets.load();
  if (s == "replica_engines_reused") return g_rep_reused.load();          // multi-start fits that took the cached replica engine
  // replica slots whose inputs went from pivot order back to training order when they took another run's emulator or another fit
  if (s == "replica_inputs_restored") return g_inputs_restored.load();
  if (s == "device_bytes_live") return g_device_bytes_live.load();       // device bytes held by DevBuf objects right now (devmem.h)
  if (s == "replica_pool_us") return g_rep_pool_us.load();               // ... from there to the end of fit_map's replica block (pool + its destruction excluded)
  return -1;
}
bool prof_is_on() { return g_prof_on; }
void prof_reset() {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  g_prof.clear();
}
bool prof_get(const char* tag, double* ms, long long* launches, double* flops, double* bytes) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  auto it = g_prof.find(tag);
  if (it == g_prof.end()) return false;
  ProfRec& r = it->second;
  for (auto& p : r.ev) {
    hipEventSynchronize(p.second);
    float t = 0.f;
    hipEventElapsedTime(&t, p.first, p.second);
    r.ms_done += t;
  }
  r.ev.clear();
  *ms = r.ms_done;
  *launches = r.launches;
  *flops = r.flops;
  *bytes = r.bytes;
  return true;
}

// ---------------------------------------------------------------------------------------------

Engine::Engine(const double* X, int n_, int D_, const double* targets, int B_, unsigned testing_size_, const MeanFunc& mean_,
               int kernel_type_, int nug_type, double nug_size, bool analytic_mean)
    : n(n_), D(D_), B(B_), kernel_type(kernel_type_), testing_size(testing_size_), mean(mean_) {
  analytic = analytic_mean && mean.n_params() > 0;
  q = analytic ? mean.n_params() : 0;
  R = 1 + q;
  if (R > RMAX) throw std::runtime_error("analytic mean: at most " + std::to_string(RMAX - 1) + " mean-function terms are supported");
  if (analytic && q >= n_) throw std::runtime_error("analytic mean: more mean-function terms than training points");
  if (n < 1 || D < 1 || B < 1) throw std::runtime_error("inputs must have shape (n, D) with n, D >= 1");
  if (kernel_type < 0 || kernel_type > 4) throw std::runtime_error("Unrecognized kernel type\n");
  if (D < 1) throw std::runtime_error("inputs must have at least one column");
  if (D > MAX_D)
    throw std::runtime_error("at most " + std::to_string(MAX_D) + " input dimensions are supported by the device kernels (" +
                             std::to_string(D) + " given): the per-tile copy of the inputs must fit the 160 KB LDS");
  if (nug_type < 0 || nug_type > 3) throw std::runtime_error("Unrecognized nugget_type");
  for (int d : mean.dims)
    if (d >= D) throw std::runtime_error("Dimension index must be less than " + std::to_string(D));
  NP = roundup(n + R, TILE);
  // Row stride = NP.  A non-power-of-two stride (NP + 16) was tried against L2 set aliasing of the 16 KiB-strided tile rows
  // and measured SLOWER on MI355X (fit 7.5 -> 8.2 ms, fit+grad 15.3 -> 16.2 ms; predictive variance unchanged).
  LD = NP;
  MS = (size_t)NP * LD;
  NC = uniform() ? 1 : D;
  PS = D + 2;
  hX.assign(X, X + (size_t)n * D);
  hT.assign(targets, targets + (size_t)B * n);
  gp.resize(B);
  for (auto& g : gp) {
    g.nug_type = nug_type;
    g.nug_size = nug_size;
    g.data.assign(NC + 1 + (nug_type == NUG_FIT ? 1 : 0), 0.);
    g.meanp.assign(n_mean(), 0.);
    g.beta.assign(q, 0.);
  }
  {
    // stream memory operations (look-ahead schedule) are a property of the device THIS engine lives on
    int dev = 0, ok = 0;
    int cus = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0) n_cu = cus;
    can_waitval = hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&ok, hipDeviceAttributeCanUseStreamWaitValue, dev) == hipSuccess && ok != 0;
    device = dev;
  }
  // (no try / catch: when one of these throws, the members built so far are destroyed by the language)
  stream = make_stream(hipStreamNonBlocking);
  evReady = make_event(hipEventDisableTiming);
  for (auto& e : evGroup) e = make_event(hipEventDisableTiming);
  {
    int lo = 0, hi = 0;   // numerically lower = higher priority
    HIPCK(hipDeviceGetStreamPriorityRange(&lo, &hi));
    pstream = make_stream(hipStreamNonBlocking, hi);
  }
  dX.reserve((size_t)n * D);
  dP.reserve((size_t)B * PS);
  dT.reserve((size_t)B * n);
  dA.reserve((size_t)B * MS);
  RA = (R > 1) ? R + 1 : 1;
  dAlpha.reserve((size_t)B * RA * LD);
  if (R > 1) {
    dZ.reserve((size_t)B * R * LD);
    dM.reserve((size_t)B * (RMAX + 1) * RMAX);
    // design matrix columns: row c of mean_deriv = d mean / d beta_c = basis function c evaluated at X
    hH.assign((size_t)q * n, 0.);
    std::vector<double> dummy(q, 0.);
    mean.mean_deriv(X, n, D, dummy.data(), q, hH.data());
    dH.reserve(hH.size());
    HIPCK(hipMemcpy(dH, hH.data(), hH.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  dRes.reserve((size_t)B * RES_STRIDE);
  hRes = PinnedBuf<double>((size_t)B * RES_STRIDE);
  dInfo.reserve(B);
  dIdx.reserve(B);
  dLpack.reserve((size_t)B * lpack128_doubles_per_emulator());
  // (pinned: the parameter block goes up in front of every evaluation, and an asynchronous copy from pageable memory is staged by the runtime)
  hP = PinnedBuf<double>((size_t)B * PS);
  std::fill(hP.get(), hP.get() + (size_t)B * PS, 0.);
  HIPCK(hipMemcpy(dX, hX.data(), hX.size() * sizeof(double), hipMemcpyHostToDevice));
  // residual targets for parameter-free means are fixed once
  std::vector<double> res(hT);
  if (!analytic && mean.n_params() == 0 && mean.kind == 1)
    for (auto& x : res) x -= mean.value;
  HIPCK(hipMemcpy(dT, res.data(), res.size() * sizeof(double), hipMemcpyHostToDevice));
  rng.seed(fit_options().seed ? fit_options().seed : std::random_device{}());
}

// every buffer, stream and event is a member that releases itself; the signal word is the one exception (engine.h)
Engine::~Engine() {
  if (sigU1) hipFree(sigU1);
}

double Engine::nugget_size(int i) const {
  const GPState& g = gp[i];
  if (g.nug_type == NUG_FIT) return std::exp(g.data[NC + 1]);   // zero-initialised data -> 1 before the first fit   // gpparams.hpp:176-182
  return g.nug_size;
}

bool Engine::free_device_bytes(double& free_bytes) const {
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return false;
  free_bytes = (double)free_b;
  return true;
}

double Engine::free_bytes_or_twice_budget() const {
  double free_b = 0.;
  return free_device_bytes(free_b) ? free_b : 2.0 * ks_budget_bytes();
}

// K build of the slots in dIdx.  With one right-hand side it also presets the solution rows to the all-ones pattern the one-launch
// back substitution polls for (backsolve_chain_kernel<SENT>); `z_armed` records that, so that a chain launched on a row that has
// not been preset since its last solve arms it itself instead of reading stale values as "already there".
// A row stays armed for as long as its solve is deferred (ensure_alpha), over any number of calls: nothing but a back substitution of
// that emulator writes the row, and a reader that forgot to ask finds the pattern -- NaN -- and not the alpha of an older factor.
void Engine::build_cov(const BatchView& v, const ZeroRanges& zero, const CovFill* fill) {
  if (fill) {
    for (int r = 0; r < 2; ++r)
      if (zero.p[r] && zero.n[r]) HIPCK(hipMemsetAsync(zero.p[r], 0, zero.n[r] * sizeof(unsigned), stream));
    (*fill)(v);
    if (z_armed.size() != (size_t)B) z_armed.assign(B, 0);
    for (int i : idx_on_device) z_armed[i] = 0;
    return;
  }
  launch_cov_build(v, stream, zero);
  if (z_armed.size() != (size_t)B) z_armed.assign(B, 0);
  for (int i : idx_on_device) z_armed[i] = (R == 1 && v.Z != nullptr) ? 1 : 0;
}

BatchView Engine::view(int nb) const {
  BatchView v;
  v.n = n; v.D = D; v.NP = NP; v.LD = LD; v.MS = MS; v.PS = PS; v.kernel_type = device_kernel();
  v.X = dXp ? dXp : dX; v.XS = dXp ? (size_t)n * D : 0; v.P = dP; v.T = dT; v.A = dA; v.Linv = dLinv; v.Kinv = dKinv; v.alpha = dAlpha;
  v.idx = dIdx; v.nb = nb;
  v.R = R; v.RA = RA; v.H = dH; v.Z = (R > 1) ? dZ : dAlpha;
  return v;
}

void Engine::upload_idx(const std::vector<int>& ids) {
  if (ids == idx_on_device) return;      // the optimiser and the benchmark evaluate the same list again and again
  HIPCK(hipMemcpyAsync(dIdx, ids.data(), ids.size() * sizeof(int), hipMemcpyHostToDevice, stream));
  HIPCK(hipStreamSynchronize(stream));   // ids may be a temporary
  idx_on_device = ids;
}

void Engine::set_mean_priors(int i, int q_in, const double* b, const double* Binv, const double* Binvb, double logdetB) {
  GPState& g = gp[i];
  if (q_in == 0) {
    g.mp_b.clear(); g.mp_Binv.clear(); g.mp_Binvb.clear(); g.mp_logdetB = 0.;
  } else {
    if (!analytic) throw std::runtime_error("mean priors need the analytic mean function (analytic_mean=True)");
    if (q_in != q) throw std::runtime_error("mean priors must have one entry per mean-function term (" + std::to_string(q) + ")");
    g.mp_b.assign(b, b + q);
    g.mp_Binv.assign(Binv, Binv + (size_t)q * q);
    g.mp_Binvb.assign(Binvb, Binvb + q);
    g.mp_logdetB = logdetB;
  }
  g.unfit();
}

void Engine::set_theta(int i, const double* theta) {
  GPState& g = gp[i];
  const int nm = n_mean(), nd = n_data(i);
  g.meanp.assign(theta, theta + nm);
  g.data.assign(theta + nm, theta + nm + nd);
  g.unfit();
  if (g.nug_type == NUG_ADAPTIVE) g.nug_size = 0.;   // gpparams.hpp:118-126
  if (nm > 0) {
    std::vector<double> m(n), r(n);
    mean.mean_f(hX.data(), n, D, g.meanp.data(), nm, m.data());
    for (int k = 0; k < n; ++k) r[k] = hT[(size_t)i * n + k] - m[k];
    HIPCK(hipMemcpyAsync(dT + (size_t)i * n, r.data(), n * sizeof(double), hipMemcpyHostToDevice, stream));
    HIPCK(hipStreamSynchronize(stream));
  }
}

void Engine::upload_params(const std::vector<int>& ids) {
  for (int i : ids) {
    const GPState& g = gp[i];
    double* p = hP + (size_t)i * PS;
    for (int d = 0; d < D; ++d) p[d] = std::exp(g.data[uniform() ? 0 : d]);
    p[D] = std::exp(g.data[NC]);
    p[D + 1] = g.nugget_used;
  }
  HIPCK(hipMemcpyAsync(dP, hP, (size_t)B * PS * sizeof(double), hipMemcpyHostToDevice, stream));
}

// the one-launch back substitution on stream `st` (status words and sentinel rows prepared on the same stream, in front of it)
bool Engine::launch_backsolve_chain_on(hipStream_t st, const BatchView& v, const std::vector<int>& todo, bool with_res) {
  if (!dBsStatus) {
    dBsStatus.reserve(B);
    HIPCK(hipMemsetAsync(dBsStatus, 0, B * sizeof(int), st));
  }
  if (bs_epoch > 0x7FFFFF00) {                       // the status words are compared with the epoch: start over before it wraps
    HIPCK(hipMemsetAsync(dBsStatus, 0, B * sizeof(int), st));
    bs_epoch = 0;
  }
  if (z_armed.size() != (size_t)B) z_armed.assign(B, 0);
  for (int i : todo) {
    if (!z_armed[i]) HIPCK(hipMemsetAsync(dAlpha + (size_t)i * RA * LD, 0xFF, (size_t)LD * sizeof(double), st));
    z_armed[i] = 0;                                  // consumed by this solve
  }
  if (!with_res) return launch_backsolve_chain(v, ++bs_epoch, dBsStatus, n_cu, st);
  return launch_backsolve_chain(v, ++bs_epoch, dBsStatus, n_cu, st, dInfo, dRes, mc_used ? dMcCtrl : nullptr);
}

// Objective-only evaluations with one right-hand side leave alpha to whoever reads it first.  The analytic mean combines the solution
// rows right behind the solve (launch_combine_rows, with a matrix only eval has), and the pivoted path keeps its order of work.
bool Engine::alpha_is_deferred(const std::vector<int>& list, bool want_grad) const {
  if (want_grad || R > 1) return false;
  for (int i : list)
    if (gp[i].nug_type == NUG_PIVOT || gp[i].permuted) return false;
  return true;
}

void Engine::resolve_alpha_after_timeout(const std::vector<int>& timed_out) {
  if (timed_out.empty()) return;
  g_bs_timeouts += (long long)timed_out.size();
  upload_idx(timed_out);
  launch_backsolve(view((int)timed_out.size()), stream);
}

void Engine::ensure_alpha(const std::vector<int>& ids) {
  std::vector<int> need;
  for (int i : ids) {
    if (!gp[i].factored) throw std::runtime_error("emulator has not been fit");
    if (!gp[i].alpha) need.push_back(i);
  }
  if (need.empty()) return;
  if (R > 1) throw std::logic_error("ensure_alpha: with the analytic mean alpha is solved by the evaluation itself");
  upload_idx(need);
  launch_backsolve_chain_on(stream, view((int)need.size()), need, false);
  // (off the hot path: the evaluations of a fit with gradients solve alpha themselves, grad_current reads these words with its own results)
  std::vector<int> status(B, 0);
  HIPCK(hipMemcpyAsync(status.data(), dBsStatus, B * sizeof(int), hipMemcpyDeviceToHost, stream));
  HIPCK(hipStreamSynchronize(stream));
  HIPCK(hipGetLastError());
  std::vector<int> again;
  for (int i : need)
    if (status[i] == bs_epoch) again.push_back(i);
  resolve_alpha_after_timeout(again);
  for (int i : need) gp[i].have_alpha();
  g_alpha_solves += (long long)need.size();
}

// One synchronisation per evaluation: the factorisation leaves its status words on the device, log-det / Gram (and, unless
// alpha_is_deferred, alpha -- with L^-1 on the gradient path) are launched right behind it, and everything is read back together.
// An emulator whose factorisation failed has produced garbage there -- it is either retried (adaptive jitter) or reported.
// Deferred alpha: the factorisation carried the targets along as row n of the factor, so y = L^-1 t is there and launch_logdet forms
// log det K and |y|^2 with the device function the chain's leftmost chunk runs -- the same bits; the back substitution
// alpha = L^-T y (213 us per launch of a 3.95 ms fit at 64 x n=2000, profiles/lazy_alpha_ab.txt) is work the objective does not need.
void Engine::solve_and_collect(const std::vector<int>& list, std::vector<int>* info_out, bool want_grad, std::vector<double>& logdet,
                               std::vector<double>& gram) {
  for (int i : list) gp[i].factored = true;                // provisional (ensure_linv checks it)
  if (info_out) info_out->assign(B, 0);
  // second pass (rare): emulators whose one-launch back substitution gave up waiting are solved again with the
  // multi-launch path, which has no inter-workgroup waits
  const bool deferred = alpha_is_deferred(list, want_grad);
  long long solved = 0;                                    // emulators with a good factor whose alpha this call solved (alpha_solves)
  std::vector<int> todo(list);
  for (int pass = 0; pass < 2 && !todo.empty(); ++pass) {
    upload_idx(todo);
    BatchView v = view((int)todo.size());
    bool res_done = false;
    // single right-hand side: the one-launch chain; the per-block launches (launch_backsolve) serve R > 1 and the repeat of a timed-out chain
    const bool use_chain = R == 1 && pass == 0 && !deferred;
    if (deferred) {
      // (nothing to solve: the sentinel rows the K build laid stay armed for ensure_alpha)
    } else if (want_grad) {
      if (use_chain) {
        // Round 6: alpha by the SAME one-launch back substitution as a plain fit -- on the panel stream, UNDER the triangular inversion
        // (both only read the factor): the gemv with L^-1 that used to follow the inversion (0.25 ms for 64 x n=2000, HBM-bound) and the
        // logdet launch leave the path, and eval(grad=True) returns bit for bit the alpha, log-determinant and log-posterior of eval(grad=False).
        // fit + gradient, gemv behind the inversion / chain under it: 64 x n=2000 10.87 -> 10.81 ms, 8 x 1.751 -> 1.711, one matrix 0.918 -> 0.889.
        HIPCK(hipEventRecord(evReady, stream));            // the factor and the index list are in place
        HIPCK(hipStreamWaitEvent(pstream, evReady, 0));
        res_done = launch_backsolve_chain_on(pstream, v, todo);
        HIPCK(hipEventRecord(evGroup[14], pstream));
        ensure_linv(todo);                                 // (fresh factors: every listed emulator needs it, so the index list on the device stays as it is)
        HIPCK(hipStreamWaitEvent(stream, evGroup[14], 0));
      } else {
        // L^-1 is needed anyway, so K^-1 [t, H] = L^-T Y is one fully parallel gemv with it
        ensure_linv(todo);
        upload_idx(todo);
        v = view((int)todo.size());
        launch_alpha_from_linv(v, stream);
      }
    } else if (use_chain) {
      res_done = launch_backsolve_chain_on(stream, v, todo);
    } else {
      launch_backsolve(v, stream);
    }
    // (after the solves: it also collects the status words; use_chain = the chain ran and left its time-out words)
    if (!res_done) launch_logdet(v, dInfo, dRes, stream, use_chain ? dBsStatus : nullptr, bs_epoch, mc_used ? dMcCtrl : nullptr);
    // status words, log-determinants and Gram matrices come back in ONE copy into pinned host memory
    HIPCK(hipMemcpyAsync(hRes, dRes, (size_t)B * RES_STRIDE * sizeof(double), hipMemcpyDeviceToHost, stream));
    HIPCK(hipStreamSynchronize(stream));
    HIPCK(hipGetLastError());
    std::vector<int> again;
    for (int i : todo) {
      const double* r = hRes + (size_t)i * RES_STRIDE;
      if ((int)r[1] == BACKSOLVE_TIMEOUT) {
        again.push_back(i);
        continue;
      }
      logdet[i] = r[0];
      if (!deferred && (int)r[1] == 0) solved += 1;        // (a failed factorisation has no alpha: what was "solved" from it is garbage)
      if (info_out) (*info_out)[i] = (int)r[1];
      std::memcpy(gram.data() + (size_t)i * RMAX * RMAX, r + 2, sizeof(double) * RMAX * RMAX);
    }
    g_bs_timeouts += (long long)again.size();
    todo.swap(again);
  }
  if (!deferred) {
    for (int i : list) gp[i].have_alpha();                 // (eval drops the factor, and this with it, where the factorisation failed)
    g_alpha_solves += solved;
  }
}

// adaptive jitter ladder: linalg/cholesky.py:268-279 -- jitter = mean(diag K) * 1e-6, x10 per try, 5 tries.
// diag K = sigma^2 k(0) = sigma^2 exactly, so mean(diag K) = sigma^2.
void Engine::jitter_ladder(const std::vector<int>& failed, std::vector<int>& info, std::vector<char>& good, bool want_grad,
                           std::vector<double>& logdet, std::vector<double>& gram) {
  std::vector<double> jitter(B, 0.);
  std::vector<int> retry, recovered;
  for (int i : failed)
    if (gp[i].nug_type == NUG_ADAPTIVE) {
      jitter[i] = std::exp(gp[i].data[NC]) * 1e-6;
      retry.push_back(i);
    }
  for (int attempt = 0; attempt < 5 && !retry.empty(); ++attempt) {
    std::vector<int> todo;
    for (int i : retry)
      if (std::isfinite(jitter[i])) {
        gp[i].nugget_used = jitter[i];
        todo.push_back(i);
      }
    if (todo.empty()) break;
    factorize(todo, info);
    std::vector<int> still;
    for (int i : todo) {
      if (info[i] == 0) {
        good[i] = 1;
        gp[i].nug_size = jitter[i];
        recovered.push_back(i);
      } else {
        jitter[i] *= 10;
        still.push_back(i);
      }
    }
    retry.swap(still);
  }
  if (!recovered.empty()) solve_and_collect(recovered, nullptr, want_grad, logdet, gram);
}

void Engine::scatter_gradient(const std::vector<int>& ids, const std::vector<char>& good, double* grad, int grad_ld) {
  std::vector<int> gids;
  std::vector<int> pos;
  for (size_t k = 0; k < ids.size(); ++k)
    if (good[ids[k]]) {
      gids.push_back(ids[k]);
      pos.push_back((int)k);
    }
  if (gids.empty()) return;
  std::vector<double> tmp((size_t)gids.size() * grad_ld);
  grad_current(gids, tmp.data(), grad_ld);
  for (size_t q = 0; q < gids.size(); ++q)
    std::memcpy(grad + (size_t)pos[q] * grad_ld, tmp.data() + q * grad_ld, sizeof(double) * n_theta(gids[q]));
}

// set theta -> factorise -> solve and collect -> repeat after an abort -> jitter ladder -> log-posterior per emulator -> combine rows -> gradient
void Engine::eval(const std::vector<int>& ids, const std::vector<const double*>& thetas, bool want_grad, double* f, double* grad,
                  int grad_ld, int* ok) {
  const int nb = (int)ids.size();
  if (nb == 0) return;
  g_obj_evals += nb;
  if (want_grad) g_grad_evals += nb;
  for (int k = 0; k < nb; ++k) {
    set_theta(ids[k], thetas[k]);
    GPState& g = gp[ids[k]];
    g.nugget_used = (g.nug_type == NUG_FIXED) ? g.nug_size : (g.nug_type == NUG_FIT ? std::exp(g.data[NC + 1]) : 0.0);
  }
  std::vector<double> logdet(B, 0.), gram((size_t)B * RMAX * RMAX, 0.);
  std::vector<int> info;
  bool has_pivot = false;
  for (int i : ids) has_pivot = has_pivot || gp[i].nug_type == NUG_PIVOT;
  factorize(ids, info, !has_pivot);                          // (the pivoted path reads its status after every panel anyway)
  solve_and_collect(ids, has_pivot ? nullptr : &info, want_grad, logdet, gram);
  if (!has_pivot) {
    // the one-launch Cholesky gave up on a wait (never observed; the bound exists so that nothing can hang): its abort word
    // came back as the status of every emulator -- factorise again with the multi-launch schedule
    bool aborted = false;
    for (int i : ids) aborted = aborted || info[i] == MCHOL_ABORTED;
    if (aborted) {
      for (int i : ids) gp[i].drop_factor();                 // (L^-1 of the unusable factor may have been formed)
      refactor_after_abort(ids, info, true);
      solve_and_collect(ids, &info, want_grad, logdet, gram);
    }
  }
  std::vector<char> good(B, 0);
  std::vector<int> failed;
  for (int i : ids) {
    if (info[i] == 0) good[i] = 1;
    else {
      failed.push_back(i);
      gp[i].drop_factor();
    }
  }
  jitter_ladder(failed, info, good, want_grad, logdet, gram);
  std::vector<int> okids;
  for (int i : ids) {
    if (good[i]) {
      okids.push_back(i);
      gp[i].factored = true;
    } else {
      gp[i].drop_factor();
    }
  }
  std::vector<double> hM;
  if (R > 1) hM.assign((size_t)B * (RMAX + 1) * RMAX, 0.);
  AnalyticMean am;
  for (int k = 0; k < nb; ++k) {
    const int i = ids[k];
    GPState& g = gp[i];
    double val = std::numeric_limits<double>::quiet_NaN();
    bool fine = good[i];
    if (fine) {
      const double* G = gram.data() + (size_t)i * RMAX * RMAX;
      double quad = G[0], logdetA = 0.;
      int n_coeff = n;
      if (R > 1) {
        analytic_mean(G, RMAX, q, n, g.mp_b, g.mp_Binv, g.mp_Binvb, g.mp_logdetB, am);
        fine = am.ok;
        g.LA = am.LA;
        if (fine) {
          quad = am.quad; logdetA = am.logdetA; n_coeff = am.n_coeff;
          g.beta = am.beta;
          std::copy(am.M.begin(), am.M.end(), hM.begin() + (size_t)i * (RMAX + 1) * RMAX);
        }
      }
      if (fine) {
        // GaussianProcess.py:679-685; densegp_gpu.hpp:604-611
        val = 0.5 * (quad + logdet[i] + logdetA + n_coeff * std::log(2.0 * M_PI)) - g.pri.logp(g.data, NC, g.nug_type);
        if (!std::isfinite(val)) fine = false;
      }
    }
    // nugget="pivot": the reference never fails a fit whose pivoted factorisation exists; with many skipped rows the
    // log-posterior over the tiny replacement diagonal is inf / nan there as well, and the emulator is left "fit" with
    // that value (garbage in, garbage out) instead of raising.  ok[] still reports it, so the optimiser steps away.
    g.set_fit(fine || (good[i] && g.nug_type == NUG_PIVOT));
    g.logpost = val;
    g.logpost_stale = false;
    if (f) f[k] = val;
    if (ok) ok[k] = fine ? 1 : 0;
    if (!fine) good[i] = 0;
  }
  if (R > 1 && !okids.empty()) {
    HIPCK(hipMemcpyAsync(dM, hM.data(), hM.size() * sizeof(double), hipMemcpyHostToDevice, stream));
    upload_idx(okids);
    launch_combine_rows(view((int)okids.size()), dM, stream);
    HIPCK(hipStreamSynchronize(stream));
  }
  if (want_grad && grad) scatter_gradient(ids, good, grad, grad_ld);
}

void Engine::fit_one(int i, const double* theta, int len) {
  if (len != n_theta(i)) throw std::runtime_error("Shape of new GPParams object does not match existing one");
  double f;
  int ok;
  std::vector<int> ids{i};
  std::vector<const double*> th{theta};
  eval(ids, th, false, &f, nullptr, 0, &ok);
  if (!ok && !(gp[i].nug_type == NUG_PIVOT && gp[i].factored)) {
    if (gp[i].nug_type == NUG_ADAPTIVE) throw std::runtime_error("All attempts at factorization failed. Last return code 1");
    throw std::runtime_error("Unable to factorize matrix using selected nugget type");
  }
}

void Engine::ensure_linv(const std::vector<int>& ids) {
  std::vector<int> need;
  for (int i : ids) {
    if (!gp[i].factored) throw std::runtime_error("emulator has not been fit");
    if (!gp[i].linv) need.push_back(i);
  }
  if (need.empty()) return;
  if (!dLinv) {
    dKinv.reserve((size_t)B * MS);
    dGradOut.reserve((size_t)B * (D + 3));
    dGradPartial.reserve((size_t)B * grad_num_tiles(n) * (D + 3));
    dLinv.reserve((size_t)B * MS);      // (last: it is the one that says "all four are there")
  }
  upload_idx(need);
  BatchView v = view((int)need.size());
  launch_trtri(v, stream);
  for (int i : need) {
    gp[i].have_linv();    // (trtri used Kinv as scratch: K^-1 is gone)
  }
}

// for_gradient: an emulator whose pivoted factorisation skipped rows gets K^-1 WITHOUT the rows of L^-1 of the skipped
// pivots (they go to w2 and enter the gradient through launch_grad_lowrank, see kernels_cov.hip); otherwise the full K^-1.
void Engine::ensure_kinv(const std::vector<int>& ids, bool for_gradient) {
  ensure_linv(ids);
  std::vector<int> need;
  for (int i : ids) {
    const bool deficient = gp[i].permuted && gp[i].rank < n;
    const bool want_split = for_gradient && deficient;
    if (!gp[i].kinv || gp[i].kinv_split != want_split) need.push_back(i);
  }
  if (need.empty()) return;
  const size_t rowb = (size_t)LD * sizeof(double), wb = (size_t)n * sizeof(double);
  std::vector<int> split;
  for (int i : need)
    if (for_gradient && gp[i].permuted && gp[i].rank < n) {
      const int m = n - gp[i].rank;
      w2.erase(i);                              // (first: the old rows go before the new ones come)
      DevBuf<double>& buf = w2[i];
      buf.reserve((size_t)m * LD);
      double* rows = dLinv + (size_t)i * MS + (size_t)gp[i].rank * LD;
      HIPCK(hipMemcpy2DAsync(buf, rowb, rows, rowb, wb, m, hipMemcpyDeviceToDevice, stream));
      HIPCK(hipMemset2DAsync(rows, rowb, 0, wb, m, stream));
      split.push_back(i);
    }
  upload_idx(need);
  BatchView v = view((int)need.size());
  launch_kinv(v, n_cu, stream);
  for (int i : split) {
    double* rows = dLinv + (size_t)i * MS + (size_t)gp[i].rank * LD;
    HIPCK(hipMemcpy2DAsync(rows, rowb, w2[i], rowb, wb, n - gp[i].rank, hipMemcpyDeviceToDevice, stream));
  }
  for (int i : need) gp[i].have_kinv(false);
  for (int i : split) gp[i].have_kinv(true);
}

void Engine::grad_current(const std::vector<int>& ids, double* grad, int grad_ld) {
  if (ids.empty()) return;
  // alpha that an objective-only evaluation left out (the lazy-gradient line search: run_pool).  Where the same emulators also lack
  // L^-1 -- fresh factors, the usual case -- the chain runs on the panel stream UNDER the triangular inversion, as in
  // solve_and_collect, and its time-out words come back with the gradient; otherwise in front, on the main stream.
  std::vector<int> lazy, no_linv;
  for (int i : ids) {
    if (!gp[i].factored) throw std::runtime_error("emulator has not been fit");
    if (!gp[i].alpha) lazy.push_back(i);
    if (!gp[i].linv) no_linv.push_back(i);
  }
  const bool under = R == 1 && !lazy.empty() && lazy == no_linv;
  if (under) {
    upload_idx(lazy);
    HIPCK(hipEventRecord(evReady, stream));                // the index list is in place (the factor has been since the evaluation)
    HIPCK(hipStreamWaitEvent(pstream, evReady, 0));
    launch_backsolve_chain_on(pstream, view((int)lazy.size()), lazy, false);
    HIPCK(hipEventRecord(evGroup[14], pstream));
    ensure_linv(lazy);                                     // (the same list: the index list on the device stays as it is)
    HIPCK(hipStreamWaitEvent(stream, evGroup[14], 0));
    for (int i : lazy) gp[i].have_alpha();
    g_alpha_solves += (long long)lazy.size();
  } else {
    ensure_alpha(ids);
  }
  const int chain_epoch = bs_epoch;
  ensure_kinv(ids, true);
  upload_idx(ids);
  BatchView v = view((int)ids.size());
  launch_grad(v, dGradPartial, dGradOut, stream);
  for (int i : ids)
    if (gp[i].kinv_split) {
      const int m = n - gp[i].rank;
      DevBuf<double> part((size_t)m * ((n + 127) / 128) * (D + 1));
      SyncOnUnwind drained{stream};
      launch_grad_lowrank(v, i, w2.at(i), m, part, dGradOut, stream);
      HIPCK(hipStreamSynchronize(stream));
    }
  const int NQ = D + 3;
  std::vector<double> out((size_t)B * NQ);
  HIPCK(hipMemcpyAsync(out.data(), dGradOut, out.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
  std::vector<int> status;
  if (under) {
    status.assign(B, 0);
    HIPCK(hipMemcpyAsync(status.data(), dBsStatus, B * sizeof(int), hipMemcpyDeviceToHost, stream));
  }
  HIPCK(hipStreamSynchronize(stream));
  HIPCK(hipGetLastError());
  if (under) {
    // a chain that gave up on a wait (rare) left an unusable alpha under this gradient: solve it again, then the gradient again
    std::vector<int> again;
    for (int i : lazy)
      if (status[i] == chain_epoch) again.push_back(i);
    if (!again.empty()) {
      // One level deep, never more: every emulator of ids holds alpha and L^-1 by its flags now, so the call below finds `lazy` empty,
      // takes neither the chain nor this branch, and only launches the gradient again behind the repeat on `stream`.
      resolve_alpha_after_timeout(again);
      grad_current(ids, grad, grad_ld);
      return;
    }
  }
  const int nm = n_mean();
  std::vector<double> dpr(D + 2);
  for (size_t q = 0; q < ids.size(); ++q) {
    const int i = ids[q];
    const GPState& g = gp[i];
    double* gr = grad + q * grad_ld;
    const double* o = out.data() + (size_t)i * NQ;
    g.pri.dlogpdtheta(g.data, NC, g.nug_type, dpr.data());
    // GaussianProcess.py:751-780: 0.5 sum W dK/dtheta_p  -  d log prior / d theta_p
    if (uniform()) {
      // one shared length scale: dr2/dtheta_0 = r2 (Kernel.py:338-376) = the sum of the per-dimension terms
      double s = 0.;
      for (int p = 0; p < D; ++p) s += o[p];
      gr[nm] = s - dpr[0];
    } else {
      for (int p = 0; p < D; ++p) gr[nm + p] = o[p] - dpr[p];
    }
    gr[nm + NC] = o[D] - dpr[NC];
    if (g.nug_type == NUG_FIT) gr[nm + NC + 1] = 0.5 * std::exp(g.data[NC + 1]) * (o[D + 1] - o[D + 2]) - dpr[NC + 1];
    if (nm > 0) {
      // densegp_gpu.hpp:734-747: -(d mean / d beta)^T alpha
      std::vector<double> a(n), md((size_t)nm * n);
      HIPCK(hipMemcpy(a.data(), dAlpha + (size_t)i * RA * LD, n * sizeof(double), hipMemcpyDeviceToHost));
      unpermute(i, a.data());              // the mean derivatives below are in training order
      mean.mean_deriv(hX.data(), n, D, g.meanp.data(), nm, md.data());
      for (int p = 0; p < nm; ++p) {
        double s = 0.;
        for (int k = 0; k < n; ++k) s += md[(size_t)p * n + k] * a[k];
        gr[p] = -s;
      }
    }
  }
}

void Engine::unpermute(int i, double* vec) const {
  if (!gp[i].permuted) return;
  const int* P = hPerm.data() + (size_t)i * n;
  std::vector<double> tmp(vec, vec + n);
  for (int k = 0; k < n; ++k) vec[P[k]] = tmp[k];
}

void Engine::get_pivot(int i, int* perm_out, int* rank_out) {
  if (!gp[i].factored) throw std::runtime_error("emulator has not been fit");
  for (int k = 0; k < n; ++k) perm_out[k] = gp[i].permuted ? hPerm[(size_t)i * n + k] : k;
  if (rank_out) *rank_out = gp[i].permuted ? gp[i].rank : n;
}

void Engine::get_K(int i, double* out) {
  if (!gp[i].has_data) throw std::runtime_error("emulator has not been fit");
  DevBuf<double> tmp((size_t)n * n);
  std::vector<int> ids{i};
  upload_params(ids);
  BatchView v = view(1);
  v.X = dX;          // training order, also for a pivoted emulator
  v.XS = 0;
  launch_cov_full(v, i, tmp, stream);
  HIPCK(hipMemcpyAsync(out, tmp, (size_t)n * n * sizeof(double), hipMemcpyDeviceToHost, stream));
  HIPCK(hipStreamSynchronize(stream));
}

void Engine::get_invQ(int i, double* out) {
  std::vector<int> ids{i};
  ensure_kinv(ids, false);
  DevBuf<double> tmp((size_t)n * n);
  launch_extract(dKinv + (size_t)i * MS, LD, n, tmp, 2, stream);
  HIPCK(hipMemcpyAsync(out, tmp, (size_t)n * n * sizeof(double), hipMemcpyDeviceToHost, stream));
  HIPCK(hipStreamSynchronize(stream));
  if (gp[i].permuted) {          // K^-1 of the pivoted matrix back to training order
    const int* P = hPerm.data() + (size_t)i * n;
    std::vector<double> t(out, out + (size_t)n * n);
    for (int a = 0; a < n; ++a)
      for (int b = 0; b < n; ++b) out[(size_t)P[a] * n + P[b]] = t[(size_t)a * n + b];
  }
}

void Engine::get_invQt(int i, double* out) {
  ensure_alpha({i});
  HIPCK(hipStreamSynchronize(stream));      // (a repeat after a time-out is still in flight)
  HIPCK(hipMemcpy(out, dAlpha + (size_t)i * RA * LD, n * sizeof(double), hipMemcpyDeviceToHost));
  unpermute(i, out);
}

void Engine::pivot_cholesky(const double* Ain, int n, double* L_out, int* P_out, int* rank_out) {
  if (n < 1) throw std::runtime_error("A must have shape (n,n)");
  // _check_cholesky_inputs, linalg/cholesky.py:196-222
  for (int i = 0; i < n; ++i) {
    if (!(Ain[(size_t)i * n + i] > 0.)) throw std::runtime_error("not pd: non-positive diagonal elements");
    for (int j = 0; j < i; ++j) {
      const double a = Ain[(size_t)i * n + j], b = Ain[(size_t)j * n + i];
      if (!(std::fabs(a - b) <= 1e-7 * std::fabs(b))) throw std::runtime_error("A must be symmetric");
    }
  }
  // padded copy: NP x NP with the identity beyond n, so that the blocked trailing update can be used as it is
  const int NPp = roundup(n, TILE);
  std::vector<double> hA((size_t)NPp * NPp, 0.);
  for (int i = 0; i < NPp; ++i) {
    if (i < n) std::memcpy(hA.data() + (size_t)i * NPp, Ain + (size_t)i * n, (size_t)n * sizeof(double));
    else hA[(size_t)i * NPp + i] = 1.0;
  }
  DevBuf<double> dA_(hA.size()), dW(pstrf_work_doubles(NPp));
  DevBuf<int> dI((size_t)n + 2);
  BatchView v{};
  v.n = n; v.D = 1; v.NP = NPp; v.LD = NPp; v.MS = (size_t)NPp * NPp; v.PS = 0; v.kernel_type = 0;
  v.A = dA_; v.R = 0; v.RA = 0; v.idx = nullptr; v.nb = 1;
  HIPCK(hipMemcpy(dA_, hA.data(), hA.size() * sizeof(double), hipMemcpyHostToDevice));
  launch_pstrf_begin(v, dI, dI + n, dI + n + 1, dW, nullptr);
  int rk = -1;
  for (int k0 = 0; k0 < n; k0 += NBI) {
    const bool first_half = (k0 % TILE) == 0;
    launch_pstrf_panel(v, k0, std::min(NBI, n - k0), dI, dI + n, dW, nullptr);
    HIPCK(hipMemcpy(&rk, dI + n, sizeof(int), hipMemcpyDeviceToHost));
    if (rk >= 0) break;
    if (first_half) launch_update_narrow(v, k0 + NBI, k0, k0 + NBI, nullptr);
    launch_update_trailing(v, first_half ? k0 + TILE : k0 + NBI, k0, k0 + NBI, nullptr);
  }
  launch_pstrf_tail(v, dI, dI + n, nullptr);
  std::vector<int> hi((size_t)n + 2);
  HIPCK(hipMemcpy(hi.data(), dI, hi.size() * sizeof(int), hipMemcpyDeviceToHost));
  HIPCK(hipMemcpy(hA.data(), dA_, hA.size() * sizeof(double), hipMemcpyDeviceToHost));
  for (int i = 0; i < n; ++i) std::memcpy(L_out + (size_t)i * n, hA.data() + (size_t)i * NPp, (size_t)n * sizeof(double));
  if (hi[n + 1] != 0) throw std::runtime_error("not pd: no positive pivot");
  for (int i = 0; i < n; ++i) {
    P_out[i] = hi[i];
    for (int j = i + 1; j < n; ++j) L_out[(size_t)i * n + j] = 0.;
  }
  if (rank_out) *rank_out = hi[n];
}

void Engine::get_chol(int i, double* out) {
  if (!gp[i].factored) throw std::runtime_error("emulator has not been fit");
  DevBuf<double> tmp((size_t)n * n);
  launch_extract(dA + (size_t)i * MS, LD, n, tmp, 1, stream);
  HIPCK(hipMemcpyAsync(out, tmp, (size_t)n * n * sizeof(double), hipMemcpyDeviceToHost, stream));
  HIPCK(hipStreamSynchronize(stream));
}

}  // namespace mogp
