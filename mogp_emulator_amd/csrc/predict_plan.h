// How the prediction family of Engine (engine_predict.hip), its Hessian (engine_hessian.hip) and the analyses of analysis.h (analysis_*.hip:
// predict_mixture, cross_validate, sample_posterior, alc, alc_batch, predict_cov) cut their work to a byte budget, the index tables of their passes, and where the mean-function terms of a prediction are
// staged.  Plain host arithmetic with no HIP in it, so that a host compiler takes it and tests/c/predict_plan_check.cpp, mixture_plan_check.cpp,
// cv_plan_check.cpp, sample_plan_check.cpp, alc_plan_check.cpp, alc_batch_plan_check.cpp, local_plan_check.cpp, vecchia_plan_check.cpp, iter_plan_check.cpp and local_args_check.cpp (the refusals
// and the LDS layout of the LocalGP handle, engine_local.hip) can check it without a device.  The caps that need the device (MOGP_KS_BUDGET_GB, free memory) are passed in.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <stdexcept>
#include <string>
#include <vector>

namespace mogp {

// query points per chunk of a prediction of nb emulators: as many whole 128-point tiles of cross-covariance rows (LD doubles per point and
// emulator) as cap_bytes holds, at least one tile, at most the m points rounded up to tiles (one chunk)
inline int predict_chunk_points(double cap_bytes, int nb, int LD, int m) {
  const long all = ((long)m + 127) / 128 * 128;
  const long MC = (long)(cap_bytes / ((double)nb * LD * 8.0)) / 128 * 128;
  return (int)std::max<long>(128, std::min<long>(MC, all));
}

// the chunk budget of implausibility / implausibility_top
constexpr double implausibility_cap_bytes = 6.0e9;

// base rows per chunk of pass 2 of Engine::sobol: per row the D inputs of AB_i, its nb means, predict()'s R dot-product rows per emulator
// (analytic mean only) and the basis columns of the mean function; whole 128-row tiles, at least one, never more than the N rows
inline long sobol_chunk_rows(double cap_bytes, int D, int nb, int R, int mean_kind, int n_poly_terms, long N) {
  const double per_row = 8.0 * ((double)D + (double)nb * (1.0 + (R > 1 ? R : 0)) + (mean_kind == 3 ? 2.0 * n_poly_terms + 1.0 : 1.0));
  const long CH = (long)(cap_bytes / per_row) / 128 * 128;
  return std::min<long>(std::max<long>(128, CH), N);
}

// emulators per group of Engine::hessian: as many of the n_good as the budget holds at per_bytes of scratch each, at least one
inline std::size_t hessian_group_size(double budget, double per_bytes, std::size_t n_good) {
  return (std::size_t)std::max(1.0, std::min((double)n_good, std::floor(budget / per_bytes)));
}

// bytes of scratch one emulator of a group of Engine::hessian takes: the D planes M_p (NPh x NPh, NPh = hess_np(n)), Xs, V, U and z, the
// trace table ((D + 1) x (D + 2)) in TG partial slots and its sum, the pair table (D x D) in PGR slots and its sum (launch.h has TG / PGR)
inline double hessian_scratch_bytes(int NPh, int D, int TG, int PGR) {
  const std::size_t plane = (std::size_t)NPh * NPh;
  const int TS = (D + 1) * (D + 2);
  return 8.0 * ((double)D * plane + (double)NPh * (3.0 * D + 1.0) + (double)TS * (TG + 1.0) + (double)D * D * (PGR + 1.0));
}

// The one rule for "slots that fit beside this engine" (fit_map_from, predict_mixture, cross_validate): half of the free device memory
// at bytes_per_slot each, at least one.
inline long slots_in_half_of(double free_bytes, double bytes_per_slot) { return (long)std::max(1.0, std::floor(0.5 * free_bytes / bytes_per_slot)); }
// a slot of a replica engine: A, L^-1 and K^-1 (MS doubles each) plus the small per-emulator buffers
inline double replica_slot_bytes(std::size_t MS, int LD) { return 3.0 * (double)MS * 8.0 + 16.0 * LD * 8.0; }
// replicas beyond what fills the device buy nothing: the batched kernels of a factorisation stay below 4096 tile rows per launch
inline long replica_slot_bound(int NP, int TILE) { return 4095 / std::max(1, NP / TILE) + 1; }

// predict_mixture: how many replica slots one pass takes and how many query points one chunk.  The E * S (emulator, sample) pairs
// are laid out emulator-major, sample-ascending, and pass g takes the pairs [g * slots, (g + 1) * slots): a slot always holds one whole
// sample, and a contiguous cut of that order never puts a later sample of an emulator in front of an earlier one.  slots: at least one,
// never more than the E * S pairs, the `device_slots` the device holds beside the source engine, or max_slots (0: the library's choice);
// above 8 the library's own choice is a multiple of 8, as fit_map's is.  points: max_points where given (at least one, at most m), else the
// chunk rule of predict() for `slots` emulators (predict_chunk_points).
struct MixturePlan {
  long slots;
  int points;
};
inline MixturePlan mixture_plan(long E, long S, int LD, long device_slots, int m, int max_slots, int max_points, double cap_bytes) {
  const long pairs = std::max<long>(1, E * S);
  long slots = std::min(pairs, std::max<long>(1, device_slots));
  if (max_slots > 0) slots = std::min<long>(slots, max_slots);
  else if (slots > 8 && slots < pairs) slots -= slots % 8;
  slots = std::max<long>(1, slots);
  int points;
  if (max_points > 0) points = std::max(1, std::min(max_points, std::max(1, m)));
  else points = predict_chunk_points(cap_bytes, (int)std::min<long>(slots, 1L << 30), LD, m);
  return {slots, points};
}

// cross_validate: how many (emulator, fold) pairs one pass of the ScratchFactor takes.  The E * k pairs are laid out emulator-major,
// fold-ascending, and pass g takes the pairs [g * slots, (g + 1) * slots).  slots: at least one, never more than the E * k pairs, the
// `device_slots` that half of the free memory holds at 3 NPsub^2 doubles per slot, NPsub = scratch_np(largest fold) (factor, L^-1 and its scratch; cv_slot_bytes), the batch
// bound predict_mixture's replica engine observes (cv_slot_bound: the batched kernels of a factorisation stay in the range of tiles per
// launch they run at there, and a slot is one grid row), or max_slots (0: the library's choice).
// the padded size of the matrices of a ScratchFactor of `rows` rows (engine_internal.h): the rows and one right-hand side, in whole tiles
inline long scratch_np(long rows) { return (rows + 128) / 128 * 128; }
inline double cv_slot_bytes(int NPsub) { return 3.0 * (double)NPsub * (double)NPsub * 8.0; }
inline long cv_slot_bound(int NPsub) { return std::min<long>(65535, 4095 / std::max(1, NPsub / 128) + 1); }
inline long cv_plan(long E, long k, int NPsub, long device_slots, int max_slots) {
  const long pairs = std::max<long>(1, E * k);
  long slots = std::min(pairs, std::max<long>(1, device_slots));
  slots = std::min(slots, cv_slot_bound(NPsub));
  if (max_slots > 0) slots = std::min<long>(slots, max_slots);
  return std::max<long>(1, slots);
}

// The folds of cross_validate from the labels (n) of the training points: size (k) = points per fold, nsub = the largest fold,
// folds (k, nsub) = the points of every fold in ascending order, -1 behind the end of a short one.  Throws for a label outside [0, k)
// and for an empty fold.
struct CvFolds {
  std::vector<int> size;
  int nsub;
  std::vector<int> folds;
};
inline CvFolds cv_folds(const int* labels, int n, int k) {
  CvFolds c{std::vector<int>(k, 0), 0, {}};
  for (int i = 0; i < n; ++i) {
    if (labels[i] < 0 || labels[i] >= k) throw std::runtime_error("cross_validate: fold label " + std::to_string(labels[i]) + " of point " + std::to_string(i) + " is outside [0, " + std::to_string(k) + ")");
    c.size[labels[i]] += 1;
  }
  for (int f = 0; f < k; ++f) {
    if (c.size[f] == 0) throw std::runtime_error("cross_validate: fold " + std::to_string(f) + " is empty");
    c.nsub = std::max(c.nsub, c.size[f]);
  }
  c.folds.assign((std::size_t)k * c.nsub, -1);
  std::vector<int> fillp(k, 0);
  for (int i = 0; i < n; ++i) c.folds[(std::size_t)labels[i] * c.nsub + fillp[labels[i]]++] = i;
  return c;
}

// The slot table (slots, 4) of the pass of cross_validate that starts at pair p0 and holds cnt pairs: per slot
// [emulator of the engine, its position in ids, fold, size of the fold]; the slots behind cnt are [-1, 0, 0, 0] -- not used: an identity,
// so that the batch factorises.
inline void cv_pass_table(long p0, long cnt, long slots, long k, const int* ids, const int* size, int* tab) {
  for (long s = 0; s < slots; ++s) {
    const long e = (p0 + s) / k, f = (p0 + s) % k;
    int* t = tab + 4 * s;
    if (s < cnt) { t[0] = ids[e]; t[1] = (int)e; t[2] = (int)f; t[3] = size[f]; }
    else { t[0] = -1; t[1] = t[2] = t[3] = 0; }
  }
}

// sample_posterior: how many emulators one pass takes and how many draws one chunk.  The emulators go in passes [p0, p0 + slots)
// in caller order and, inside a pass, the S draws in chunks [s0, s0 + draws): every (emulator, draw) pair is computed exactly once.
// Bytes of one slot (sample_slot_bytes):
//   Sigma* and what predict_full_cov builds it from: K* (MP x LD), V (NP x MP), Sigma* (m x m), the R dot-product rows   (MP = roundup(m, 128))
//   the ScratchFactor's factor matrix NPs x NPs (NPs = scratch_np(m)) and its small per-slot rows, mu* (m)
//   Z and Y of one chunk: 2 x roundup(draws, 64) x MP doubles (sample_apply_kernel reads whole tiles of 64 draws)
// and a pass never takes more than HALF of the free device memory.  draws: max_draws where given, else SAMPLE_DEFAULT_DRAWS, at most S and
// SAMPLE_MAX_DRAWS (a chunk's draws are one grid dimension of the generator), cut to whole tiles of 64 where one slot would not fit
// otherwise.  slots: what the budget holds at that chunk, at most E, max_slots where given, the batch bound of cv_plan and what
// predict_full_cov's own 64 GB rule allows.  Throws when one slot with a single tile of draws does not fit, when one emulator trips the
// 64 GB rule, and for negative max_slots / max_draws.
constexpr long SAMPLE_DRAW_TILE = 64, SAMPLE_DEFAULT_DRAWS = 1024, SAMPLE_MAX_DRAWS = 32768;
struct SamplePlan {
  long slots, draws;
};
inline long sample_mp(int m) { return ((long)m + 127) / 128 * 128; }
inline long sample_nps(int m) { return scratch_np(m); }
inline long sample_draw_rows(long draws) { return (draws + SAMPLE_DRAW_TILE - 1) / SAMPLE_DRAW_TILE * SAMPLE_DRAW_TILE; }
inline double sample_fixed_bytes(int m, int LD, int NP, int R) {
  const double MP = (double)sample_mp(m), NPs = (double)sample_nps(m);
  return 8.0 * (MP * LD + (double)NP * MP + (double)m * m + (double)R * m + NPs * NPs + 16.0 * NPs + (double)m);
}
inline double sample_draw_bytes(int m, long draws) { return 2.0 * 8.0 * (double)sample_draw_rows(draws) * (double)sample_mp(m); }
inline double sample_slot_bytes(int m, int LD, int NP, int R, long draws) { return sample_fixed_bytes(m, LD, NP, R) + sample_draw_bytes(m, draws); }
inline double fullcov_rule_bytes(int m, int LD) { return 8.0 * ((double)LD * (double)sample_mp(m) * 2.0 + (double)m * m); }
inline SamplePlan sample_plan(long E, int m, long S, int LD, int NP, int R, double free_bytes, int max_slots, int max_draws) {
  if (max_slots < 0 || max_draws < 0) throw std::runtime_error("sample_posterior: max_slots and max_draws must not be negative");
  if (fullcov_rule_bytes(m, LD) > 64.0e9)
    throw std::runtime_error("sample_posterior: " + std::to_string(m) + " test points need more than 64 GB of device scratch; use fewer points per call");
  const double budget = 0.5 * free_bytes, fixed = sample_fixed_bytes(m, LD, NP, R);
  if (fixed + sample_draw_bytes(m, 1) > budget)
    throw std::runtime_error("sample_posterior: one emulator at " + std::to_string(m) + " test points needs " +
                             std::to_string((long long)(fixed + sample_draw_bytes(m, 1))) +
                             " bytes of device scratch, more than half of the free device memory; use fewer points per call");
  long draws = std::max<long>(1, std::min<long>(std::max<long>(1, S), max_draws > 0 ? max_draws : SAMPLE_DEFAULT_DRAWS));
  draws = std::min(draws, SAMPLE_MAX_DRAWS);
  if (fixed + sample_draw_bytes(m, draws) > budget) {
    const long tiles = (long)std::floor((budget - fixed) / sample_draw_bytes(m, 1));
    draws = std::min(draws, std::max<long>(1, tiles) * SAMPLE_DRAW_TILE);
  }
  long slots = (long)std::max(1.0, std::floor(budget / (fixed + sample_draw_bytes(m, draws))));
  slots = std::min(slots, std::max<long>(1, E));
  slots = std::min(slots, (long)std::max(1.0, std::floor(64.0e9 / fullcov_rule_bytes(m, LD))));
  slots = std::min(slots, cv_slot_bound((int)sample_nps(m)));
  if (max_slots > 0) slots = std::min<long>(slots, max_slots);
  return {std::max<long>(1, slots), draws};
}
// The jitter ladder of sample_posterior: rung t = 0 .. SAMPLE_LADDER_RUNGS - 1 adds 10^-6 * 10^t * (mean diagonal of Sigma*) -- the adaptive
// rule of the fit applied to the predictive covariance, the factor ten applied t times as there.
constexpr int SAMPLE_LADDER_RUNGS = 5;
inline double sample_ladder_delta(int t, double mean_diag) {
  double d = mean_diag * 1e-6;
  for (int i = 0; i < t; ++i) d *= 10.0;
  return d;
}

// alc: how many emulators one group takes and how many reference points one chunk.  The emulators go in groups [e0, e0 + slots) in
// caller order and, inside a group, the m_r reference points in chunks [c0, c0 + points), points a multiple of 128: a chunk is a run of whole
// 128-point tiles of the reference set, and the partial sums of the criterion are kept per GLOBAL tile, so neither number changes a bit of
// the result.  Bytes of one slot (alc_slot_bytes), MP_c = roundup(m_c, 128), tiles_r = ceil(m_r / 128):
//   V_c (NP x MP_c), V_r of one chunk (NP x points), the K* scratch both are built from (LD x max(MP_c, points)), the partials (tiles_r x MP_c)
// and a group never takes more than HALF of the free device memory (slots_in_half_of).  points: max_points rounded down to a multiple of
// 128 where given (at least 128), else the whole reference set; cut to what one slot holds where that does not fit.  slots: what the budget
// holds at that chunk, at most E, 65535 (a slot is one grid row of the variance launches) and max_slots where given.  Throws when one
// emulator with one 128-point chunk does not fit, and for negative max_slots / max_points.
struct AlcPlan {
  long slots, points;
};
inline long alc_mp(long m) { return (m + 127) / 128 * 128; }
inline double alc_slot_bytes(int NP, int LD, long MPc, long points, long tiles_r) {
  return 8.0 * ((double)NP * MPc + (double)NP * points + (double)LD * std::max(MPc, points) + (double)tiles_r * MPc);
}
inline AlcPlan alc_plan(long E, long m_c, long m_r, int LD, int NP, double free_bytes, int max_slots, int max_points) {
  if (max_slots < 0 || max_points < 0) throw std::runtime_error("alc_criterion: max_slots and max_points must not be negative");
  const long MPc = alc_mp(std::max<long>(1, m_c)), all = alc_mp(std::max<long>(1, m_r)), tiles_r = all / 128;
  const double budget = 0.5 * free_bytes;
  if (alc_slot_bytes(NP, LD, MPc, 128, tiles_r) > budget)
    throw std::runtime_error("alc_criterion: one emulator at " + std::to_string(m_c) + " candidates and " + std::to_string(m_r) +
                             " reference points needs " + std::to_string((long long)alc_slot_bytes(NP, LD, MPc, 128, tiles_r)) +
                             " bytes of device scratch, more than half of the free device memory; use fewer points per call");
  long points = max_points > 0 ? std::max<long>(128, (long)max_points / 128 * 128) : all;
  points = std::min(points, all);
  if (alc_slot_bytes(NP, LD, MPc, points, tiles_r) > budget) {
    // the largest multiple of 128 one slot holds: first with the K* scratch sized by the chunk, then -- below MP_c -- by the candidates
    const double fixed = (double)NP * MPc + (double)tiles_r * MPc, doubles = budget / 8.0;
    long fit = (long)std::floor((doubles - fixed) / ((double)NP + LD));
    if (fit < MPc) fit = (long)std::floor((doubles - fixed - (double)LD * MPc) / (double)NP);
    points = std::max<long>(128, std::min(points, fit / 128 * 128));
  }
  long slots = slots_in_half_of(free_bytes, alc_slot_bytes(NP, LD, MPc, points, tiles_r));
  slots = std::min(slots, std::max<long>(1, E));
  slots = std::min<long>(slots, 65535);
  if (max_slots > 0) slots = std::min<long>(slots, max_slots);
  return {std::max<long>(1, slots), points};
}
// alc_batch: how many emulators one group takes.  V_r stays resident across the picks, so the reference set is ONE chunk, and both
// V carry ext = roundup(steps, 16) conditioning rows behind their base rows (steps = pending points + picks).  Bytes of one slot:
//   alc_slot_bytes with NP + ext rows and points = MP_r = roundup(m_r, 128)
//   + 8 NP max(MP_c, MP_r)                      the stored V as launch_predict_v_store leaves it, before it is copied into the wider buffer
//   + 8 (NP / 128 + 2) max(MP_c, MP_r)          the partial sums of the predictive variance and the unused dot products
//   + 8 (2 MP_c + MP_r + 2 ext)                 tracked variances of both sets, the scores, the score and the denominator of every pick
//   + 4 (2 MP_c + ext)                          mask, degenerate flags, picks
// A group takes at most half of the free device memory.  select = "each": groups of `slots` emulators in caller order, at most E, 65535
// and max_slots where given; one emulator's picks do not depend on its group.  select = "total" (total = true): every emulator of the call
// must sit in one group, since each step's score sums over them; refused otherwise, with the bytes named.  Throws when one emulator does not fit.
inline long alc_ext_rows(long steps) { return (std::max<long>(1, steps) + 15) / 16 * 16; }
inline double alc_batch_slot_bytes(int NP, int LD, long MPc, long MPr, long tiles_r, long ext) {
  const double mpx = (double)std::max(MPc, MPr);
  return alc_slot_bytes(NP + (int)ext, LD, MPc, MPr, tiles_r) + 8.0 * (double)NP * mpx + 8.0 * (double)(NP / 128 + 2) * mpx +
         8.0 * (double)(2 * MPc + MPr + 2 * ext) + 4.0 * (double)(2 * MPc + ext);
}
inline long alc_batch_plan(long E, long m_c, long m_r, long steps, int LD, int NP, double free_bytes, int max_slots, bool total) {
  if (max_slots < 0) throw std::runtime_error("alc_batch: max_slots must not be negative");
  const long MPc = alc_mp(std::max<long>(1, m_c)), MPr = alc_mp(std::max<long>(1, m_r));
  const double per = alc_batch_slot_bytes(NP, LD, MPc, MPr, MPr / 128, alc_ext_rows(steps));
  const std::string shape = std::to_string(m_c) + " candidates, " + std::to_string(m_r) + " reference points and " + std::to_string(steps) + " steps";
  if (per > 0.5 * free_bytes)
    throw std::runtime_error("alc_batch: one emulator at " + shape + " needs " + std::to_string((long long)per) +
                             " bytes of device scratch, more than half of the free device memory; use fewer points per call");
  long slots = std::min<long>(slots_in_half_of(free_bytes, per), std::max<long>(1, E));
  slots = std::min<long>(slots, 65535);
  if (total) {
    if (slots < E)
      throw std::runtime_error("alc_batch: select=\"total\" needs all " + std::to_string(E) + " emulators of a device in one group: at " + shape +
                               " that is " + std::to_string((long long)(per * (double)E)) + " bytes of device scratch, and half of the free memory is " +
                               std::to_string((long long)(0.5 * free_bytes)) + "; use fewer points per call or select=\"each\"");
    return slots;       // (max_slots does not apply)
  }
  if (max_slots > 0) slots = std::min<long>(slots, max_slots);
  return std::max<long>(1, slots);
}
// predict_cov: V_1, V_2, the output and the K* scratch of one emulator against the 64 GB rule of predict_full_cov
inline double predict_cov_rule_bytes(long m1, long m2, int LD, int NP) {
  const double MP1 = (double)alc_mp(m1), MP2 = (double)alc_mp(m2);
  return 8.0 * ((double)NP * (MP1 + MP2) + (double)m1 * (double)m2 + (double)LD * std::max(MP1, MP2));
}

// The refusals LocalGP::predict, vecchia_neighbours and vecchia_loglik share (engine_local.hip); `who` is the prefix of the message.
//   local_check_kernel  kt: 0 squared exponential, 1 Matern 5/2
//   local_check_k       1 <= k <= LOCAL_MAX_K (launch.h: 126, passed in) and k <= N; vecchia: k <= N - 1, a point's neighbours come before it
//   local_check_hyper   sigma^2, nugget and jitter, then the D scales (local_check_scales: all that vecchia_neighbours needs)
inline void local_check_kernel(const std::string& who, int kt) {
  if (kt != 0 && kt != 1) throw std::runtime_error(who + ": the kernel must be a function of one scaled distance (squared exponential or Matern 5/2)");
}
inline void local_check_k(const std::string& who, long N, int k, bool vecchia, int max_k) {
  const long top = vecchia ? N - 1 : N;
  if (top < 1 || k < 1 || k > max_k || k > top)
    throw std::runtime_error(who + ": n_neighbours must be between 1 and " + std::to_string(std::min<long>(top, max_k)));
}
inline void local_check_scales(const std::string& who, int D, const double* scale) {
  for (int d = 0; d < D; ++d)
    if (!(scale[d] > 0.) || !std::isfinite(scale[d])) throw std::runtime_error(who + ": the scales must be positive and finite");
}
inline void local_check_hyper(const std::string& who, int D, const double* scale, double sigma2, double nugget, double jitter) {
  if (!(sigma2 > 0.) || !std::isfinite(sigma2) || !(nugget >= 0.) || !std::isfinite(nugget) || !(jitter >= 0.) || !std::isfinite(jitter))
    throw std::runtime_error(who + ": sigma^2 must be positive and finite, nugget and jitter finite and not negative");
  local_check_scales(who, D, scale);
}

// The dynamic LDS of local_gp_kernel and vecchia_ll_kernel (kernels_local.hip), offsets in doubles: chol128_dev's own, the exponential's
// table tab (256), the targets yv (128), with the gradient w and alpha (wv, av: 128 each) and the partial sums of a_d and b_d (reda, redb:
// 256 each), the gathered points pts (128 rows of ld doubles) and chol128_dev's status word info (in the dynamic region: a static one
// would misalign it).  constexpr, so that the kernels and the host read the same text.
constexpr int LOCAL_CHOL_LDS_DOUBLES = 128 * 18 + 256 + 256;      // chol128_dev.h C128_LDS_DOUBLES (kernels_local.hip asserts it)
struct LocalLds {
  int tab, yv, wv, av, reda, redb, pts, ld, info, doubles;
  constexpr LocalLds(int D, bool grad)
      : tab(LOCAL_CHOL_LDS_DOUBLES), yv(tab + 256), wv(yv + 128), av(wv + (grad ? 128 : 0)), reda(av + (grad ? 128 : 0)),
        redb(reda + (grad ? 256 : 0)), pts(redb + (grad ? 256 : 0)),
        ld(D | 1),                                                 // odd row stride: rows a lane apart fall on different banks
        info(pts + 128 * ld), doubles(info + 2) {}
};
inline std::size_t local_lds_bytes(int D, bool grad) { return sizeof(double) * (std::size_t)LocalLds(D, grad).doubles; }

// LocalGP::predict (engine_local.hip): how many queries one pass takes and how many persistent workgroups factor their local matrices.
// Bytes of one query of a pass (local_point_bytes): its raw and its scaled coordinates (2 D doubles), k neighbour indices and the ok flag
// (ints), radius, mean and variance (doubles).  Every workgroup owns wg_bytes of scratch (launch.h LOCAL_WG_DOUBLES).
//   grid    LOCAL_GRID_PER_CU workgroups per compute unit, never more than the queries of a pass, at least one
//   points  max_points where given, else what half of the free device memory holds beside the scratch of a full grid; at most m and
//           LOCAL_MAX_PASS, at least one
// Neither changes a bit of a result: a query's neighbours and its factorisation depend on nothing but the query.  Throws for a negative
// max_points and when one query beside one workgroup's scratch does not fit.
constexpr long LOCAL_GRID_PER_CU = 4, LOCAL_MAX_PASS = 1L << 20;
struct LocalPlan {
  long points;
  int grid;
};
inline double local_point_bytes(int D, int k) { return 8.0 * (2.0 * D + 3.0) + 4.0 * (k + 1.0); }
inline LocalPlan local_plan(long m, int D, int k, int n_cu, double free_bytes, int max_points, double wg_bytes) {
  if (max_points < 0) throw std::runtime_error("predict_local: max_points must not be negative");
  const long full = LOCAL_GRID_PER_CU * std::max(1, n_cu);
  const double budget = 0.5 * free_bytes, per = local_point_bytes(D, k);
  const long want = std::max<long>(1, std::min<long>(m, LOCAL_MAX_PASS));
  long points;
  if (max_points > 0) {
    points = std::min<long>(want, max_points);
    if ((double)points * per + (double)std::min(points, full) * wg_bytes > budget)
      throw std::runtime_error("predict_local: " + std::to_string(points) + " queries per pass need more than half of the free device memory; use a smaller max_points");
  } else {
    const double left = budget - (double)std::min(want, full) * wg_bytes;
    if (left < per)
      throw std::runtime_error("predict_local: the scratch of " + std::to_string(std::min(want, full)) +
                               " workgroups does not fit half of the free device memory");
    points = std::min<long>(want, (long)std::floor(left / per));
  }
  return {points, (int)std::min(points, full)};
}

// LocalGP::vecchia_loglik (engine_local.hip): how many points one launch takes and how many persistent workgroups factor their local
// matrices.  Held for the whole design, whatever the launches (vecchia_fixed_bytes): per point the term and, with the gradient, its D + 2
// derivatives (doubles) and the ok flag (int); two buffers of ceil(N / 1024) partial sums per column.  Every workgroup owns wg_bytes of
// scratch (launch.h LOCAL_WG_DOUBLES, VECCHIA_WG_DOUBLES with the gradient).
//   points  max_points where given, else LOCAL_MAX_PASS; at most N, at least one
//   grid    LOCAL_GRID_PER_CU workgroups per compute unit, never more than the points of a launch, at least one
// Neither changes a bit of a result: a point's term depends on nothing but the point, and the sum runs over the whole design in blocks of 1024
// afterwards.  Throws for a negative max_points and when the whole does not fit half of the free device memory.  What the handle holds
// from earlier calls is not free any more but is reused: vecchia_held_bytes of its buffers (elements: out, red and scratch doubles, ok ints)
// count as free.
inline double vecchia_held_bytes(std::size_t out, std::size_t red, std::size_t scratch, std::size_t ok) {
  return 8.0 * ((double)out + (double)red + (double)scratch) + 4.0 * (double)ok;
}
struct VecchiaPlan {
  long points;
  int grid;
  long blocks;      // partial sums per column after the first pass of the sum
};
inline long vecchia_blocks(long N) { return (std::max<long>(1, N) + 1023) / 1024; }
inline double vecchia_fixed_bytes(long N, int D, bool grad) {
  const double cols = grad ? D + 3.0 : 1.0;
  return 8.0 * cols * (double)N + 4.0 * (double)N + 2.0 * 8.0 * cols * (double)vecchia_blocks(N);
}
inline VecchiaPlan vecchia_plan(long N, int D, bool grad, int n_cu, double free_bytes, int max_points, double wg_bytes) {
  if (max_points < 0) throw std::runtime_error("vecchia_loglik: max_points must not be negative");
  const long full = LOCAL_GRID_PER_CU * std::max(1, n_cu);
  long points = std::max<long>(1, std::min<long>(N, LOCAL_MAX_PASS));
  if (max_points > 0) points = std::min<long>(points, max_points);
  const long grid = std::min(points, full);
  const double need = vecchia_fixed_bytes(N, D, grad) + (double)grid * wg_bytes;
  if (need > 0.5 * free_bytes)
    throw std::runtime_error("vecchia_loglik: " + std::to_string((long long)need) + " bytes of device scratch for " + std::to_string(N) +
                             " points are more than half of the free device memory");
  return {points, (int)grid, vecchia_blocks(N)};
}

// Iterative exact prediction on the LocalGP handle (engine_iter.hip): the refusals, the device memory it holds and the query passes.
//   iter_check_hyper   the hyperparameters of local_check_hyper, and a nugget that is positive: the preconditioner divides by it
//   iter_check_rank    0 <= rank <= min(N, ITER_MAX_RANK); 0 is plain conjugate gradients
//   iter_check_solve   at least one right-hand side, rtol inside (0, 1), max_iter >= 1
//   iter_held_bytes    L (8 N rank), G and its inverse, ITER_PANELS panels of ITER_PLAN_COLS columns, the remaining diagonal, the partial sums
//                      of the tall-skinny product (ceil(N / ITER_PLAN_SEG) rank ITER_PLAN_COLS, and two rank x ITER_PLAN_COLS blocks behind
//                      them), of the dots (ceil(N / 1024) ITER_PLAN_COLS) and of the pivot search (2 ceil(N / 1024))
//   iter_check_memory  refuses, before anything is allocated, what does not fit half of the free device memory (what the handle holds of
//                      it already counts as free: it is reused)
//   iter_plan          queries per pass: max_points where given, else what the rest of that half holds at iter_point_bytes per query (raw and
//                      scaled coordinates and the 16 output columns of the rectangular product), at most m and LOCAL_MAX_PASS, at least one;
//                      blocks = the variance's solves per pass, ITER_PLAN_COLS queries each.  No bit of a result depends on either.
constexpr int ITER_MAX_RANK = 1024, ITER_PLAN_COLS = 32, ITER_PANELS = 8, ITER_PLAN_SEG = 4096, ITER_PLAN_DOT = 1024;
inline void iter_check_hyper(const std::string& who, int D, const double* scale, double sigma2, double nugget) {
  local_check_hyper(who, D, scale, sigma2, nugget, 0.);
  if (!(nugget > 0.)) throw std::runtime_error(who + ": the nugget must be positive (the preconditioner divides by it)");
}
inline void iter_check_rank(const std::string& who, long N, int rank) {
  const long top = std::min<long>(N, ITER_MAX_RANK);
  if (rank < 0 || rank > top) throw std::runtime_error(who + ": precond_rank must be between 0 and min(N, 1024) = " + std::to_string(top));
}
inline void iter_check_solve(const std::string& who, long cols, double rtol, int max_iter) {
  if (cols < 1) throw std::runtime_error(who + ": at least one right-hand side is needed");
  if (!(rtol > 0.) || !(rtol < 1.)) throw std::runtime_error(who + ": rtol must lie between 0 and 1 (both excluded)");
  if (max_iter < 1) throw std::runtime_error(who + ": max_iter must be at least 1");
}
inline double iter_held_bytes(long N, int rank) {
  const double n = (double)N, p = (double)rank, segs = std::ceil(n / ITER_PLAN_SEG), dots = std::ceil(n / ITER_PLAN_DOT);
  return 8.0 * (n * p + 2.0 * p * p + ((double)ITER_PANELS * ITER_PLAN_COLS + 1.0) * n + ITER_PLAN_COLS * (segs * p + 2.0 * p + dots) + 2.0 * dots);
}
inline void iter_check_memory(const std::string& who, long N, int rank, double free_bytes, double already_held) {
  const double need = iter_held_bytes(N, rank);
  if (need > 0.5 * (free_bytes + already_held))
    throw std::runtime_error(who + ": " + std::to_string((long long)need) + " bytes of device memory for " + std::to_string(N) +
                             " points at preconditioner rank " + std::to_string(rank) + " are more than half of the free device memory");
}
// The exact likelihood (engine_iter_lik.hip) holds, beside iter_held_bytes: one further panel (the first preconditioned residuals), the
// coefficient log (2 ITER_PLAN_COLS max_iter), the normals g1 (rank x ITER_PLAN_COLS) and the partial sums and results of the sweep
// ((ceil(N / 64) + ITER_PLAN_COLS) 2 D).  1 <= T <= ITER_PLAN_COLS - 1 probes: one panel with the data column.
inline double iter_lik_bytes(long N, int D, int rank, int max_iter) {
  const double n = (double)N;
  return 8.0 * (ITER_PLAN_COLS * n + 2.0 * ITER_PLAN_COLS * (double)max_iter + (double)ITER_PLAN_COLS * std::max(rank, 1) +
                (std::ceil(n / 64.0) + ITER_PLAN_COLS) * 2.0 * D);
}
inline void iter_lik_check_probes(const std::string& who, int T) {
  if (T < 1 || T > ITER_PLAN_COLS - 1) throw std::runtime_error(who + ": n_probes must be between 1 and " + std::to_string(ITER_PLAN_COLS - 1));
}
inline void iter_lik_check_memory(const std::string& who, long N, int D, int rank, int max_iter, double free_bytes, double already_held) {
  const double need = iter_lik_bytes(N, D, rank, max_iter);
  if (need > 0.5 * (free_bytes + already_held))
    throw std::runtime_error(who + ": " + std::to_string((long long)need) + " bytes of device memory for the probe panel and the coefficient log of " +
                             std::to_string(N) + " points and " + std::to_string(max_iter) + " iterations are more than half of the free device memory");
}
struct IterPlan {
  long points;      // queries per pass
  long blocks;      // solves of ITER_PLAN_COLS cross columns per pass (with the variance)
};
inline double iter_point_bytes(int D) { return 8.0 * (2.0 * D + 16.0); }
inline IterPlan iter_plan(const std::string& who, long m, int D, double free_bytes, int max_points) {
  if (max_points < 0) throw std::runtime_error(who + ": max_points must not be negative");
  const double budget = 0.5 * free_bytes, per = iter_point_bytes(D);
  const long want = std::max<long>(1, std::min<long>(m, LOCAL_MAX_PASS));
  long points;
  if (max_points > 0) {
    points = std::min<long>(want, max_points);
    if ((double)points * per > budget)
      throw std::runtime_error(who + ": " + std::to_string(points) + " queries per pass need more than half of the free device memory; use a smaller max_points");
  } else {
    if (budget < per) throw std::runtime_error(who + ": one query does not fit half of the free device memory");
    points = std::min<long>(want, (long)std::floor(budget / per));
  }
  return {points, (points + ITER_PLAN_COLS - 1) / ITER_PLAN_COLS};
}
// The variance bound (engine_iter.hip variance_bound) holds, beside iter_held_bytes, the cache R (N rows, the rank rounded up to whole
// panels of ITER_PLAN_COLS columns) and one triangular factor of that padded order.  Its query passes are those of iter_plan: the 16 doubles
// per query that iter_point_bytes counts hold the partial sums of the at most ITER_MAX_RANK / ITER_VAR_CHUNK = 16 column chunks.
//   iter_var_check_precond   the bound is built from the preconditioner's factor: rank 0 is refused
//   iter_var_check_memory    refuses, before anything is allocated, what does not fit half of the free device memory with the solver's buffers
//   iter_var_check_rank      the rank asked for: 0 (all the cache has) or 1 .. the rank the preconditioner reached
constexpr int ITER_VAR_CHUNK = 64;      // columns of R per workgroup of the variance kernel (four MFMA blocks of 16)
static_assert(ITER_MAX_RANK / ITER_VAR_CHUNK <= 16, "the partial sums of a query live in the 16 doubles of iter_point_bytes");
inline long iter_var_pad(int rank) { return (long)ITER_PLAN_COLS * ((rank + ITER_PLAN_COLS - 1) / ITER_PLAN_COLS); }
inline double iter_var_bytes(long N, int rank) {
  const double pad = (double)iter_var_pad(rank);
  return 8.0 * ((double)N * pad + pad * pad);
}
inline void iter_var_check_precond(const std::string& who, int rank) {
  if (rank == 0) throw std::runtime_error(who + ": the variance bound is built from the preconditioner's factor: precond_rank must be at least 1");
}
inline void iter_var_check_memory(const std::string& who, long N, int rank, double free_bytes, double already_held) {
  const double need = iter_held_bytes(N, rank) + iter_var_bytes(N, rank);
  if (need > 0.5 * (free_bytes + already_held))
    throw std::runtime_error(who + ": " + std::to_string((long long)need) + " bytes of device memory for the solver and the variance cache of " +
                             std::to_string(N) + " points at rank " + std::to_string(rank) + " are more than half of the free device memory");
}
inline void iter_var_check_rank(const std::string& who, int request, int reached) {
  if (request < 0 || request > reached)
    throw std::runtime_error(who + ": rank must be between 1 and the rank the preconditioner reached, " + std::to_string(reached));
}

// Pathwise posterior draws (engine_rff.hip): the feature product amp Phi W and the solves of the paths' updates.
//   rff_check_counts   1 <= n_features <= RFF_MAX_FEATURES, n_draws >= 1, first_draw >= 0 and first_draw + n_draws within 2^31 - 1 (the
//                      generator's draw index)
//   rff_fixed_bytes    held whatever the points: the frequencies (F D), the phases (F) and one panel of ITER_PLAN_COLS columns of W (F each)
//   rff_point_bytes    per point of a pass: raw and scaled coordinates and the ITER_PLAN_COLS output columns
//   rff_plan           points per pass: max_points where given, else what the rest of half of the free memory holds, at most m and
//                      LOCAL_MAX_PASS, at least one; passes = blocks of ITER_PLAN_COLS draws.  No bit of a result depends on either.
constexpr int RFF_MAX_FEATURES = 65536;
inline void rff_check_counts(const std::string& who, long n_features, long n_draws, long first_draw) {
  if (n_features < 1 || n_features > RFF_MAX_FEATURES)
    throw std::runtime_error(who + ": n_features must be between 1 and " + std::to_string(RFF_MAX_FEATURES));
  if (n_draws < 1) throw std::runtime_error(who + ": n_draws must be at least 1");
  if (first_draw < 0) throw std::runtime_error(who + ": first_draw must not be negative");
  if (first_draw + n_draws > 2147483647L) throw std::runtime_error(who + ": first_draw + n_draws must stay below 2^31");
}
inline double rff_fixed_bytes(int D, int F) { return 8.0 * (double)F * ((double)D + 1.0 + ITER_PLAN_COLS); }
inline double rff_point_bytes(int D) { return 8.0 * (2.0 * D + ITER_PLAN_COLS); }
struct RffPlan {
  long points;      // points per pass
  long passes;      // blocks of ITER_PLAN_COLS draws
};
inline RffPlan rff_plan(const std::string& who, long m, int D, int F, long S, double free_bytes, int max_points) {
  if (max_points < 0) throw std::runtime_error(who + ": max_points must not be negative");
  rff_check_counts(who, F, S, 0);
  const double fixed = rff_fixed_bytes(D, F), budget = 0.5 * free_bytes - fixed, per = rff_point_bytes(D);
  if (budget < per)
    throw std::runtime_error(who + ": " + std::to_string((long long)(fixed + per)) + " bytes of device memory for " + std::to_string(F) +
                             " features and one point are more than half of the free device memory");
  const long want = std::max<long>(1, std::min<long>(m, LOCAL_MAX_PASS));
  long points;
  if (max_points > 0) {
    points = std::min<long>(want, max_points);
    if ((double)points * per > budget)
      throw std::runtime_error(who + ": " + std::to_string(points) + " points per pass need more than half of the free device memory; use a smaller max_points");
  } else {
    points = std::min<long>(want, (long)std::floor(budget / per));
  }
  return {points, (S + ITER_PLAN_COLS - 1) / ITER_PLAN_COLS};
}

// Input derivatives at large designs (engine_iter.hip kmatvec_inputderiv, engine_rff.hip rff_inputderiv): d/dx_d of the rectangular product and
// of the feature product, (points, D, columns) outputs.
//   INDERIV_DG              dimensions per workgroup of the two kernels: INDERIV_DG x 2 accumulator fragments of 4 doubles per lane
//   inderiv_point_bytes     per point of a pass: raw and scaled coordinates and the D x ITER_PLAN_COLS output columns
//   kinderiv_fixed_bytes    held whatever the points: one panel of ITER_PLAN_COLS columns of V (N each); the feature product holds rff_fixed_bytes
//   kinderiv_plan / rff_inderiv_plan   points per pass: max_points where given, else what the rest of half of the free memory holds, at most m and
//                           LOCAL_MAX_PASS, at least one; blocks = blocks of ITER_PLAN_COLS columns; groups = ceil(D / INDERIV_DG), the second
//                           grid dimension.  No bit of a result depends on any of them.
constexpr int INDERIV_DG = 8;
struct InderivPlan {
  long points;      // points per pass
  long blocks;      // blocks of ITER_PLAN_COLS columns
  int groups;       // groups of INDERIV_DG dimensions
};
inline double inderiv_point_bytes(int D) { return 8.0 * (double)D * (2.0 + ITER_PLAN_COLS); }
inline double kinderiv_fixed_bytes(long N) { return 8.0 * ITER_PLAN_COLS * (double)N; }
inline InderivPlan inderiv_plan_of(const std::string& who, long m, int D, long cols, double fixed, const std::string& held, double free_bytes,
                                   int max_points) {
  if (max_points < 0) throw std::runtime_error(who + ": max_points must not be negative");
  const double budget = 0.5 * free_bytes - fixed, per = inderiv_point_bytes(D);
  if (budget < per)
    throw std::runtime_error(who + ": " + std::to_string((long long)(fixed + per)) + " bytes of device memory for " + held +
                             " and one point are more than half of the free device memory");
  const long want = std::max<long>(1, std::min<long>(m, LOCAL_MAX_PASS));
  long points;
  if (max_points > 0) {
    points = std::min<long>(want, max_points);
    if ((double)points * per > budget)
      throw std::runtime_error(who + ": " + std::to_string(points) + " points per pass need more than half of the free device memory; use a smaller max_points");
  } else {
    points = std::min<long>(want, (long)std::floor(budget / per));
  }
  return {points, (cols + ITER_PLAN_COLS - 1) / ITER_PLAN_COLS, (D + INDERIV_DG - 1) / INDERIV_DG};
}
inline InderivPlan kinderiv_plan(const std::string& who, long m, int D, long N, long r, double free_bytes, int max_points) {
  if (r < 1) throw std::runtime_error(who + ": at least one column is needed");
  return inderiv_plan_of(who, m, D, r, kinderiv_fixed_bytes(N), "a panel of " + std::to_string(N) + " rows", free_bytes, max_points);
}
inline InderivPlan rff_inderiv_plan(const std::string& who, long m, int D, int F, long S, double free_bytes, int max_points) {
  rff_check_counts(who, F, S, 0);
  return inderiv_plan_of(who, m, D, S, rff_fixed_bytes(D, F), std::to_string(F) + " features", free_bytes, max_points);
}

// Stage 2 of predict_mixture: the normalised weights of the S samples of one emulator, from their negative log-posteriors F and
// ok flags and EITHER explicit weights w_in OR the log proposal density log_q (up to a constant).  With log_q:
//   l_s = -(F_s - F_min) - (log_q_s - log_q_a),  a = the first ok sample with F_a = F_min over the ok samples,  w_s = exp(l_s - max l)
// (the shift by max l changes nothing but the range of exp).  Samples that are not ok get weight 0; the rest is divided by its sum.
// Returns false -- and fills w_out with NaN -- when no sample is ok or the sum is not a positive finite number.
// mogp_emulator_amd/Marginal.py mixture_weights is the same formula in NumPy.
inline bool mixture_weights(int S, const double* F, const int* ok, const double* w_in, const double* log_q, double* w_out) {
  int a = -1;
  for (int s = 0; s < S; ++s)
    if (ok[s] && (a < 0 || F[s] < F[a])) a = s;
  double sum = 0.;
  if (a >= 0) {
    if (log_q) {
      double lmax = -INFINITY;
      for (int s = 0; s < S; ++s) {
        w_out[s] = ok[s] ? -(F[s] - F[a]) - (log_q[s] - log_q[a]) : -INFINITY;
        if (ok[s] && w_out[s] > lmax) lmax = w_out[s];
      }
      for (int s = 0; s < S; ++s) w_out[s] = ok[s] ? std::exp(w_out[s] - lmax) : 0.;
    } else {
      for (int s = 0; s < S; ++s) w_out[s] = ok[s] ? w_in[s] : 0.;
    }
    for (int s = 0; s < S; ++s) sum += w_out[s];
  }
  if (!(sum > 0.) || !std::isfinite(sum)) {
    for (int s = 0; s < S; ++s) w_out[s] = std::nan("");
    return false;
  }
  for (int s = 0; s < S; ++s) w_out[s] /= sum;
  return true;
}

// The tables of the pass of predict_mixture that holds the pairs [p0, p0 + cnt) (ok, w, nug: per pair; alive, pivot_pair: per
// emulator, pivot_pair = the first pair of the emulator that factorised or -1):
//   okslots  the slots whose sample factorised, ascending -- what is predicted, row r of the prediction = slot okslots[r];
//   rows     (cnt) the prediction row of a slot, -1 where its sample failed;
//   prm      (cnt, 2) weight and -- with include_nugget -- nugget of the slot's sample (0, 0 where it failed);
//   etab     (., 4) per alive emulator with a row in the pass [emulator, first slot, slots, row of its pivot or -1 where the pivot pair lies
//            in another pass].
// An empty okslots or etab: nothing to accumulate, the pass is skipped.
struct MixturePassTables {
  std::vector<int> okslots, rows, etab;
  std::vector<double> prm;
};
inline MixturePassTables mixture_pass_tables(long p0, long cnt, long S, const int* ok, const double* w, const double* nug, bool include_nugget,
                                             const int* alive, const int* pivot_pair) {
  MixturePassTables t;
  t.rows.assign(cnt, -1);
  t.prm.assign(2 * (std::size_t)cnt, 0.);
  for (long k = 0; k < cnt; ++k) {
    if (!ok[p0 + k]) continue;
    t.rows[k] = (int)t.okslots.size();
    t.okslots.push_back((int)k);
    t.prm[2 * k] = w[p0 + k];
    t.prm[2 * k + 1] = include_nugget ? nug[p0 + k] : 0.;
  }
  if (t.okslots.empty()) return t;
  for (long e = p0 / S; e <= (p0 + cnt - 1) / S; ++e) {
    const long first = std::max(e * S, p0) - p0, last = std::min((e + 1) * S, p0 + cnt) - p0;
    bool any = false;
    for (long k = first; k < last; ++k) any = any || t.rows[k] >= 0;
    if (!any || !alive[e]) continue;
    const long pp = pivot_pair[e] - p0;
    t.etab.insert(t.etab.end(), {(int)e, (int)first, (int)(last - first), (pp >= 0 && pp < cnt) ? t.rows[pp] : -1});
  }
  return t;
}

// Offsets (in doubles) into the staging block of the mean-function terms of a prediction of nb emulators at m points:
//   basis (nbasis x m) | dbasis (nterm x m) | coef (nb x nbasis) | LA (nb x qq x qq) | dims, powers (2 nterm ints, in nterm + 1 doubles)
// nterm = terms of a polynomial mean (0 otherwise), nbasis = 1 + nterm, qq = columns of the analytic mean (0 without).  The first two are
// filled on the device, the rest is staged from the host in one copy.
struct MeanStage {
  std::size_t o_basis, o_dbasis, o_coef, o_la, o_int, total;
  MeanStage(int nb, int m, int nbasis, int nterm, int qq)
      : o_basis(0), o_dbasis(o_basis + (std::size_t)nbasis * m), o_coef(o_dbasis + (std::size_t)nterm * m),
        o_la(o_coef + (std::size_t)nb * nbasis), o_int(o_la + (std::size_t)nb * qq * qq), total(o_int + (std::size_t)nterm + 1) {}
};

}  // namespace mogp
