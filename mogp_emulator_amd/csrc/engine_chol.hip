// Engine: the Cholesky factorisation of K + nugget I -- the schedule choice, the four blocked schedules and the pivoted one
#include "engine_internal.h"

#include "chol_schedule.h"

#include <algorithm>
#include <cstdlib>
#include <string>

namespace mogp {

// Blocked right-looking Cholesky of K + nugget I for the emulators in `ids` (one batched sequence).
// Recursive panel: a block column of width w is factored as [left half] -> update of the right half
// (K = w/2, MFMA) -> [right half], down to 64-wide leaves (potf2 + trsm).  The outer block is 512
// wide so the big trailing update runs with K = 512: per 128x128 tile the MFMA work then clearly outweighs the
// read-modify-write of C (256 KB per tile), which it does not at K = 128 (measured on C5: 256 -> 45.7 ms, 512 -> 41.7 ms).
// One 128-wide block column [c, c+128), rows [c, NP), K = [k0, k1).  With few 128 x 128 tiles in the launch (a single
// large matrix: (NP - c)/128 <= 125 workgroups on 256 CUs) the 64 x 64 tiling gives 4x the workgroups and the launch
// takes one short tile instead of one long one.
static void update_column_block(const BatchView& v, int c, int k0, int k1, hipStream_t st) {
  if ((long)v.nb * ((v.NP - c) / TILE) < 512L) launch_update_narrow_pair(v, c, k0, k1, st);
  else launch_update_wide(v, c, k0, k1, st);
}

void Engine::panel(const BatchView& v, int o, int w, hipStream_t st) {
  if (w == TILE) {
    launch_panel128(v, o, dInfo, dLpack, st);      // 128 x 128 diagonal block + 128-wide panel solve
    return;
  }
  int h = TILE;                      // largest power of two below w (w is a multiple of 128)
  while (2 * h < w) h *= 2;
  panel(v, o, h, st);
  for (int c = o + h; c < o + w; c += TILE) update_column_block(v, c, o, o + h, st);
  panel(v, o + h, w - h, st);
}

void Engine::ensure_pivot_buffers() {
  if (dXp) return;
  dPerm.reserve((size_t)B * n);
  dRank.reserve(B);
  dPivWork.reserve((size_t)B * pstrf_work_doubles(NP));
  hPerm.resize((size_t)B * n);
  for (int i = 0; i < B; ++i)
    for (int k = 0; k < n; ++k) hPerm[(size_t)i * n + k] = k;
  DevBuf<double> xp((size_t)B * n * D);
  for (int i = 0; i < B; ++i)
    HIPCK(hipMemcpyAsync(xp + (size_t)i * n * D, dX, (size_t)n * D * sizeof(double), hipMemcpyDeviceToDevice, stream));
  HIPCK(hipStreamSynchronize(stream));
  dXp = std::move(xp);
}

// nugget="pivot" (cholesky_factor(K, nugget, "pivot"), linalg/cholesky.py:182-184): K without nugget, factored with
// diagonal pivoting; afterwards the emulator's inputs are held in pivot order, so that every later kernel (prediction,
// gradient, L^-1, K^-1) works on an ordinary lower-triangular factor of k(Xp, Xp) and never sees the permutation.
void Engine::factorize_pivot(const std::vector<int>& ids, std::vector<int>& info) {
  const int nb = (int)ids.size();
  ensure_pivot_buffers();
  for (int i : ids) gp[i].nugget_used = 0.;
  upload_idx(ids);
  upload_params(ids);
  BatchView v = view(nb);
  v.X = dX;          // the covariance is built in training order; the interchanges happen inside the factorisation
  v.XS = 0;
  build_cov(v);
  launch_pstrf_begin(v, dPerm, dRank, dInfo, dPivWork, stream);
  std::vector<int> rank(B, 0), inf(B, 0);
  std::vector<int> active(ids), stopped;
  for (int k0 = 0; k0 < n && !active.empty(); k0 += NBI) {
    const bool first_half = (k0 % TILE) == 0;
    launch_pstrf_panel(v, k0, std::min(NBI, n - k0), dPerm, dRank, dPivWork, stream);
    HIPCK(hipMemcpyAsync(rank.data(), dRank, B * sizeof(int), hipMemcpyDeviceToHost, stream));
    HIPCK(hipStreamSynchronize(stream));
    std::vector<int> still;
    for (int i : active) {
      if (rank[i] < 0) still.push_back(i);
      else if (rank[i] < n) stopped.push_back(i);
    }
    if (still.size() != active.size()) {
      active.swap(still);
      if (active.empty()) break;
      upload_idx(active);
      v = view((int)active.size());
      v.X = dX;
      v.XS = 0;
    }
    // rank-64 update of everything to the right of the panel (the 128-wide tiles start at multiples of 128)
    if (first_half) launch_update_narrow(v, k0 + NBI, k0, k0 + NBI, stream);
    launch_update_trailing(v, first_half ? k0 + TILE : k0 + NBI, k0, k0 + NBI, stream);
  }
  if (!stopped.empty()) {
    upload_idx(stopped);
    BatchView t = view((int)stopped.size());
    launch_pstrf_tail(t, dPerm, dRank, stream);
  }
  upload_idx(ids);
  v = view(nb);
  launch_pstrf_end(v, stream);
  launch_permute_rows(v, dX, dPerm, dXp, stream);
  HIPCK(hipMemcpyAsync(inf.data(), dInfo, B * sizeof(int), hipMemcpyDeviceToHost, stream));
  HIPCK(hipMemcpyAsync(rank.data(), dRank, B * sizeof(int), hipMemcpyDeviceToHost, stream));
  HIPCK(hipMemcpyAsync(hPerm.data(), dPerm, hPerm.size() * sizeof(int), hipMemcpyDeviceToHost, stream));
  HIPCK(hipStreamSynchronize(stream));
  HIPCK(hipGetLastError());
  if (info.size() != (size_t)B) info.assign(B, 0);
  for (int i : ids) {
    info[i] = inf[i];
    gp[i].rank = rank[i];
    gp[i].permuted = true;
  }
}

// (asynchronous on `stream`: every later kernel that reads the inputs runs behind it on that stream or on one that waits for it)
void Engine::restore_order(int i) {
  HIPCK(hipMemcpyAsync(dXp + (size_t)i * n * D, dX, (size_t)n * D * sizeof(double), hipMemcpyDeviceToDevice, stream));
  for (int k = 0; k < n; ++k) hPerm[(size_t)i * n + k] = k;
  gp[i].permuted = false;
  gp[i].rank = 0;
}

void Engine::factorize(const std::vector<int>& ids, std::vector<int>& info, bool defer_info) {
  std::vector<int> piv, rest;
  for (int i : ids) (gp[i].nug_type == NUG_PIVOT ? piv : rest).push_back(i);
  if (piv.empty()) {
    // an emulator that was pivoted earlier goes back to training order
    for (int i : rest)
      if (gp[i].permuted) restore_order(i);
    factorize_blocked(rest, info, defer_info);
    return;
  }
  std::vector<int> tmp;
  if (!rest.empty()) {
    factorize(rest, tmp);
    info = tmp;
  } else {
    info.assign(B, 0);
  }
  factorize_pivot(piv, info);
}

void Engine::read_info(std::vector<int>& info, bool defer_info) {
  if (defer_info) return;
  info.assign(B, 0);
  HIPCK(hipMemcpyAsync(info.data(), dInfo, B * sizeof(int), hipMemcpyDeviceToHost, stream));
  HIPCK(hipStreamSynchronize(stream));
  HIPCK(hipGetLastError());
}

void Engine::factorize_blocked(const std::vector<int>& ids, std::vector<int>& info, bool defer_info, const CovFill* fill) {
  const int nb = (int)ids.size();
  upload_idx(ids);
  upload_params(ids);
  const BatchView v = view(nb);
  static const int forced = [] {
    const char* e = getenv("MOGP_CHOL");
    if (!e) return -1;
    if (e[0] == 'r') return (int)CHOL_RIGHT_LOOKING;
    if (std::string(e) == "mchol") return (int)CHOL_ONE_LAUNCH;
    if (std::string(e) == "multi") return (int)CHOL_MULTI;
    return (std::string(e) == "left") ? (int)CHOL_TWO_GROUPS : (int)CHOL_LOOKAHEAD;
  }();
  const int schedule = choose_cholesky_schedule(nb, NP, MS * sizeof(double), schedule_override().schedule, forced, mc_force_legacy);
  mc_used = schedule == CHOL_ONE_LAUNCH;
  if (mc_used) return chol_one_launch(ids, v, info, defer_info, fill);
  if (schedule == CHOL_LOOKAHEAD) chol_lookahead(v, fill);
  else if (schedule == CHOL_TWO_GROUPS) chol_two_groups(v, fill);
  else chol_right_looking(v, fill);
  read_info(info, defer_info);
}

void Engine::refactor_after_abort(const std::vector<int>& ids, std::vector<int>& info, bool defer_info, const CovFill* fill) {
  g_mc_aborts += 1;
  FlagGuard legacy_only(mc_force_legacy);          // reset also when the repeat throws
  factorize_blocked(ids, info, defer_info, fill);
}

void Engine::begin_multi_launch(const BatchView& v, const CovFill* fill) {
  HIPCK(hipMemsetAsync(dInfo, 0, B * sizeof(int), stream));
  build_cov(v, ZeroRanges(), fill);
}

void Engine::grow_step_events(int K) {
  while ((int)evUpd.size() < K + 1) {
    evPanel.push_back(make_event(hipEventDisableTiming));
    evUpd.push_back(make_event(hipEventDisableTiming));
  }
}

// ONE LAUNCH: persistent workgroups take the tasks of all block columns from a dependency-ordered queue (kernels_mchol.hip)
void Engine::chol_one_launch(const std::vector<int>& ids, const BatchView& v, std::vector<int>& info, bool defer_info, const CovFill* fill) {
  const int nb = v.nb;
  if (!dMcTable) {
    std::vector<int> tb = mchol_task_table(NP);
    const std::vector<int> ta = mchol_task_table(NP, true);
    mc_ntasks = (int)tb.size();
    tb.insert(tb.end(), ta.begin(), ta.end());              // [in-order | band-ahead]: launch_mchol picks
    dMcTable.reserve(tb.size());
    HIPCK(hipMemcpy(dMcTable, tb.data(), tb.size() * sizeof(int), hipMemcpyHostToDevice));
  }
  if (nb > mc_slots) {
    // control rows and packs are per batch SLOT of a launch, sized for the largest launch seen so far -- not for the engine's B: a
    // few-emulator retry on an engine whose full batch stays on the multi-launch schedules (B * NP / 128 >= 16384) would otherwise
    // allocate B packs per block column (4.7 GB at B = 2000, n = 2000)
    HIPCK(hipStreamSynchronize(stream));
    mc_slots = 0;                    // (both go before either comes back; a failed allocation leaves "sized for nothing")
    dMcCtrl.reset();
    dMcPacks.reset();
    dMcCtrl.reserve(mchol_ctrl_ints(NP, nb));
    dMcPacks.reserve(mchol_pack_doubles(NP, nb));
    mc_slots = nb;
  }
  // (the info words and the kernel's control words are cleared by the K build: two memset commands less in front of a small fit)
  ZeroRanges zr;
  zr.p[0] = reinterpret_cast<unsigned*>(dInfo.get()); zr.n[0] = (unsigned)B;
  zr.p[1] = dMcCtrl; zr.n[1] = (unsigned)mchol_ctrl_ints(NP, nb);
  build_cov(v, zr, fill);
  launch_mchol(v, dMcCtrl, mchol_ctrl_ints(NP, nb), dMcTable, mc_ntasks, dMcPacks, dInfo, n_cu, stream, true);
  if (defer_info) return;          // (the caller finds the abort word in the status words it reads: eval)
  read_info(info, false);
  unsigned aborted = 0;
  HIPCK(hipMemcpy(&aborted, dMcCtrl, sizeof(unsigned), hipMemcpyDeviceToHost));
  if (aborted) refactor_after_abort(ids, info, false, fill);
}

// LEFT-LOOKING WITH LOOK-AHEAD.  Block column c receives the panels 0 .. c-2 in one long-K MFMA pass U1(c) on the main
// stream -- every element of the trailing matrix is read-modified-written once, at the K depth where the MFMA main
// loop runs best -- WHILE the panel stream works on block column c-1:
//     panel stream (high priority):  U2(c): column c -= panel c-1 (K = 128)  ->  128 x 128 diagonal block  ->  panel solve
//     main stream:                   U1(c+2): column c+2 -= panels 0 .. c    (needs the panel solve of column c)
// The whole dependent chain of a block column (short update, diagonal block, panel solve) sits in ONE stream: a
// cross-stream event wait costs ~12 us on this stack when the waiter is already blocked (kernel trace), and the
// earlier schedules paid two of them per block column.  The main stream is one block column ahead, so its events
// have normally fired by the time the panel stream asks.  Replaces the two-emulator-group schedule (5.37 ms at
// 64 x n=2000), the right-looking schedule of small batches and of a single large matrix.
void Engine::chol_lookahead(const BatchView& v, const CovFill* fill) {
  const int nb = v.nb;
  const ScheduleOverride& ovr = schedule_override();
  std::vector<int> cols;
  for (int o = 0; o < n + R; o += TILE) cols.push_back(o);
  const int K = (int)cols.size();
  grow_step_events(K);
  constexpr long tail_threshold = 1100L;
  auto long_update = [&](int o, int k1, hipStream_t st) {
    // 64 x 64 tiles unless the launch has several rounds of 128 x 128 ones (measured 7.6 vs 8.3 ms at 64 x n=2000)
    if ((long)nb * ((NP - o) / TILE) >= tail_threshold) launch_update_wide(v, o, 0, k1, st);
    else launch_update_narrow_pair(v, o, 0, k1, st);
  };
  hipStream_t pst = ovr.single_stream ? stream : pstream;
  begin_multi_launch(v, fill);
  HIPCK(hipEventRecord(evReady, stream));
  HIPCK(hipStreamWaitEvent(pst, evReady, 0));
  // "U1(c) done" in front of U2(c) sits in the dependent chain although U1(c) has normally finished a block column earlier, and
  // an event wait costs the panel stream ~11 us even then.  As a stream memory operation on one signal word (the main stream
  // writes base + c behind U1(c), the panel stream waits for >= base + c) a satisfied wait is a memory poll: fit 1.62 -> 1.57 ms
  // at 8 x n=2000, 2.05 -> 1.94 at 16, 3.05 -> 2.94 at 32, 1.19 -> 1.14 at 64 x n=1000.  A waiter that really has to wait is
  // served later by the poll than by the event (n = 5000: 7.7 -> 8.0 ms at 4 emulators; the right-looking schedule, whose
  // waits are all of that kind: 5.2 -> 5.5 ms at 2 x n=5000, 34.3 -> 35.3 at n=16000; the other direction, panel -> U1, too),
  // so it is used up to NP = 3072.
  const bool wv = can_waitval && !ovr.single_stream && NP <= 3072;
  if (wv && !sigU1) {
    HIPCK(hipExtMallocWithFlags(reinterpret_cast<void**>(&sigU1), 8, hipMallocSignalMemory));
    HIPCK(hipMemset(sigU1, 0, 8));
  }
  if (wv && sig_epoch > 0xF0000000u) {      // the compare is >=: start over long before the counter wraps
    HIPCK(hipStreamSynchronize(stream));
    HIPCK(hipStreamSynchronize(pst));
    HIPCK(hipMemset(sigU1, 0, 8));
    sig_epoch = 1;
  }
  const uint32_t sig_base = sig_epoch;
  if (wv) sig_epoch += (uint32_t)K + 1;
  for (int c = 0; c < K; ++c) {
    const int o = cols[c];
    if (c >= 1) {
      if (c >= 2) {
        if (wv) HIPCK(hipStreamWaitValue32(pst, sigU1, sig_base + (uint32_t)c, hipStreamWaitValueGte, 0xFFFFFFFFu));
        else HIPCK(hipStreamWaitEvent(pst, evUpd[c], 0));                     // U1(c) done
      }
      launch_update_narrow_pair(v, o, o - TILE, o, pst);                      // U2(c): panel c-1 -> column c
    }
    panel(v, o, TILE, pst);
    HIPCK(hipEventRecord(evPanel[c], pst));
    if (c + 2 < K) {
      HIPCK(hipStreamWaitEvent(stream, evPanel[c], 0));
      long_update(cols[c + 2], cols[c + 1], stream);                          // U1(c+2): panels 0 .. c -> column c+2
      if (wv) HIPCK(hipStreamWriteValue32(stream, sigU1, sig_base + (uint32_t)(c + 2), 0));
      else HIPCK(hipEventRecord(evUpd[c + 2], stream));
    }
  }
  HIPCK(hipStreamWaitEvent(stream, evPanel[K - 1], 0));
}

// Two independent emulator groups on separate streams: while one group runs its
// latency-bound panel kernels (diagonal block / panel solve: few workgroups) the other group's MFMA update fills the
// machine.  More than two streams collapse (round 1, 64 x n=2000: 1 group 6.58 ms, 2 groups 6.23 ms, 3 groups 8.3 ms,
// 4 groups 14.2 ms -- the same when replayed from a captured hipGraph, so it is not host launch overhead).
void Engine::chol_two_groups(const BatchView& v, const CovFill* fill) {
  const int nb = v.nb;
  constexpr long tail_threshold = 1100L;
  const int G = schedule_override().single_stream ? 1 : std::min(2, std::max(1, nb / 8));
  while ((int)gstreams.size() < G - 1) {
    gstreams.push_back(make_stream(hipStreamNonBlocking));
  }
  begin_multi_launch(v, fill);
  HIPCK(hipEventRecord(evReady, stream));
  std::vector<BatchView> gv(G, v);
  std::vector<hipStream_t> gs(G, stream);
  for (int g = 0; g < G; ++g) {
    const int lo = (int)((long)nb * g / G), hi = (int)((long)nb * (g + 1) / G);
    gv[g].idx = dIdx + lo;
    gv[g].nb = hi - lo;
    if (g > 0) {
      gs[g] = gstreams[g - 1];
      HIPCK(hipStreamWaitEvent(gs[g], evReady, 0));
    }
  }
  for (int o = 0; o < n + R; o += TILE)
    for (int g = 0; g < G; ++g) {
      if (o > 0) {
        // with fewer than ~4 128-tiles per CU (always true at n=2000 x 64, measured 7.6 vs 8.3 ms) use
        // 64x64 tiles: 4x the workgroups, 3 resident per CU, better balance and latency hiding; both 64-wide
        // halves of the block column go in one launch (7.56 -> 6.84 ms: the partially filled last round of
        // workgroups is paid once instead of twice)
        const long tiles128 = (long)gv[g].nb * ((NP - o) / TILE);
        if (tiles128 >= tail_threshold) launch_update_wide(gv[g], o, 0, o, gs[g]);
        else launch_update_narrow_pair(gv[g], o, 0, o, gs[g]);
      }
      panel(gv[g], o, TILE, gs[g]);
    }
  for (int g = 1; g < G; ++g) {
    HIPCK(hipEventRecord(evGroup[g - 1], gs[g]));
    HIPCK(hipStreamWaitEvent(stream, evGroup[g - 1], 0));
  }
}

// Right-looking with look-ahead on two HIP streams: as soon as the columns of the NEXT outer block have
// received the update from panel k (U_a, main stream), panel k+1 is factored on the panel stream
// while the main stream applies panel k to the rest of the trailing matrix (U_b).  The
// latency-bound panel kernels (potf2 / trsm, few workgroups) thereby run underneath the MFMA
// trailing update instead of in front of it.
void Engine::chol_right_looking(const BatchView& v, const CovFill* fill) {
  begin_multi_launch(v, fill);
  std::vector<int> starts;
  // outer block = K depth of the trailing update (256 / 512 / 1024 -> C5 fit 45.7 / 41.7 / 44.3 ms, round 1)
  constexpr int OUTERW = 512;
  for (int o = 0; o < n + R; o += OUTERW) starts.push_back(o);
  const int K = (int)starts.size();
  grow_step_events(K);
  auto width = [&](int k) { return std::min(OUTERW, NP - starts[k]); };
  HIPCK(hipEventRecord(evUpd[K], stream));                 // K build done
  HIPCK(hipStreamWaitEvent(pstream, evUpd[K], 0));
  panel(v, starts[0], width(0), pstream);
  HIPCK(hipEventRecord(evPanel[0], pstream));
  for (int k = 0; k < K; ++k) {
    const int o = starts[k], w = width(k);
    HIPCK(hipStreamWaitEvent(stream, evPanel[k], 0));
    if (k + 1 < K) {
      const int on = starts[k + 1], wn = width(k + 1);
      for (int c = on; c < on + wn; c += TILE) update_column_block(v, c, o, o + w, stream);     // U_a
      HIPCK(hipEventRecord(evUpd[k], stream));
      HIPCK(hipStreamWaitEvent(pstream, evUpd[k], 0));
      panel(v, on, wn, pstream);
      HIPCK(hipEventRecord(evPanel[k + 1], pstream));
      launch_update_trailing(v, on + wn, o, o + w, stream);                                     // U_b
    } else {
      launch_update_trailing(v, o + w, o, o + w, stream);   // (empty unless padding rows remain)
    }
  }
}

}  // namespace mogp
