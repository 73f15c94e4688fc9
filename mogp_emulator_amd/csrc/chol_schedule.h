// Which Cholesky schedule a batch of nb matrices of padded size NP takes (Engine::factorize_blocked, engine_chol.hip).  Plain host
// arithmetic with no HIP in it, so that a host compiler takes it and tests/c/chol_schedule_check.cpp can check it without a device.
#pragma once
#include <cstddef>

namespace mogp {

// one launch / task queue (default, kernels_mchol.hip); the multi-launch schedules (fall-back, >= 16384 tiles per step): left-looking with
// look-ahead, left-looking in two emulator groups, right-looking + look-ahead; CHOL_MULTI = the multi-launch schedule of the regime.
// MOGP_CHOL forces one: mchol (4), la (3), left (0), right (1), multi (5)
enum CholSchedule { CHOL_TWO_GROUPS = 0, CHOL_RIGHT_LOOKING = 1, CHOL_LOOKAHEAD = 3, CHOL_ONE_LAUNCH = 4, CHOL_MULTI = 5 };

// hook: ScheduleOverride::schedule (mogp_profile_schedule), forced: the parsed MOGP_CHOL; -1 = not set.  force_legacy: the repeat after an
// aborted one-launch factorisation.  Never returns CHOL_MULTI.
inline int choose_cholesky_schedule(int nb, int NP, std::size_t matrix_bytes, int hook, int forced, bool force_legacy) {
  // Measured (fit, ms; look-ahead / two groups / right-looking): 8 x n=2000 1.75 / 1.97 / 1.89, 16 x 2.21 / 2.38 / 2.44,
  // 32 x 3.32 / 3.34 / 3.65, 64 x 5.47 / 5.37 / 6.76, 16 x n=5000 18.9 / 19.8 / -, 2 x n=5000 6.59 / - / 6.42,
  // 1 x n=16000 59.8 / - / 38.4: one matrix has too few tiles per block column for a left-looking pass (right-looking),
  // a large batch fills the machine with the update of ONE emulator group while the other factors its panels.
  const long tiles64 = (long)nb * (NP / 64), tiles128 = (long)nb * (NP / 128);
  // Default: the ONE-LAUNCH task-queue kernel (schedule 4) below 16384 128-tiles per block-column step.  Fit, ms, one launch /
  // best multi-launch schedule: 8 x n=2000 1.12 / 1.60, 16 x 1.54 / 1.98, 32 x 2.58 / 3.05, 64 x 4.73 - 4.84 / 5.06, 120 x 8.46 /
  // 8.83, 2 x n=5000 2.86 / 5.27, 16 x n=5000 14.4 / 17.5, n=16000 26.3 / 34.5, 3 x n=700 0.40 / 0.54, 64 x n=1000 1.04 / 1.06.
  // Beyond that and for more than 512 single-block matrices (2000 x n=100: 0.62 / 0.57, one task each) the two-group multi-launch
  // schedule stays.
  const int legacy = tiles64 < 256 ? CHOL_RIGHT_LOOKING : (tiles128 >= 1024 ? CHOL_TWO_GROUPS : CHOL_LOOKAHEAD);
  // Round 6: re-measured on the round-5 kernels, the one-launch kernel wins at every batch size -- 128 / 256 / 512 x n=2000: 7.71 / 15.24 /
  // 30.68 ms against 8.87 / 17.54 / 33.70 with the two-group schedule, 1024 x n=1000 11.19 / 11.73, 2048 x n=500 4.50 / 4.91, 4096 x n=250
  // 2.34 / 2.75, 64 x n=5000 52.2 / 56.9 (profiles/r06_big_batch.txt) -- so the bound is now the pack memory alone (147 KB per emulator and
  // block column: 16384 tiles = 2.4 GB); rounds 2-5 stopped at 2048 tiles (measured on the round-2 kernel: 240 x n=2000 17.3 / 16.8).
  const bool mc_regime = tiles128 < 16384 && (NP > 128 || nb <= 512);
  // precedence: the hook (mogp_profile_schedule), then MOGP_CHOL, then the regime
  int schedule = hook >= 0 ? hook : forced >= 0 ? forced : mc_regime ? CHOL_ONE_LAUNCH : legacy;
  if (schedule == CHOL_MULTI) schedule = legacy;
  // the one-launch kernel addresses an emulator's matrix through a 32-bit buffer offset; after an abort the multi-launch
  // schedule of the same regime takes over
  if (schedule == CHOL_ONE_LAUNCH && (force_legacy || matrix_bytes >= (std::size_t)1 << 32)) schedule = legacy;
  return schedule;
}

// Rows of the tile [row0, row0 + rows) that lie above the identity padding, in whole 16-row MFMA sub-tiles: n_real = n + R rows of an
// emulator's matrix carry data (K, then the right-hand-side rows), everything below is identity up to NP.  0, 16, .. rows.  The ONE rule
// of the factorisation's row tiles (kernels_mchol.hip), the triangular inverse (kernels_gemm.hip, kernels_chol.hip) and
// tests/c/real_rows_check.cpp: a skipped sub-tile holds no data row, so its products are exact zeros.
constexpr int real_rows(int n_real, int row0, int rows) {
  const int left = n_real - row0;
  if (left <= 0) return 0;
  const int up = (left + 15) / 16 * 16;
  return up < rows ? up : rows;
}

}  // namespace mogp
