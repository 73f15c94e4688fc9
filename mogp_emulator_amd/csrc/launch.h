// Host-side launchers for the gfx950 kernels.  All launches are asynchronous on `stream`.
//
// Data layout in HBM:
//   X      (n, D) row-major, shared by every emulator of an engine
//   P      per emulator parameter block of PS doubles: [e_0..e_{D-1} = exp(theta_d), sigma^2, nugget]
//   T      per emulator residual targets (n)
//   A      per emulator NP x NP "factor" matrix, row-major with row stride LD (= NP), NP = roundup(n+1, 128).
//          rows/cols < n : K + nugget I -> overwritten in place by L (lower triangle)
//          row n         : the targets t -> overwritten by y^T = (L^-1 t)^T   (free forward solve)
//          rows > n      : identity padding
//   Linv   per emulator NP x NP row-major, lower triangular L^-1
//   Kinv   per emulator NP x NP row-major, K^-1 (lower tiles valid); doubles as scratch for trtri
//   batch slot z -> emulator index: idx ? idx[z] : z
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <vector>

namespace mogp {

// Thread index for the device functions shared between the stand-alone kernels and the one-launch Cholesky.  In the
// latter (MOGP_OPAQUE_TID) the index is laundered through an empty asm statement: otherwise the compiler hoists every
// per-thread address computation of every task type out of the task loop and spills them (57 VGPRs).
#ifdef __HIPCC__
__device__ __forceinline__ int mogp_tid() {
  int t = threadIdx.x;
#ifdef MOGP_OPAQUE_TID
  asm volatile("" : "+v"(t));
  __builtin_assume(t >= 0 && t < 256);
#endif
  return t;
}
#endif

constexpr int TILE = 128;       // MFMA macro tile / padding granule
// The covariance kernels stage two 64-row blocks of X (and, for predict_deriv, a 64 x 65 work tile and a 64 x D
// accumulator) in LDS: (192 D + 4160) doubles <= 160 KB  ->  D <= 85.
constexpr int MAX_D = 80;
constexpr int NBI = 64;         // pivoted-Cholesky panel width / trtri leaf
constexpr double PAD_BIG = 1e300;
constexpr int RMAX = 8;         // max right-hand-side rows (targets + up to 7 mean-function columns)

struct BatchView {
  int n, D, NP, PS;             // PS = parameter block stride (doubles)
  int LD;                       // row stride of A / Linv / Kinv / Ks / alpha (= NP; padding measured slower)
  size_t MS;                    // per-emulator matrix stride = NP * LD
  int kernel_type;
  const double* X;              // n*D, or per emulator (XS = n*D) when the training inputs are held in pivoted order
  size_t XS = 0;                // per-emulator stride of X in doubles (0 = one matrix shared by all emulators)
  const double* P;              // B*PS
  const double* T;              // B*n
  double* A;                    // B*NP*NP
  double* Linv;                 // B*NP*NP (may be null)
  double* Kinv;                 // B*NP*NP (may be null)
  double* alpha;                // B*RA*LD.  R = 1: the single row K^-1 t.  R > 1 (analytic mean): row 0 = K^-1 (t - H beta_hat) (predictions),
                                // rows 1..q = rank-correction rows g_c, row R = K^-1 (t - H (b + beta')) (gradient; equals row 0 with weak mean priors)
  double* Z;                    // B*R*LD raw solves K^-1 [t, h_1 .. h_q]   (same buffer as alpha when R = 1)
  const double* H;              // q*n design-matrix columns of the analytic mean (shared by all emulators), or null
  int R;                        // 1 + q right-hand sides carried through the factorisation as rows n .. n+q of A
  int RA;                       // rows per emulator in alpha: 1 (R = 1) or R + 1
  const int* idx;               // device: nb entries or null
  int nb;                       // number of batch slots in this launch
};

// --- covariance build ---------------------------------------------------------------------
// zero: up to two int ranges the launch also clears (the factorisation's info words, the one-launch Cholesky's control words) -- each was a
// memset command of its own in front of the kernel that needs it, 9 - 10 us per command on the path of a small fit
struct ZeroRanges {
  unsigned* p[2] = {nullptr, nullptr};
  unsigned n[2] = {0, 0};
};
void launch_cov_build(const BatchView& v, hipStream_t s, const ZeroRanges& zero = ZeroRanges());
// full symmetric K (no nugget) for get_K: out (n,n) for one emulator
void launch_cov_full(const BatchView& v, int emu, double* out, hipStream_t s);
// stand-alone kernel objects (bindings.cu:340-361): device buffers x1 (n1, D), x2 (n2, D), P = [exp(theta_d) (D), sigma^2];
// mode 0 K (n1, n2), 1 dK/dtheta (D+1, n1, n2), 2 dK/dx1 (n2, n1, D); kt = device kernel 0 / 1 / 2
void launch_kernel_object(int kt, const double* x1, int n1, const double* x2, int n2, int D, const double* P, int mode, double* out, hipStream_t s);
// leave-one-out predictive variance 1/[K^-1]_ii of every training input (needs Linv): out[slot*out_ld + i]
void launch_loo_variance(const BatchView& v, double* out, int out_ld, hipStream_t s);
// history-matching score of m query points from device-resident means / variances (nb, ld); prm (nb, 3) =
// [observation, obsvar + discrepancy + nugget, mean offset]; out[j] = (rank+1)-th largest implausibility
constexpr int IMPLAUS_MAX_RANK = 15;
void launch_implausibility(int nb, const double* mean, const double* var, int ld, int m, const double* prm, int rank, double* out,
                           hipStream_t s);
// the same over the emulators of one part of a multi-part model: out[r * out_ld + j] = the (r+1)-th largest of its own, r < keep
// (-inf where it has fewer); merge: lists (nparts * (rank+1), ld) of every part -> out[j] = (rank+1)-th largest overall
void launch_implausibility_top(int nb, const double* mean, const double* var, int ld, int m, const double* prm, int keep, double* out,
                               long out_ld, hipStream_t s);
void launch_implausibility_merge(int nparts, const double* lists, long ld, int m, int rank, double* out, hipStream_t s);
// out (nb, m, m) = sigma^2 k(Xs, Xs) per slot (no nugget)
void launch_cov_self_batch(const BatchView& v, const double* Xs, int m, double* out, hipStream_t s);
// full predictive covariance: cov (nb, m, m) holds K** on entry, K** - Ks K^-1 Ks^T on return; V: nb*NP*MP scratch
void launch_predict_fullcov(const BatchView& v, const double* Ks, int m, int MP, double* V, double* cov, hipStream_t s);
// its first half alone: V (nb, NP, MP) = L^-1 Ks^T (rows < roundup(n, 128) written; columns >= m are zero as those rows of Ks are)
void launch_predict_v_store(const BatchView& v, const double* Ks, int m, int MP, double* V, hipStream_t s);

// --- blocked Cholesky ---------------------------------------------------------------------
size_t lpack128_doubles_per_emulator();   // scratch written by the diagonal-block kernel, read by the panel solve
// 128 x 128 diagonal block at c0 (one workgroup per emulator, chol128_dev.h) and the 128-wide panel below it (MFMA block
// substitution); info[emu] = 0, or c0 + 1 of the FIRST 128-wide diagonal block that met a pivot that is not a positive finite
// number (the column inside the block is not recorded: a bad pivot turns into NaN, which reaches the block's last
// reciprocal square root, tested once -- chol128_dev.h; the engine only tests for non-zero)
void launch_panel128(const BatchView& v, int c0, int* info, double* Lpack128, hipStream_t s);
// C[i,j] -= sum_{k in [k0,k1)} A[i,k] A[j,k] for the 64-wide column block [c0,c0+64), rows [c0, NP)
void launch_update_narrow(const BatchView& v, int c0, int k0, int k1, hipStream_t s);
// the two 64-wide halves of the 128-wide column block [c0, c0+128) in one launch of 64 x 64 tiles
void launch_update_narrow_pair(const BatchView& v, int c0, int k0, int k1, hipStream_t s);
// same for a 128-wide column block with 128 x 128 tiles
void launch_update_wide(const BatchView& v, int c0, int k0, int k1, hipStream_t s);
// trailing lower-triangular update, rows/cols [c0, NP), k in [k0,k1) (c0 multiple of 128)
void launch_update_trailing(const BatchView& v, int c0, int k0, int k1, hipStream_t s);
// --- the whole blocked Cholesky as ONE launch (kernels_mchol.hip): persistent workgroups work off a dependency-ordered task
// queue.  table: mchol_task_table(NP) on the device; ctrl: mchol_ctrl_ints(NP, B) unsigned ints (zeroed by the launcher; ctrl[0]
// != 0 afterwards = a wait timed out and the factors are unusable: factorise again with a multi-launch schedule); packs:
// mchol_pack_doubles(NP, B) doubles (one diagonal-block pack per emulator and block column); info as launch_panel128.
// The matrix of one emulator must be smaller than 4 GB (write-through stores go through a buffer descriptor).
std::vector<int> mchol_task_table(int NP, bool ahead = false);
size_t mchol_ctrl_ints(int NP, int B);
size_t mchol_pack_doubles(int NP, int B);
// ctrl_zeroed: the caller has cleared ctrl[0 .. ctrl_ints) on the stream already (launch_cov_build's ZeroRanges)
// tables: the in-order table, then the band-ahead one (mchol_task_table(NP, true)), ntasks entries each
void launch_mchol(const BatchView& v, unsigned* ctrl, size_t ctrl_ints, const int* tables, int ntasks, double* packs, int* info, int n_cu,
                  hipStream_t s, bool ctrl_zeroed = false);
constexpr int MCHOL_ABORTED = -3;     // status reported by launch_logdet for every emulator when ctrl[0] != 0

// res (indexed by emulator, RES_STRIDE doubles each): [0] = 2 sum_{i<n} log L_ii, [1] = info[emu] -- or BACKSOLVE_TIMEOUT when the
// factorisation succeeded but bs_status[emu] == bs_epoch (the one-launch back substitution gave up waiting) --,
// [2 + r*RMAX + s] = sum_{c<n} L[n+r,c] L[n+s,c]  (Gram matrix of the right-hand-side rows; [2] = y^T y)
constexpr int RES_STRIDE = 2 + RMAX * RMAX;
constexpr int BACKSOLVE_TIMEOUT = -2;
void launch_logdet(const BatchView& v, const int* info, double* res, hipStream_t s, const int* bs_status = nullptr, int bs_epoch = 0,
                   const unsigned* mc_abort = nullptr);
// alpha[c] = sum_r M[emu][c][r] Z[r], c < RA   (M: indexed by emulator, (RMAX+1) x RMAX row-major)
void launch_combine_rows(const BatchView& v, const double* M, hipStream_t s);
// alpha = L^-T y (y = row n of A)
void launch_backsolve(const BatchView& v, hipStream_t s);
// the same in one launch (R == 1), with alpha preset to all-ones bit patterns: status = B ints indexed by emulator, all != epoch on entry;
// status[emu] = epoch when a wait of that emulator's chain timed out (alpha is then unusable: repeat with launch_backsolve)
// info / res / mc_abort: as launch_logdet's -- the chain's leftmost chunk then writes res (log-determinant, Gram entry, status word) itself;
// returns whether it does (chain-bound launches): the caller launches launch_logdet otherwise.
bool launch_backsolve_chain(const BatchView& v, int epoch, int* status, int n_cu, hipStream_t s, const int* info = nullptr,
                            double* res = nullptr, const unsigned* mc_abort = nullptr);
// Pivoted Cholesky with LAPACK dpstrf semantics (nugget="pivot", linalg/cholesky.py:284-327), see kernels_pivot.hip.
// A (K without nugget, and the right-hand-side rows) is factored in place with symmetric row/column interchanges:
//   begin -> { panel(k0, 64 columns) -> rank-64 update of everything to its right } ... -> tail -> end
// (after every panel the host drops the emulators whose factorisation stopped)
// perm[emu*n + pos] = original index of the point now at position pos; rank[emu] = -1 while running, else the number of
// pivots accepted; info[emu] = 1 when no pivot is positive.  work: B * pstrf_work_doubles(NP) doubles, indexed by emulator.
__host__ __device__ inline size_t pstrf_work_doubles(int NP) { return 2 * (size_t)NP + 8; }
void launch_pstrf_begin(const BatchView& v, int* perm, int* rank, int* info, double* work, hipStream_t s);
void launch_pstrf_panel(const BatchView& v, int k0, int jb, int* perm, int* rank, double* work, hipStream_t s);   // jb <= 64
// emulators of the launch with 0 < rank < n: replacement diagonal, right-hand-side rows through the skipped block
void launch_pstrf_tail(const BatchView& v, const int* perm, const int* rank, hipStream_t s);
void launch_pstrf_end(const BatchView& v, hipStream_t s);
// Xp[emu] (n, D) <- X[perm[emu]] for the slots of the launch
void launch_permute_rows(const BatchView& v, const double* X, const int* perm, double* Xp, hipStream_t s);

// --- L^-1, K^-1 ----------------------------------------------------------------------------
void launch_trtri(const BatchView& v, hipStream_t s);        // A(L) -> Linv   (uses Kinv as scratch)
void launch_kinv(const BatchView& v, int n_cu, hipStream_t s);   // Linv -> Kinv (lower tiles); n_cu: compute units of the engine's device
void launch_alpha_from_linv(const BatchView& v, hipStream_t s);   // alpha = Linv^T y

// --- gradient ------------------------------------------------------------------------------
// partial: nb * ntiles * (D+3) doubles scratch; out: per emulator (D+3): [g_0..g_{D-1}, g_cov, tr(Kinv), alpha.alpha]
int grad_num_tiles(int n);
void launch_grad(const BatchView& v, double* partial, double* out, hipStream_t s);
// rank-deficient pivoted factor: out[emu][p] += 0.5 sum_k w_k^T dK_p w_k over the m rows W2 (m x LD) of L^-1 that K^-1 was
// formed without; part: m * ceil(n/128) * (D+1) doubles scratch
void launch_grad_lowrank(const BatchView& v, int emu, const double* W2, int m, double* part, double* out, hipStream_t s);

// --- predict -------------------------------------------------------------------------------
// Ks: nb * MP * NP (MP = roundup(m,128)) cross-covariance sigma^2 k(x*_m, x_j); mean (nb, m) written;
// if Ks == null only the mean is computed.  With R > 1 the kernel also returns Z_c^T k* (rows 1..R-1 of `mean`,
// row stride mean_ld per emulator block of R rows).
void launch_cross_cov_mean(const BatchView& v, const double* Xs, int m, int MP, double* Ks, double* mean, int mean_ld, hipStream_t s);
// var[z][m] = sigma^2 - sum_i (Linv Ks^T)[i][m]^2 ; partial: nb * (NP/128) * MP scratch
void launch_predict_var(const BatchView& v, const double* Ks, int m, int MP, double* partial, double* var, int var_ld, int n_cu, hipStream_t s);
// deriv[z][m][d]
void launch_predict_deriv(const BatchView& v, const double* Xs, int m, double* deriv, long deriv_stride, hipStream_t s);

// mean-function terms of a batched prediction on device buffers (kernels_chol.hip predict_mean_finish_kernel): basis (nbasis, m),
// coef (nb, nbasis), R > 1: dots (nb, R, m) and LA (nb, q, q); mean / var (nb rows of stride ld; either may be null); derivative terms
// dbasis (nterm, m), ddims / dpowers (nterm) into deriv (nb, m, D) or null
// basis (1 + nterm, m) / dbasis (nterm, m) of a polynomial mean at device-resident points Xs (m, D); dims / powers: device ints
void launch_mean_basis(const double* Xs, int m, int D, int nterm, const int* dims, const int* powers, double* basis, double* dbasis, hipStream_t s);
void launch_predict_mean_finish(int nb, int m, int D, int R, int nbasis, const double* basis, const double* coef, const double* dots,
                                const double* LA, double* mean, double* var, long ld, int nterm, const double* dbasis, const int* ddims,
                                const int* dpowers, double* deriv, hipStream_t s);

// --- sensitivity (kernels_sobol.hip) -----------------------------------------------------------
// Every reduction: wave shuffles, LDS, one partial per workgroup in a scratch slot, a final pass in a fixed order (no atomics).
constexpr int SOBOL_MAX_GROUPS = 256;   // workgroups of one row reduction
constexpr int SOBOL_STATS = 4;          // per emulator [f0, V, mean predictive variance, nugget added to the variances]
int sobol_groups(long m);               // workgroups a reduction over m elements is launched with (<= SOBOL_MAX_GROUPS)
// out (rows, D) = rows [r0, r0 + rows) of A (N, D) with column col taken from B
void launch_sobol_pick_freeze(const double* A, const double* B, long r0, int rows, int D, int col, double* out, hipStream_t s);
// out[k * ostride] = mean over j < m of  x[k][j] (mode 0),  (x[k][j] - prm[k * pstride])^2 (mode 1),  max(x[k][j] + prm[k * pstride], 0)
// (mode 2);  x (nb, ld); partial: nb * sobol_groups(m) doubles scratch
void launch_sobol_row_mean(int nb, int mode, const double* x, long ld, long m, const double* prm, int pstride, double* partial, double* out,
                           int ostride, hipStream_t s);
// one chunk of `rows` base rows of input col: fA, fB (nb, ld) and fAB (nb, ldab) point at the chunk's first row, f0 = stats[k * sstride];
// partial[((k * D + col) * nslot + slot0 + w) * 2 + {0, 1}] = sum (fB - f0)(fAB - fA), sum (fA - fAB)^2 of workgroup w < groups
void launch_sobol_pair_sum(int nb, const double* fA, const double* fB, long ld, const double* fAB, long ldab, int rows,
                           const double* stats, int sstride, double* partial, int D, int col, long nslot, long slot0, int groups,
                           hipStream_t s);
// out[q * 2 + {0, 1}] = scale * sum of the nslot partials of quantity q < nq, in a fixed order
void launch_sobol_pair_final(int nq, const double* partial, long nslot, double scale, double* out, hipStream_t s);

// --- Hessian of the log-posterior (kernels_hess.hip) ----------------------------------------------
// NPh = hess_np(n) = n rounded up to 64.  Per slot of the launch: Xs (NPh, D) scaled inputs; M (D, NPh, NPh) the planes Q^-1 Q_p;
// needs Kinv (lower triangle) and alpha.  Reductions as the sensitivity kernels': per-workgroup slots, a fixed-order final sum.
constexpr int HESS_MAX_GROUPS = 256;    // workgroups (= scratch slots) of one emulator's trace / pair reduction
int hess_np(int n);
int hess_trace_groups(int n);
int hess_pair_groups(int n);
void launch_hess_scale(const BatchView& v, double* Xs, hipStream_t s);
void launch_hess_planes(const BatchView& v, const double* Xs, double* M, hipStream_t s);
// out (nb, D + 1, D + 2): [p][q] = sum_ab P_p[a,b] P_q[b,a], planes P_p = M_p (p < D), P_D = Q^-1, P_{D+1} = I; valid for p < D, p <= q
// and for [D][D]; partial: nb * hess_trace_groups(n) * (D + 1) * (D + 2) doubles
void launch_hess_trace(const BatchView& v, const double* M, double* partial, double* out, hipStream_t s);
// out (nb, D, D): [p][q] = sum_ab W[a,b] sigma^2 k''(r2) s_p s_q, p <= q; partial: nb * hess_pair_groups(n) * D * D doubles
void launch_hess_pair(const BatchView& v, const double* Xs, double* partial, double* out, hipStream_t s);
// V, U (nb, D, NPh): v_p = M_p^T t, u_p = M_p alpha;  Zv (nb, NPh) = Q^-1 alpha
void launch_hess_vectors(const BatchView& v, const double* M, double* V, double* U, double* Zv, hipStream_t s);

// --- mixture prediction over hyperparameter samples (kernels_mixture.hip) -------------------------
// One pass of predict_mixture: mu / var (rows, ld) are the means and raw variances of the pass's slots that factorised, at the mc
// query points [c0, c0 + mc) of m.  The pass's slots are emulator-major, sample-ascending; emulator entry b < nemu of the pass is
//   etab[4 b ..] = { emulator e, its first slot, its number of slots, the row of its pivot sample or -1 (the pivot is of an earlier pass) }
// and slot k has rows[k] (its row of mu / var, -1: the sample failed and is skipped) and prm[2 k ..] = { weight, nugget to add }.
// acc (E, 3, m): the running sums  sum w d,  sum w max(var + nugget, 0),  sum w d^2  with d = mu - pivot mean; pivot (E, m): the pivot
// mean, written by the pass that holds the pivot sample.  One thread per (emulator, point), one add per sample and sum in slot order,
// plain multiplies and adds (contraction off), no atomics: the sums do not depend on how samples fall into passes or points into chunks.
void launch_mixture_accumulate(const double* mu, const double* var, long ld, int mc, int nemu, const int* etab, const int* rows,
                               const double* prm, double* acc, double* pivot, long m, long c0, hipStream_t s);
// in place, per emulator e < E and point: acc[e][0] <- pivot + sum w d (mean), acc[e][1] stays (within), acc[e][2] <- max(sum w d^2 -
// (sum w d)^2, 0) (between); all three NaN where alive[e] == 0
void launch_mixture_finalise(int E, long m, const int* alive, const double* pivot, double* acc, hipStream_t s);

// --- cross-validation at the fitted hyperparameters (kernels_cv.hip) -------------------------------
// Result rows are in the order of the launch's slots (caller rows): mean / var (rows, n), maha / log_score / ok (rows, k); targets (rows, n)
// are the observations t themselves (mean = t - e), eta (rows) the nugget taken off var again without include_nugget.
// Leave-one-out from L^-1 and alpha of the slots of v: labels (n) = the fold of every point, a permutation of 0 .. n-1 (k = n).
void launch_cv_loo(const BatchView& v, const int* labels, const double* targets, const double* eta, bool include_nugget, double* mean,
                   double* var, double* maha, double* log_score, int* ok, hipStream_t s);
// One pass of the k-fold path over `nslots` slots of a sub-engine of nsub rows (NPsub = roundup(nsub + 1, 128)).  tab: four ints per slot,
// { source emulator (index into v's buffers; -1: slot not used), caller row, fold, fold size }; folds (k, nsub): the training indices of
// every fold, -1 where it is shorter than nsub.  gather: subA[slot] <- the factor-matrix layout above with S = Kinv[F, F] (lower tiles of
// Kinv mirrored on load), alpha[F] in row nsub, a unit diagonal and a zero target for the missing points of a short fold (and for a
// slot that is not used).  finish: Linv / sol / res / info are the sub-engine's L^-1, solution rows, launch_logdet words and status words.
void launch_cv_gather(const BatchView& v, const int* folds, const int* tab, int nslots, double* subA, int nsub, int NPsub, hipStream_t s);
void launch_cv_finish(const int* folds, const int* tab, int nslots, const double* Linv, const double* sol, const double* res, const int* info,
                      int nsub, int NPsub, const double* targets, const double* eta, bool include_nugget, int n, int k, double* mean,
                      double* var, double* maha, double* log_score, int* ok, hipStream_t s);

// --- joint posterior draws (kernels_sample.hip) -----------------------------------------------------
// The scratch engine of sample_posterior has n' = m rows (NPs = roundup(m + 1, 128)); `sv` is ITS view, batch entry z of the launch
// = its slot sv.idx[z].  gather: A[slot] <- the factor-matrix layout above with Sigma* = cov[src[slot]] (m x m dense, row stride m) plus
// shift[slot] on its diagonal; the target row m is neutral (zeros, PAD_BIG on the diagonal), rows > m identity, src[slot] < 0 an identity
// matrix.  Only the 64 x 64 tiles on and below the diagonal carry the matrix: the tiles above it are written as exact zeros (the
// factorisation reads the lower triangle only, and sample_apply reads whole 128 x 128 diagonal blocks of the factor).
void launch_sample_gather(const BatchView& sv, const double* cov, const int* src, const double* shift, int m, hipStream_t s);
// Behind the factorisation, for the slots 0 .. nslots - 1 of the scratch engine with src[slot] >= 0: the diagonal of the factor recomputed from
// its finished row, L[j][j] = sqrt(Sigma~[j][j] - sum_{k<j} L[j][k]^2) with the correctly rounded square root (the factorisation's own diagonal
// comes from a reciprocal square root and may be one unit in the last place off; with a single point the draw is then mu + sqrt(Sigma~) z to
// the bit).  One wave per row, lane-strided partial sums added in a fixed order; a value that is not a positive finite number is not stored.
void launch_sample_polish(double* A, int NPs, int nslots, const double* cov, const int* src, const double* shift, int m, hipStream_t s);
// Z (nslots, zrows, MP) row-major, MP = roundup(m, 128): rows r < sc of every slot <- the standard normals of draws s0 + r at the points
// 0 .. m-1 of stream streams[slot] (philox_dev.h: a value depends on (seed, stream, draw, point) alone).  Columns >= m are not written.
void launch_sample_normals(double* Z, int nslots, long zrows, int MP, int m, int sc, long s0, unsigned long long seed, const unsigned* streams,
                           hipStream_t s);
// Y (nslots, yrows, m): Y[slot][r][j] = mu[slot][j] + sum_k L[slot][j][k] Z[slot][r][k] for r < sc, j < m; L = the lower triangle of
// A[slot] (nslots matrices NPs x NPs), its 128 x 128 diagonal blocks read whole (their strict upper triangle must hold zeros), Z as above
// with zrows a multiple of 64 and columns >= m zero.  fp64 MFMA, one writer per output, a fixed k order, no atomics.
void launch_sample_apply(const double* A, int NPs, const double* Z, long zrows, int MP, const double* mu, int m, int sc, int nslots,
                         double* Y, long yrows, hipStream_t s);

// --- active learning (kernels_alc.hip) ------------------------------------------------------------------
// Posterior cross covariance c(x, x') = sigma^2 k(x, x') - v(x)^T v(x') of two point sets from their stored V = L^-1 K*^T (launch_predict_v_store):
// V1 (nb, NP, MP1) / X1 (m1, D) the rows, V2 (nb, NP, MP2) / X2 (m2, D) the columns, one 128 x 128 tile per workgroup on fp64 MFMA, the prior
// term formed in the accumulator's layout.  store: out (nb, m1, m2) = c.
void launch_alc_store(const BatchView& v, const double* V1, int MP1, int m1, const double* X1, const double* V2, int MP2, int m2, const double* X2,
                      double* out, hipStream_t s);
// reduce: the columns are one chunk of the reference points, its first 128-point tile number tile0 of tiles_r in the whole set, w its
// weights (m2); part[(slot * tiles_r + tile0 + tj) * MP1 + i] = sum over the tile's columns j of w_j c(x_i, r_j)^2: ONE writer per entry, a
// fixed order inside the tile (the lane's four column blocks ascending, a 16-lane butterfly, the two wave columns), no atomics.
// rows: the rows of V per slot (v.NP as launch_predict_v_store leaves them; more where conditioning rows follow the base rows, alc_batch);
// kend: the K range [0, kend) of the product, whole 16-row steps (alc_kend(n) for the stored V alone).
inline int alc_kend(int n) { return (n + 15) / 16 * 16; }
void launch_alc_cross(const BatchView& v, const double* V1, int MP1, int m1, const double* X1, const double* V2, int MP2, int m2, const double* X2,
                      const double* w, int rows, int kend, int tile0, int tiles_r, double* part, hipStream_t s);
// per (slot, candidate i < m1): var[slot * var_ld + i] <- max(var, 0) = s^2; d = s^2 + tau[slot]; with the floor (nrows + 2) 2^-52 sigma^2
// (nrows = n, plus the picks conditioned on so far in alc_batch): d <= floor (or not a number): red = 0, deg = 1; else
// red = (sum of the tiles_r partials, ascending) / d, deg = 0
void launch_alc_finish(const BatchView& v, int nrows, int m1, int MP1, int tiles_r, const double* part, double* var, int var_ld, const double* tau,
                       double* red, int* deg, hipStream_t s);
// Greedy ALC batches (AlcBatch; DESIGN.md section 3 "Active learning: batches").  Per slot, step t of T:
//   argmax   the pick of step t: forced >= 0 that candidate, else the candidate with mask == 0 and the largest red (ties: the lowest index;
//            NaN never wins).  With d = max(var[pick], 0) + tau and the floor (n + t + 2) 2^-52 sigma^2: no candidate left, a best score
//            that is not above 0 or d at or below the floor give picks[slot * T + t] = -1, pick_red = 0 (nothing is conditioned on);
//            else picks = the index, pick_red = its red, pick_d = d.  mask[pick] = 1 either way.  One workgroup per slot.
//   condition  for the m points X (V (nb, rows, MP), tracked variances var) and the pick p of step t (Vc (nb, rows, MPc), Xc its
//            points): u(x) = (sigma^2 k(x, x_p) - sum_{k < n16 + t} V[k][x] Vc[k][p]) / sqrt(pick_d);  V[n16 + t][x] = u(x);
//            var[x] -= u(x)^2.  A slot whose pick is -1 is left alone (its row stays 0).  k in a fixed order, one owner per output.
void launch_alc_argmax(const BatchView& v, int t, int T, int forced, int m, const double* red, const double* var, int var_ld, const double* tau,
                       int* mask, int* picks, double* pick_red, double* pick_d, hipStream_t s);
void launch_alc_condition(const BatchView& v, int t, int T, int rows, const int* picks, const double* pick_d, const double* Vc, int MPc,
                          const double* Xc, double* V, int MP, int m, const double* X, double* var, int var_ld, hipStream_t s);

// --- local approximate GP (kernels_local.hip) -----------------------------------------------------------
// Prediction from the k nearest design points of every query alone (DESIGN.md section 3 "Local prediction").  Point indices are int (N < 2^31),
// element offsets size_t.
constexpr int LOCAL_MAX_K = 126;        // k neighbours + the target row + the query row share ONE 128 x 128 tile
constexpr long LOCAL_MAX_N = 2147483647L - 256;        // a tile's row index j0 + 127 of the neighbour search stays an int
constexpr int LOCAL_KNN_QW = 4;         // queries per wave of the neighbour search
constexpr int LOCAL_KNN_QUERIES = 4 * LOCAL_KNN_QW;    // ... per 256-thread workgroup
constexpr int LOCAL_KNN_ROWS = 128;     // design rows per staged tile
// per workgroup of local_gp_kernel: the 128 x 128 tile and the pack chol128_dev writes beside it (chol128_dev.h PACK128_STRIDE)
constexpr size_t LOCAL_WG_DOUBLES = (size_t)128 * 128 + 128 * 128 + 8 * 256;
// out[i][d] = x[i][d] * s[d]: one rounded multiply per element
void launch_local_scale(const double* x, long rows, int D, const double* s, double* out, hipStream_t st);
// Xs (N, D) and Qs (mc, D) scaled as above.  Per query the k smallest pairs (r2, index) in lexicographic order, ascending, r2 =
// ((0 + t_0 t_0) + t_1 t_1) + ..., t_d = Xs[i][d] - Qs[q][d], every operation rounded on its own (no FMA): nbr (mc, k), radius (mc) = the
// r2 of the last one.  One wave per LOCAL_KNN_QW queries, no atomics; a query's result does not depend on the others of the launch.
void launch_local_knn(const double* Xs, long N, int D, const double* Qs, int mc, int k, int* nbr, double* radius, hipStream_t st);
// Per query the GP on its k neighbours: mean = y^T Q^-1 k*, var = max(sigma2 - |L^-1 k*|^2 + var_add, 0), Q = sigma2 k(.,.) + diag_add I over
// the neighbours, kt = 0 squared exponential / 1 Matern 5/2 of the scaled distance; Y (N) residual targets.  ok = 0 and NaN where Q is not
// positive definite.  grid persistent workgroups, scratch: grid * LOCAL_WG_DOUBLES doubles.  No result bit depends on grid.
void launch_local_gp(const double* Xs, const double* Y, long N, int D, const double* Qs, int mc, int k, const int* nbr, int kt, double sigma2,
                     double diag_add, double var_add, double* scratch, int grid, double* mean, double* var, int* ok, hipStream_t st);
// Vecchia likelihood on the same handle (DESIGN.md section 3 "Vecchia fit").  The design is stored in the Vecchia order: the neighbours of
// row t are rows < t.
constexpr size_t VECCHIA_WG_DOUBLES = LOCAL_WG_DOUBLES + (size_t)128 * 128;      // with the gradient: sigma^2 k'(r2) of the pairs beside the tile
constexpr size_t VECCHIA_REDUCE_BLOCK = 1024;                                      // points per block of the fixed-order sum
// nbr (N, k): per row t the min(t, k) smallest pairs (r2, index) over the rows < t, the arithmetic and the order of launch_local_knn; -1 behind them
void launch_vecchia_knn(const double* Xs, long N, int D, int k, int* nbr, hipStream_t st);
// The points p0 .. p0 + mc - 1: out[t] = log p(y_t | y_nbr(t)) and, with grad, out[(1 + p) * N + t] = its derivative with respect to
// theta_p = log s_p^2 (p < D), log sigma2 (p = D) and log nugget (p = D + 1); ok[t] = 0 and NaN where the local matrix sigma2 k + diag_add I
// is not positive definite.  grid persistent workgroups; scratch: grid * (grad ? VECCHIA_WG_DOUBLES : LOCAL_WG_DOUBLES) doubles.
void launch_vecchia_ll(const double* Xs, const double* Y, long N, int D, long p0, int mc, int k, const int* nbr, int kt, double sigma2,
                       double diag_add, double nugget, bool grad, double* scratch, int grid, double* out, int* ok, hipStream_t st);
// the sums of the columns of in (cols, n), in an order that depends on n alone; a, b: cols * ceil(n / VECCHIA_REDUCE_BLOCK) doubles each;
// returns the one of them whose first cols entries are the sums
double* launch_vecchia_reduce(const double* in, long n, int cols, double* a, double* b, hipStream_t st);

// --- iterative exact prediction (kernels_iter.hip) ----------------------------------------------------
// Matrix-free preconditioned conjugate gradients on the whole design (DESIGN.md section 3 "Iterative exact prediction").  A PANEL is a set
// of columns stored one after another: entry (i, c) at [c * ld + i].  No kernel of the unit waits on another workgroup and none uses an
// atomic: every result is the same bits for a repeated call, and column c of a result depends on column c of its inputs alone.
constexpr int ITER_COLS = 32;           // columns of a CG panel (two MFMA blocks of 16 right-hand sides)
constexpr int ITER_SEG = 4096;          // rows per workgroup of the tall-skinny product L^T V (its partial sums are added in ascending order)
constexpr int ITER_DOT_BLOCK = 1024;    // rows per workgroup of a column-wise dot
// Out (M rows, 16 nb columns, ld ldo) = [sigma2 k(r2(As_i, Bs_j)) + nug * (same && i == j)] V (N rows, 16 nb columns, ld ldv); nb = 1 or 2.
// As (M, D), Bs (N, D) scaled coordinates; the entries are generated per lane (r2 with FMAs, kern_val with the staged table) as the A
// operand of v_mfma_f64_16x16x4_f64 and never stored.  A workgroup owns 64 rows and sweeps the columns j in ascending tiles of 64.
void launch_kmatvec(const double* As, long M, const double* Bs, long N, int D, int kt, double sigma2, double nug, bool same, const double* V,
                    long ldv, int nb, double* Out, long ldo, hipStream_t st);
// The input derivative of the rectangular product (DESIGN.md section 3 "Input derivatives at large designs"):
//   Out[(d * 16 nb + c) * ldo + i] = 2 scale[d] sum_j sigma2 k'(r2(Qs_i, Xs_j)) (Qs_id - Xs_jd) V[c * ldv + j]      d < D, c < 16 nb, i < M
// the derivative of sum_j sigma2 k(r2(q_i * scale, Xs_j)) V_jc with respect to the RAW coordinate d of query i (no nugget: it has no
// derivative).  Qs (M, D), Xs (N, D) scaled coordinates, scale (D) on the device, V a panel of 16 nb columns; nb = 1 or 2.  launch_kmatvec's
// tiling: the grid is (ceil(M / 64), ceil(D / INDERIV_DG)), a workgroup owns 64 queries and INDERIV_DG dimensions and sweeps the design in
// ascending tiles of 64; the lane generates r2 and sigma2 k' once per entry and feeds k' times the DIFFERENCE of the staged coordinates
// to the MFMAs of every dimension of its group against one staged B operand.  No atomics and no split of j: one fixed order of the sum; column
// c depends on column c of V alone, row i on query i alone; rows >= M and columns >= N are exact zeros, a query on a design point gets an
// exact zero from that point.
void launch_kinderiv(const double* Qs, long M, const double* Xs, long N, int D, int kt, double sigma2, const double* scale, const double* V, long ldv,
                     int nb, double* Out, long ldo, hipStream_t st);
// Partial pivoted Cholesky of sigma2 k(Xs, Xs), one step per call of launch_pchol_step: state[0] = the rank reached, state[1] = 1 once the
// largest remaining diagonal was <= 0 (later steps then do nothing); piv (rank) and the pivot's diagonal dmax (rank) stay on the device.
// L (N rows, `rank` columns, ld N); diag (N) the remaining diagonal; part: 2 * ceil(N / 1024) doubles and as many ints.
void launch_pchol_init(double* diag, long N, double sigma2, int* state, hipStream_t st);
void launch_pchol_step(const double* Xs, long N, int D, int kt, double sigma2, int t, double* L, double* diag, int* piv, double* dmax,
                       int* state, double* pval, int* pidx, hipStream_t st);
// G (p, p) = eta I + L^T L, every entry summed over the rows in ascending order
void launch_pchol_gram(const double* L, long N, int p, double eta, double* G, hipStream_t st);
// Z = (R - L Ginv L^T R) / eta on panels of ITER_COLS columns (ld N); wpart: ceil(N / ITER_SEG) * p * ITER_COLS doubles, w and w2: p * ITER_COLS
void launch_precond_apply(const double* L, long N, int p, const double* Ginv, double eta, const double* R, double* Z, double* wpart, double* w,
                          double* w2, hipStream_t st);
// column-wise <A_c, B_c> of two panels (ld N): part (ITER_COLS, ceil(N / ITER_DOT_BLOCK)), then launch_cg_scalars(step) adds them in ascending
// order and does that step's scalar work on the device.  sc: 5 * ITER_COLS doubles (bb, rz, alpha, beta, out), fl: 3 * ITER_COLS ints (frozen,
// converged, iterations).  CG_ALPHA, CG_TEST and CG_BETA leave a frozen column alone.
enum CgStep {
  CG_BB,      // bb = s; a column with s == 0 is frozen as converged at iteration 0
  CG_RZ,      // rz = s
  CG_ALPHA,   // s = p^T A p: alpha = rz / s, or frozen as not converged when s is not a positive finite number
  CG_TEST,    // s = |r|^2: frozen as converged at iteration it + 1 when sqrt(s) <= rtol sqrt(bb)
  CG_BETA,    // s = r^T z: beta = s / rz, rz = s
  CG_OUT      // out = s
};
void launch_cg_dot(const double* A, const double* B, long N, double* part, hipStream_t st);
// lg (or null): the coefficient log of the exact likelihood, lg[(2 it + 0) * ITER_COLS + c] = alpha of iteration it (CG_ALPHA) and
// lg[(2 it + 1) * ITER_COLS + c] = beta (CG_BETA), stored for the columns that are live at that point; no other result depends on it.
void launch_cg_scalars(CgStep step, const double* part, long N, double* sc, int* fl, int it, double rtol, hipStream_t st, double* lg = nullptr);
// x += alpha p with the roundings of that sum collected in xl (x + xl is the iterate), r -= alpha q;  p = z + beta p (first: p = z);
// out = a - b;  x += xl: panels of ITER_COLS columns (ld N).  The two updates leave frozen columns untouched.
void launch_cg_update(double* x, double* xl, double* r, const double* p, const double* q, long N, const double* sc, const int* fl, hipStream_t st);
void launch_panel_add(double* x, const double* xl, long N, hipStream_t st);
void launch_cg_direction(double* p, const double* z, long N, bool first, const double* sc, const int* fl, hipStream_t st);
void launch_panel_sub(const double* a, const double* b, long N, double* out, hipStream_t st);
// The probes of the exact likelihood, in place on a panel (ld N): Z[c][i] = sum_s L[s][i] g1[s * ITER_COLS + c] (ascending s, FMAs)
// + root * Z[c][i] for the columns c_lo <= c < c_hi, which hold the normals g2 on entry.  g1: p * ITER_COLS doubles.
void launch_probes(const double* L, long N, int p, const double* g1, double root, int c_lo, int c_hi, double* Z, hipStream_t st);
// The bilinear forms of the derivative matrices dA/dtheta_d = sigma2 k'(r2_ij) (x~_id - x~_jd)^2 in one sweep over the generated matrix:
//   out[d]     = sum_ij U[0][i] W[0][j] dA_ij/dtheta_d                               (the data pair: column 0 of the panels alone)
//   out[D + d] = sum over the columns c_lo <= c < c_hi (1 <= c_lo, c_hi <= ITER_COLS) of sum_ij U[c][i] W[c][j] dA_ij/dtheta_d
// U, W: panels of ITER_COLS columns (ld N).  A workgroup owns 64 rows and KGRAD_DC dimensions, forms S_ij = sum_c U_ic W_jc of a 16 x 16
// block with v_mfma_f64_16x16x4_f64, generates r2 and k' in the lane that holds S_ij and adds in a fixed order; part: ceil(N / 64) * 2 * D
// doubles, one partial per workgroup and output, added in ascending order by a second kernel (the one that adds the segments of launch_ltv).  No atomics; no bit of out[0 .. D) depends on
// the probe columns, and none of out on KGRAD_DC.
constexpr int KGRAD_DC = 16;
void launch_kgrad_forms(const double* Xs, long N, int D, int kt, double sigma2, const double* U, const double* W, int c_lo, int c_hi, double* part,
                        double* out, hipStream_t st);
// The variance bound (DESIGN.md section 3 "Variance bound").  w (p, ITER_COLS) = L^T R for a panel R of ITER_COLS columns: the first two
// steps of launch_precond_apply, which calls it (wpart: ceil(N / ITER_SEG) * p * ITER_COLS doubles).
void launch_ltv(const double* L, long N, int p, const double* R, double* wpart, double* w, hipStream_t st);
// Out[:, c0 .. c0 + 31] = In[:, :r] T[:, c0 .. c0 + 31] for panels In, Out (ld N) and an upper triangular T (r rows of ldt >= c0 + 32
// doubles, zeros below the diagonal), every entry summed over s in ascending order; columns >= r are not written.  In == Out is allowed when
// the blocks c0 are launched in descending order on one stream.
void launch_tri_right(const double* In, long N, int r, const double* T, int ldt, int c0, double* Out, hipStream_t st);
// part[i] = max(base - sum_{c < rank} (sum_j sigma2 k(r2(Qs_i, Xs_j)) R[c][j])^2, 0) for the M queries Qs (scaled coordinates); R a panel
// (ld ldr) of at least `rank` columns.  The grid is (ceil(M / 64), ceil(rank / ITER_VAR_CHUNK)): a workgroup owns 64 queries and ITER_VAR_NB
// MFMA blocks of 16 columns of R, generates its entries of k* by the sweep kmatvec_kernel runs and adds the squares in a fixed order; the chunks'
// partial sums part[chunk * M + i] are added in ascending order by a second kernel, in place.  part: M * ceil(rank / ITER_VAR_CHUNK) doubles.
// No atomics; a query's result depends on that query alone, and on `rank` only through the columns that enter.
// ITER_VAR_NB = 4: a generated entry (3 D + ~20 operations of the lane) then feeds four MFMAs, twice what it feeds in the solver's product,
// with 32 accumulator registers per lane and 33 KB of LDS for the staged columns beside the 1 KB per dimension of the two coordinate tiles
// (117 KB of the CU's 160 at D = 80, three workgroups per CU at D = 10); a wider chunk would leave m / 64 x chunks too few workgroups for
// the 256 CUs at the ranks below 256.
constexpr int ITER_VAR_NB = 4;
void launch_kvar(const double* Qs, long M, const double* Xs, long N, int D, int kt, double sigma2, const double* R, long ldr, int rank, double base,
                 double* part, hipStream_t st);

// --- pathwise posterior draws (kernels_rff.hip) ---------------------------------------------------------
// Random Fourier features that are generated and never stored (DESIGN.md section 3 "Pathwise posterior draws").
// Out (M rows, 16 nb columns, ld ldo) = amp Phi W with Phi_if = cos(t_if), t_if = phase[f] then fma(omega[f][d], Ps[i][d], t) over d ascending;
// Ps (M, D) scaled coordinates, omega (F, D), phase (F), W a panel of F rows and 16 nb columns (ld ldw); nb = 1 or 2.  kmatvec_kernel's
// tiling and lane layout: one cosine per lane as the A operand of v_mfma_f64_16x16x4_f64, the features in ascending tiles of 64, one
// fixed order of the sum, no atomics; column c of Out depends on column c of W alone, row i on point i alone.
void launch_rff(const double* Ps, long M, const double* omega, const double* phase, int F, int D, const double* W, long ldw, int nb, double amp,
                double* Out, long ldo, hipStream_t st);
// The input derivative of the feature product:
//   Out[(d * 16 nb + c) * ldo + i] = -(amp scale[d]) sum_f sin(t_if) (omega[f][d] W[c * ldw + f])      d < D, c < 16 nb, i < M
// with t_if built as launch_rff builds it (the same FMAs in the same order).  The grid is (ceil(M / 64), ceil(D / INDERIV_DG)): the sine is the
// A operand of the MFMAs of every dimension of the group, the B operand is one rounded product of the staged frequency and weight.  The
// sines are never stored; no atomics, one fixed order of the sum; column c depends on column c of W alone, row i on point i alone.
void launch_rff_inderiv(const double* Ps, long M, const double* omega, const double* phase, int F, int D, const double* W, long ldw, int nb, double amp,
                        const double* scale, double* Out, long ldo, hipStream_t st);
// W[c * ldw + j] = the normal j of draw draw0 + c of (seed, stream) (philox_dev.h) for c < cols, j < n
void launch_rff_normals(unsigned long long seed, unsigned stream, unsigned draw0, int cols, long n, double* W, long ldw, hipStream_t st);
// The right-hand sides of the paths, panels of ITER_COLS columns (ld N): B[c][i] = fma(-root, noise, y[i] - g[c][i]) for c < cols, exact zeros
// behind them; the noise is E[c][i] or, with E null, the normal i of draw draw0 + c of (seed, stream).
void launch_rff_rhs(const double* y, const double* g, const double* E, long N, int cols, double root, unsigned long long seed, unsigned stream,
                    unsigned draw0, double* B, hipStream_t st);

// --- utilities -------------------------------------------------------------------------------
// out (n,n) <- tile of src (NP,NP): mode 0 copy, mode 1 transpose of the lower triangle (zeros below the diagonal of out), mode 2 symmetrise from lower
void launch_extract(const double* src, int NP, int n, double* out, int mode, hipStream_t s);

// --- profiling hooks (bench only) -------------------------------------------------------------
bool prof_is_on();
void prof_begin(const char* tag, hipStream_t s);
void prof_end(const char* tag, hipStream_t s, double flops, double bytes);

}  // namespace mogp
