// The kernels of the iterative exact prediction (engine_iter.hip) and their launchers: conjugate gradients on (K + eta I) of the WHOLE
// design, K never stored (Gardner et al. 2018; Wang et al. 2019).  A panel is a set of columns stored one after another, entry (i, c) at
// [c * ld + i].
//
//   kmatvec_kernel       Out = [sigma2 k(r2(A_i, B_j)) + eta (same set, i = j)] V.  A workgroup of four waves owns 64 output rows, a wave 16
//                        of them, and sweeps the columns j in ascending tiles of 64 whose scaled rows and whose rows of V are staged in LDS.
//                        One v_mfma_f64_16x16x4_f64 takes 16 rows i x 4 columns j as its A operand -- one kernel entry per lane, generated
//                        by that lane (r2 by FMAs over d, kern_val with the staged exponential table) and never stored -- and 4 rows of V x 16
//                        right-hand sides as its B operand; the entry feeds every block of 16 right-hand sides.  No atomics and no split of
//                        j across workgroups: the sum of a row runs over j in one fixed order.  Column c of Out depends on column c of V
//                        alone (the MFMA keeps its columns apart).  Rows >= M are not stored, entries of columns >= N are exact zeros.
//   pchol_*_kernel       partial pivoted Cholesky of sigma2 k(X, X), one column per step: the largest remaining diagonal entry by a two-stage
//                        reduction on pairs (value, index), ties to the lowest index (a total order: the result does not depend on the
//                        order of the comparisons); the column of K generated, L[:, :t] L[piv, :t]^T subtracted in ascending t, scaled;
//                        the diagonal updated.  The pivot index, its diagonal and the rank reached stay on the device.
//   gram_kernel          G = eta I + L^T L, 16 x 16 entries per workgroup, each summed over the rows in ascending order
//   ltv / z kernels      P^-1 R = (R - L Ginv L^T R) / eta: L^T R in segments of ITER_SEG rows added in ascending order, the p x p product
//                        with Ginv, and L times it with 32 accumulators per row
//   cg_*_kernel          column-wise dots (x carried as a compensated sum; blocks of ITER_DOT_BLOCK rows in a fixed tree, the blocks added in ascending order by one thread
//                        per column, which also does the step's scalar work: the step scalars and the frozen flags never leave the
//                        device) and the fused updates, which leave a frozen column alone
//   probe_kernel         the probes of the exact likelihood (engine_iter_lik.hip), Z = L g1 + sqrt(eta) g2, one row per thread
//   kgrad_forms_kernel   sum_ij U_ic W_jc dA_ij/dtheta_d for the data column and for the sum over the probe columns, in one sweep over the
//                        generated matrix on kmatvec_kernel's tiling: the MFMA forms S_ij = sum_c U_ic W_jc, the lane that holds S_ij
//                        generates sigma2 k'(r2_ij) and adds per dimension; one partial per workgroup, added in ascending order
//   tri_right_kernel     a tall panel times an upper triangular matrix, 32 columns per launch: the two orthonormalisations of the variance
//                        bound's cache (engine_iter.hip iter_var_build)
//   kvar_kernel          sum_c (sum_j sigma2 k(r2(q_i, x_j)) R_jc)^2 on kmatvec_kernel's tiling, the grid split over chunks of ITER_VAR_CHUNK
//                        columns of R; kvar_reduce_kernel adds the chunks in ascending order and forms max(base - sum, 0)
// Every launch is a plain grid that ends by itself: nothing here waits on another workgroup.
#include <algorithm>
#include <climits>

#include "cov_dev.h"
#include "predict_plan.h"

namespace mogp {

namespace {

typedef double v4d __attribute__((ext_vector_type(4)));

constexpr int KM_ROWS = 64;             // rows of a workgroup and columns of a staged tile

template <int NB>
constexpr int km_ldv() { return 16 * NB + 1; }      // odd row stride of the staged rows of V: the transposing stores spread over the banks

// LDS: tab (256) | sa (D x 64) | sb (D x 64) | sv (64 x km_ldv)
template <int KT, int NB>
__global__ __launch_bounds__(256) void kmatvec_kernel(const double* __restrict__ As, int M, const double* __restrict__ Bs, int N, int D,
                                                      double sigma2, double nug, int same, const double* __restrict__ V, size_t ldv,
                                                      double* __restrict__ Out, size_t ldo) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  constexpr int LDV = km_ldv<NB>();
  double* tab = sm;
  double* sa = tab + 256;
  double* sb = sa + (size_t)KM_ROWS * D;
  double* sv = sb + (size_t)KM_ROWS * D;
  const int t = threadIdx.x, lane = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int i0 = blockIdx.x * KM_ROWS;
  const int il = w * 16 + (lane & 15), jq = lane >> 4, cl = lane & 15;
  const int gi = i0 + il;
  stage_exp_tab(tab);
  stage_rows(As, M, D, i0, sa);
  v4d acc[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) acc[b] = v4d{0.0, 0.0, 0.0, 0.0};
  for (int j0 = 0; j0 < N; j0 += KM_ROWS) {
    __syncthreads();                                         // the previous tile has been read
    stage_rows(Bs, N, D, j0, sb);
    for (int e = t; e < KM_ROWS * 16 * NB; e += 256) {
      const int j = e & 63, c = e >> 6;
      sv[j * LDV + c] = (j0 + j < N) ? V[(size_t)c * ldv + (size_t)(j0 + j)] : 0.0;
    }
    __syncthreads();
#pragma unroll 1
    for (int g = 0; g < 4; ++g) {                            // 16 columns: four MFMA steps of four
      double r2[4] = {0.0, 0.0, 0.0, 0.0};
      for (int d = 0; d < D; ++d) {
        const double a = sa[d * 64 + il];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const double df = a - sb[d * 64 + (g * 4 + u) * 4 + jq];
          r2[u] = __builtin_fma(df, df, r2[u]);
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int jl = (g * 4 + u) * 4 + jq;
        const int gj = j0 + jl;
        const double kk = kern_val<KT>(r2[u], tab);
        double kv = (same && gi == gj) ? __builtin_fma(sigma2, kk, nug) : sigma2 * kk;      // (explicit: the same bits in every instantiation)
        if (gj >= N || gi >= M) kv = 0.0;
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(kv, sv[jl * LDV + b * 16 + cl], acc[b], 0, 0, 0);
      }
    }
  }
  // C fragment: row (lane >> 4) + 4 reg, column lane & 15
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int i = i0 + w * 16 + jq + 4 * reg;
      if (i < M) Out[(size_t)(b * 16 + cl) * ldo + (size_t)i] = acc[b][reg];
    }
}

// ---- partial pivoted Cholesky ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool pair_better(double a, int ai, double b, int bi) { return a > b || (a == b && ai < bi); }

__global__ __launch_bounds__(256) void pchol_init_kernel(double* __restrict__ diag, size_t N, double sigma2, int* __restrict__ state) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < N) diag[i] = sigma2;
  if (i < 2) state[i] = 0;
}

// the tree over the 256 pairs of a workgroup; the best pair is in (sv[0], si[0]) afterwards
__device__ __forceinline__ void pair_tree(double* sv, int* si, double bv, int bi) {
  const int t = threadIdx.x;
  sv[t] = bv;
  si[t] = bi;
  for (int off = 128; off > 0; off >>= 1) {
    __syncthreads();
    if (t < off && pair_better(sv[t + off], si[t + off], sv[t], si[t])) {
      sv[t] = sv[t + off];
      si[t] = si[t + off];
    }
  }
  __syncthreads();
}

__global__ __launch_bounds__(256) void pchol_argmax1_kernel(const double* __restrict__ diag, int N, const int* __restrict__ state,
                                                            double* __restrict__ pval, int* __restrict__ pidx) {
  __shared__ double sv[256];
  __shared__ int si[256];
  if (state[1]) return;
  const int t = threadIdx.x;
  double bv = -__builtin_inf();
  int bi = INT_MAX;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const long i = (long)blockIdx.x * 1024 + u * 256 + t;
    if (i < N) {
      const double v = diag[i];
      if (pair_better(v, (int)i, bv, bi)) {
        bv = v;
        bi = (int)i;
      }
    }
  }
  pair_tree(sv, si, bv, bi);
  if (t == 0) {
    pval[blockIdx.x] = sv[0];
    pidx[blockIdx.x] = si[0];
  }
}

__global__ __launch_bounds__(256) void pchol_argmax2_kernel(const double* __restrict__ pval, const int* __restrict__ pidx, int nb, int step,
                                                            int* __restrict__ state, int* __restrict__ piv, double* __restrict__ dmax) {
  __shared__ double sv[256];
  __shared__ int si[256];
  if (state[1]) return;
  const int t = threadIdx.x;
  double bv = -__builtin_inf();
  int bi = INT_MAX;
  for (int b = t; b < nb; b += 256)
    if (pair_better(pval[b], pidx[b], bv, bi)) {
      bv = pval[b];
      bi = pidx[b];
    }
  pair_tree(sv, si, bv, bi);
  if (t == 0) {
    if (sv[0] > 0.0 && si[0] != INT_MAX) {
      piv[step] = si[0];
      dmax[step] = sv[0];
      state[0] = step + 1;
    } else {
      state[1] = 1;                                          // the largest remaining diagonal is <= 0 (or NaN): the rank stops here
    }
  }
}

// column `step` of L and the diagonal behind it.  LDS: the table, the pivot's scaled row and the pivot's row of L
template <int KT>
__global__ __launch_bounds__(256) void pchol_column_kernel(const double* __restrict__ Xs, int N, int D, double sigma2, int step,
                                                           double* __restrict__ L, double* __restrict__ diag, const int* __restrict__ piv,
                                                           const double* __restrict__ dmax, const int* __restrict__ state) {
  __shared__ double tab[256];
  __shared__ double xp[MAX_D];
  __shared__ double lp[ITER_MAX_RANK];
  if (state[1]) return;
  const int t = threadIdx.x;
  const int pv = piv[step];
  const size_t ld = (size_t)N;
  stage_exp_tab(tab);
  if (t < D) xp[t] = Xs[(size_t)pv * D + t];
  for (int s = t; s < step; s += 256) lp[s] = L[(size_t)s * ld + pv];
  __syncthreads();
  const long i = (long)blockIdx.x * 256 + t;
  if (i >= N) return;
  const double* xi = Xs + (size_t)i * D;
  double r2 = 0.0;
  for (int d = 0; d < D; ++d) {
    const double df = xi[d] - xp[d];
    r2 = __builtin_fma(df, df, r2);
  }
  double c = sigma2 * kern_val<KT>(r2, tab);
  for (int s = 0; s < step; ++s) c = __builtin_fma(-L[(size_t)s * ld + i], lp[s], c);
  const double root = sqrt(dmax[step]);
  double l = c / root;
  if (i == pv) {
    l = root;
    diag[i] = 0.0;                                           // never picked again: the factorisation stops at a maximum <= 0
  } else {
    diag[i] = __builtin_fma(-l, l, diag[i]);
  }
  L[(size_t)step * ld + i] = l;
}

// G = eta I + L^T L: workgroup (x, y), y <= x, owns the entries (16 x + a, 16 y + b) and writes their mirror images too
__global__ __launch_bounds__(256) void gram_kernel(const double* __restrict__ L, int N, int p, double eta, double* __restrict__ G) {
  __shared__ double la[16 * 65], lb[16 * 65];
  if (blockIdx.y > blockIdx.x) return;
  const int t = threadIdx.x, a = t >> 4, b = t & 15;
  const int a0 = blockIdx.x * 16, b0 = blockIdx.y * 16;
  const size_t ld = (size_t)N;
  double acc = 0.0;
  for (int i0 = 0; i0 < N; i0 += 64) {
    __syncthreads();
    for (int e = t; e < 16 * 64; e += 256) {
      const int col = e >> 6, k = e & 63;
      const bool in = i0 + k < N;
      la[col * 65 + k] = (in && a0 + col < p) ? L[(size_t)(a0 + col) * ld + i0 + k] : 0.0;
      lb[col * 65 + k] = (in && b0 + col < p) ? L[(size_t)(b0 + col) * ld + i0 + k] : 0.0;
    }
    __syncthreads();
#pragma unroll 8
    for (int k = 0; k < 64; ++k) acc = __builtin_fma(la[a * 65 + k], lb[b * 65 + k], acc);
  }
  const int ga = a0 + a, gb = b0 + b;
  if (ga < p && gb < p) {
    if (ga == gb) acc += eta;
    G[(size_t)ga * p + gb] = acc;
    G[(size_t)gb * p + ga] = acc;
  }
}

// ---- the preconditioner's three products -------------------------------------------------------------------------------------------------
// wpart[(seg * p + a) * 32 + c] = sum over the rows of segment seg of L[i][a] R[i][c]
__global__ __launch_bounds__(256) void ltv_kernel(const double* __restrict__ L, int N, int p, const double* __restrict__ R,
                                                  double* __restrict__ wpart) {
  __shared__ double la[16 * 65], lv[ITER_COLS * 65];
  const int t = threadIdx.x, a = t >> 4, c2 = t & 15;
  const int a0 = blockIdx.x * 16;
  const size_t ld = (size_t)N;
  const long ibeg = (long)blockIdx.y * ITER_SEG;
  const int iend = ibeg + ITER_SEG < (long)N ? (int)(ibeg + ITER_SEG) : N;
  double acc0 = 0.0, acc1 = 0.0;
  for (int i0 = (int)ibeg; i0 < iend; i0 += 64) {
    __syncthreads();
    for (int e = t; e < 16 * 64; e += 256) {
      const int col = e >> 6, k = e & 63;
      la[col * 65 + k] = (i0 + k < iend && a0 + col < p) ? L[(size_t)(a0 + col) * ld + i0 + k] : 0.0;
    }
    for (int e = t; e < ITER_COLS * 64; e += 256) {
      const int col = e >> 6, k = e & 63;
      lv[col * 65 + k] = (i0 + k < iend) ? R[(size_t)col * ld + i0 + k] : 0.0;
    }
    __syncthreads();
#pragma unroll 8
    for (int k = 0; k < 64; ++k) {
      const double l = la[a * 65 + k];
      acc0 = __builtin_fma(l, lv[c2 * 65 + k], acc0);
      acc1 = __builtin_fma(l, lv[(c2 + 16) * 65 + k], acc1);
    }
  }
  if (a0 + a < p) {
    double* dst = wpart + ((size_t)blockIdx.y * p + a0 + a) * ITER_COLS;
    dst[c2] = acc0;
    dst[c2 + 16] = acc1;
  }
}

__global__ __launch_bounds__(256) void ltv_reduce_kernel(const double* __restrict__ wpart, int nseg, int p, double* __restrict__ w) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= p * ITER_COLS) return;
  double s = 0.0;
  for (int g = 0; g < nseg; ++g) s += wpart[(size_t)g * p * ITER_COLS + e];
  w[e] = s;
}

__global__ __launch_bounds__(256) void ginv_kernel(const double* __restrict__ Ginv, int p, const double* __restrict__ w, double* __restrict__ w2) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= p * ITER_COLS) return;
  const int a = e / ITER_COLS, c = e - a * ITER_COLS;
  double s = 0.0;
  for (int b = 0; b < p; ++b) s = __builtin_fma(Ginv[(size_t)a * p + b], w[b * ITER_COLS + c], s);
  w2[e] = s;
}

__global__ __launch_bounds__(256) void precond_z_kernel(const double* __restrict__ L, int N, int p, const double* __restrict__ w2, double eta,
                                                        const double* __restrict__ R, double* __restrict__ Z) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const size_t ld = (size_t)N;
  double acc[ITER_COLS];
#pragma unroll
  for (int c = 0; c < ITER_COLS; ++c) acc[c] = 0.0;
  for (int s = 0; s < p; ++s) {
    const double l = L[(size_t)s * ld + i];
#pragma unroll
    for (int c = 0; c < ITER_COLS; ++c) acc[c] = __builtin_fma(l, w2[s * ITER_COLS + c], acc[c]);
  }
#pragma unroll
  for (int c = 0; c < ITER_COLS; ++c) Z[(size_t)c * ld + i] = (R[(size_t)c * ld + i] - acc[c]) / eta;
}

// ---- conjugate gradients: dots, scalars, updates -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cg_dot_kernel(const double* __restrict__ A, const double* __restrict__ B, int N, double* __restrict__ part) {
  __shared__ double s[256];
  const int t = threadIdx.x, c = blockIdx.y;
  const double* a = A + (size_t)c * N;
  const double* b = B + (size_t)c * N;
  double acc = 0.0;
#pragma unroll
  for (int u = 0; u < ITER_DOT_BLOCK / 256; ++u) {
    const long i = (long)blockIdx.x * ITER_DOT_BLOCK + u * 256 + t;
    if (i < N) acc = __builtin_fma(a[i], b[i], acc);
  }
  s[t] = acc;
  for (int off = 128; off > 0; off >>= 1) {
    __syncthreads();
    if (t < off) s[t] += s[t + off];
  }
  if (t == 0) part[(size_t)c * gridDim.x + blockIdx.x] = s[0];
}

// sc: bb | rz | alpha | beta | out, ITER_COLS each; fl: frozen | converged | iterations
__global__ __launch_bounds__(64) void cg_scalars_kernel(int mode, const double* __restrict__ part, int nblk, double* __restrict__ sc,
                                                        int* __restrict__ fl, int it, double rtol, double* __restrict__ lg) {
  const int c = threadIdx.x;
  if (c >= ITER_COLS) return;
  double s = 0.0;
  for (int b = 0; b < nblk; ++b) s += part[(size_t)c * nblk + b];
  double *bb = sc, *rz = sc + ITER_COLS, *alpha = sc + 2 * ITER_COLS, *beta = sc + 3 * ITER_COLS, *out = sc + 4 * ITER_COLS;
  int *frozen = fl, *conv = fl + ITER_COLS, *iters = fl + 2 * ITER_COLS;
  const bool good = s > 0.0 && s <= 1.7e308;                 // a positive finite number
  if (mode == 0) {
    bb[c] = s;
    frozen[c] = good ? 0 : 1;
    conv[c] = s == 0.0 ? 1 : 0;
    iters[c] = 0;
  } else if (mode == 1) {
    rz[c] = s;
  } else if (mode == 5) {
    out[c] = s;
  } else if (!frozen[c]) {
    if (mode == 2) {
      if (good) {
        alpha[c] = rz[c] / s;
        if (lg) lg[(size_t)(2 * it) * ITER_COLS + c] = alpha[c];
      } else {
        frozen[c] = 1;
        conv[c] = 0;
        iters[c] = it;
      }
    } else if (mode == 3) {
      if (sqrt(s) <= rtol * sqrt(bb[c])) {
        frozen[c] = 1;
        conv[c] = 1;
        iters[c] = it + 1;
      }
    } else {
      beta[c] = s / rz[c];
      rz[c] = s;
      if (lg) lg[(size_t)(2 * it + 1) * ITER_COLS + c] = beta[c];
    }
  }
}

// x is carried as the unevaluated sum x + xl: every rounding of x + alpha p goes into xl (Knuth's two-sum; contraction is off in this kernel,
// a fused multiply-add would break it).  |x| grows to |A^-1 b| while the steps shrink, so without xl every late step costs a rounding of
// the size of x itself, and A times those is the gap between the recurrence residual and the true one.
__global__ __launch_bounds__(256) void cg_update_kernel(double* __restrict__ x, double* __restrict__ xl, double* __restrict__ r,
                                                        const double* __restrict__ p, const double* __restrict__ q, int N,
                                                        const double* __restrict__ sc, const int* __restrict__ fl) {
#pragma clang fp contract(off)
  const int c = blockIdx.y;
  if (fl[c]) return;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const size_t o = (size_t)c * N + i;
  const double a = sc[2 * ITER_COLS + c];
  const double x0 = x[o], ph = a * p[o];
  const double s = x0 + ph;
  const double bb = s - x0;
  const double err = (x0 - (s - bb)) + (ph - bb);
  x[o] = s;
  xl[o] = xl[o] + err;
  r[o] = __builtin_fma(-a, q[o], r[o]);
}

__global__ __launch_bounds__(256) void cg_direction_kernel(double* __restrict__ p, const double* __restrict__ z, int N, int first,
                                                           const double* __restrict__ sc, const int* __restrict__ fl) {
  const int c = blockIdx.y;
  if (fl[c]) return;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const size_t o = (size_t)c * N + i;
  p[o] = first ? z[o] : __builtin_fma(sc[3 * ITER_COLS + c], p[o], z[o]);
}

__global__ __launch_bounds__(256) void panel_sub_kernel(const double* __restrict__ a, const double* __restrict__ b, int N, double* __restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const size_t o = (size_t)blockIdx.y * N + i;
  out[o] = a[o] - b[o];
}

__global__ __launch_bounds__(256) void panel_add_kernel(double* __restrict__ x, const double* __restrict__ xl, int N) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const size_t o = (size_t)blockIdx.y * N + i;
  x[o] = x[o] + xl[o];
}

// ---- the exact likelihood: probes and the forms of the derivative matrices ---------------------------------------------------------------------
// column c_lo + blockIdx.y of the panel Z, one row per thread: the normals g2 it holds become L g1 + root g2
__global__ __launch_bounds__(256) void probe_kernel(const double* __restrict__ L, int N, int p, const double* __restrict__ g1, double root, int c_lo,
                                                    double* __restrict__ Z) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const int c = c_lo + blockIdx.y;
  const size_t ld = (size_t)N;
  double acc = 0.0;
  for (int s = 0; s < p; ++s) acc = __builtin_fma(L[(size_t)s * ld + i], g1[s * ITER_COLS + c], acc);
  Z[(size_t)c * ld + i] = __builtin_fma(root, Z[(size_t)c * ld + i], acc);
}

constexpr int KG_LDP = ITER_COLS + 1;   // odd row stride of the staged panel rows

// Workgroup (x, y): rows [64 x, 64 x + 64), dimensions [KGRAD_DC y, KGRAD_DC y + KGRAD_DC).  A wave owns 16 rows; per tile of 64 columns and
// block g of 16 of them the wave forms S (16 x 16) = sum over the probe columns of U_ic W_jc by MFMA (operands: row / column lane & 15,
// panel column 4 s + (lane >> 4); the lane then holds S of rows (lane >> 4) + 4 reg and column lane & 15), generates r2 of its four entries over
// ALL dimensions and sigma2 k', and adds (S sigma2 k') (x~_id - x~_jd)^2 -- and the same with the data pair's U_i0 W_j0, one plain product,
// in place of S -- into the accumulators of its slice of dimensions.  A slice repeats the generation: KGRAD_DC accumulator pairs are
// what a lane holds in registers.  The sum of one output runs over tiles, blocks and reg in one fixed order whatever the slice, then over the
// lanes by a fixed shuffle tree, the waves and (kgrad_reduce_kernel) the workgroups in ascending order.  Rows and columns >= N enter with
// zero panel rows, the diagonal with a zero difference.
// LDS: tab (256) | sa (D x 64) | sb (D x 64) | su (64 x 33) | sw (64 x 33) | su0 (64) | sw0 (64) | red (4 x 2 KGRAD_DC)
template <int KT>
__global__ __launch_bounds__(256) void kgrad_forms_kernel(const double* __restrict__ Xs, int N, int D, double sigma2, const double* __restrict__ U,
                                                          const double* __restrict__ W, size_t ld, int c_lo, int c_hi, double* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  double* tab = sm;
  double* sa = tab + 256;
  double* sb = sa + (size_t)KM_ROWS * D;
  double* su = sb + (size_t)KM_ROWS * D;
  double* sw = su + KM_ROWS * KG_LDP;
  double* su0 = sw + KM_ROWS * KG_LDP;
  double* sw0 = su0 + KM_ROWS;
  double* red = sw0 + KM_ROWS;
  const int t = threadIdx.x, lane = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int i0 = blockIdx.x * KM_ROWS, d0 = blockIdx.y * KGRAD_DC;
  const int jq = lane >> 4, cl = lane & 15;
  const int s_lo = c_lo >> 2, s_hi = (c_hi + 3) >> 2;        // the MFMA steps that hold a probe column (the others would add exact zeros)
  stage_exp_tab(tab);
  stage_rows(Xs, N, D, i0, sa);
  for (int e = t; e < KM_ROWS * ITER_COLS; e += 256) {
    const int i = e & 63, c = e >> 6;
    su[i * KG_LDP + c] = (c >= c_lo && c < c_hi && i0 + i < N) ? U[(size_t)c * ld + (size_t)(i0 + i)] : 0.0;
  }
  if (t < KM_ROWS) su0[t] = (i0 + t < N) ? U[(size_t)(i0 + t)] : 0.0;
  double accp[KGRAD_DC], accd[KGRAD_DC];
#pragma unroll
  for (int dd = 0; dd < KGRAD_DC; ++dd) accp[dd] = accd[dd] = 0.0;
  for (int j0 = 0; j0 < N; j0 += KM_ROWS) {
    __syncthreads();                                         // the previous tile has been read (first pass: nothing to wait for)
    stage_rows(Xs, N, D, j0, sb);
    for (int e = t; e < KM_ROWS * ITER_COLS; e += 256) {
      const int j = e & 63, c = e >> 6;
      sw[j * KG_LDP + c] = (c >= c_lo && c < c_hi && j0 + j < N) ? W[(size_t)c * ld + (size_t)(j0 + j)] : 0.0;
    }
    if (t < KM_ROWS) sw0[t] = (j0 + t < N) ? W[(size_t)(j0 + t)] : 0.0;
    __syncthreads();
#pragma unroll 1
    for (int g = 0; g < 4; ++g) {
      const int jl = g * 16 + cl;
      v4d S = v4d{0.0, 0.0, 0.0, 0.0};
      for (int s = s_lo; s < s_hi; ++s)
        S = __builtin_amdgcn_mfma_f64_16x16x4f64(su[(w * 16 + cl) * KG_LDP + 4 * s + jq], sw[jl * KG_LDP + 4 * s + jq], S, 0, 0, 0);
      double r2[4] = {0.0, 0.0, 0.0, 0.0};
      for (int d = 0; d < D; ++d) {
        const double b = sb[d * 64 + jl];
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const double df = sa[d * 64 + w * 16 + jq + 4 * reg] - b;
          r2[reg] = __builtin_fma(df, df, r2[reg]);
        }
      }
      const double w0 = sw0[jl];
      double cp[4], cd[4];
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const double kd = sigma2 * kern_dr2<KT>(r2[reg], tab);
        cp[reg] = S[reg] * kd;
        cd[reg] = (su0[w * 16 + jq + 4 * reg] * w0) * kd;
      }
#pragma unroll
      for (int dd = 0; dd < KGRAD_DC; ++dd) {
        const int d = d0 + dd;
        if (d < D) {
          const double b = sb[d * 64 + jl];
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) {
            const double df = sa[d * 64 + w * 16 + jq + 4 * reg] - b;
            const double q = df * df;
            accp[dd] = __builtin_fma(cp[reg], q, accp[dd]);
            accd[dd] = __builtin_fma(cd[reg], q, accd[dd]);
          }
        }
      }
    }
  }
#pragma unroll
  for (int dd = 0; dd < KGRAD_DC; ++dd) {
    double a = accd[dd], b = accp[dd];
    for (int off = 32; off > 0; off >>= 1) {
      a += __shfl_down(a, off, 64);
      b += __shfl_down(b, off, 64);
    }
    if (lane == 0) {
      red[w * 2 * KGRAD_DC + dd] = a;
      red[w * 2 * KGRAD_DC + KGRAD_DC + dd] = b;
    }
  }
  __syncthreads();
  if (t < 2 * KGRAD_DC) {
    const int grp = t / KGRAD_DC, d = d0 + (t - grp * KGRAD_DC);
    double s = red[t];
    for (int v = 1; v < 4; ++v) s += red[v * 2 * KGRAD_DC + t];
    if (d < D) part[((size_t)blockIdx.x * 2 + grp) * D + d] = s;
  }
}

// out[e] = the partials of the workgroups in ascending order; part (nblk, n)
__global__ __launch_bounds__(256) void kgrad_reduce_kernel(const double* __restrict__ part, int nblk, int n, double* __restrict__ out) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  double s = 0.0;
  for (int b = 0; b < nblk; ++b) s += part[(size_t)b * n + e];
  out[e] = s;
}

// ---- the variance bound: the cache's triangular products and the sum of squares over the generated cross covariance --------------------------
// Out[:, c0 + c] = sum over s <= c0 + c of In[:, s] T[s][c0 + c] for the 32 columns of block c0, one row per thread, s ascending (T is upper
// triangular with zeros stored below its diagonal: those terms leave the accumulator as it is).  Only columns < r are written.  In == Out is
// allowed when the blocks are launched in descending order: a thread reads its own row of the columns <= c0 + 31 and writes that row alone.
__global__ __launch_bounds__(256) void tri_right_kernel(const double* In, int N, int r, const double* __restrict__ T, int ldt, int c0, double* Out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const size_t ld = (size_t)N;
  double acc[ITER_COLS];
#pragma unroll
  for (int c = 0; c < ITER_COLS; ++c) acc[c] = 0.0;
  const int send = c0 + ITER_COLS < r ? c0 + ITER_COLS : r;
  for (int s = 0; s < send; ++s) {
    const double l = In[(size_t)s * ld + i];
#pragma unroll
    for (int c = 0; c < ITER_COLS; ++c) acc[c] = __builtin_fma(l, T[(size_t)s * ldt + c0 + c], acc[c]);
  }
#pragma unroll
  for (int c = 0; c < ITER_COLS; ++c)
    if (c0 + c < r) Out[(size_t)(c0 + c) * ld + i] = acc[c];
}

// part[chunk * ldp + i] = sum over the columns c of chunk blockIdx.y (16 NB of them, those >= rank as exact zeros) of
// (sum_j sigma2 k(r2(Q_i, X_j)) R_jc)^2.  The sweep is kmatvec_kernel's: a workgroup owns 64 queries, a wave 16, the design columns j come
// in ascending tiles of 64, every lane generates its entry of k* once and feeds it as the A operand to the NB blocks of 16 columns of R staged
// in LDS.  A lane then holds the sums of rows (lane >> 4) + 4 reg and column lane & 15: it squares them, the 16 column lanes are added by a
// fixed butterfly (both partners form the same sum), the blocks in ascending order.  One writer per entry of part, no atomics.
// LDS: tab (256) | sa (D x 64) | sb (D x 64) | sv (64 x km_ldv)
template <int KT, int NB>
__global__ __launch_bounds__(256) void kvar_kernel(const double* __restrict__ Qs, int M, const double* __restrict__ Xs, int N, int D, double sigma2,
                                                   const double* __restrict__ R, size_t ldr, int rank, double* __restrict__ part, size_t ldp) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  constexpr int LDV = km_ldv<NB>();
  double* tab = sm;
  double* sa = tab + 256;
  double* sb = sa + (size_t)KM_ROWS * D;
  double* sv = sb + (size_t)KM_ROWS * D;
  const int t = threadIdx.x, lane = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int i0 = blockIdx.x * KM_ROWS, c0 = blockIdx.y * 16 * NB;
  const int il = w * 16 + (lane & 15), jq = lane >> 4, cl = lane & 15;
  const int gi = i0 + il;
  stage_exp_tab(tab);
  stage_rows(Qs, M, D, i0, sa);
  v4d acc[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) acc[b] = v4d{0.0, 0.0, 0.0, 0.0};
  for (int j0 = 0; j0 < N; j0 += KM_ROWS) {
    __syncthreads();                                         // the previous tile has been read
    stage_rows(Xs, N, D, j0, sb);
    for (int e = t; e < KM_ROWS * 16 * NB; e += 256) {
      const int j = e & 63, c = e >> 6;
      sv[j * LDV + c] = (j0 + j < N && c0 + c < rank) ? R[(size_t)(c0 + c) * ldr + (size_t)(j0 + j)] : 0.0;
    }
    __syncthreads();
#pragma unroll 1
    for (int g = 0; g < 4; ++g) {
      double r2[4] = {0.0, 0.0, 0.0, 0.0};
      for (int d = 0; d < D; ++d) {
        const double a = sa[d * 64 + il];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const double df = a - sb[d * 64 + (g * 4 + u) * 4 + jq];
          r2[u] = __builtin_fma(df, df, r2[u]);
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int jl = (g * 4 + u) * 4 + jq;
        double kv = sigma2 * kern_val<KT>(r2[u], tab);
        if (j0 + jl >= N || gi >= M) kv = 0.0;
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(kv, sv[jl * LDV + b * 16 + cl], acc[b], 0, 0, 0);
      }
    }
  }
  double q[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      double s = acc[b][reg] * acc[b][reg];
      for (int off = 8; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
      q[reg] += s;
    }
  if (cl == 0) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int i = i0 + w * 16 + jq + 4 * reg;
      if (i < M) part[(size_t)blockIdx.y * ldp + (size_t)i] = q[reg];
    }
  }
}

// part[i] = max(base - (the partial sums of query i over the chunks, added in ascending order), 0): the floor of predict(), NaN stays
__global__ __launch_bounds__(256) void kvar_reduce_kernel(double* __restrict__ part, int M, size_t ldp, int nchunk, double base) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= M) return;
  double q = 0.0;
  for (int c = 0; c < nchunk; ++c) q += part[(size_t)c * ldp + (size_t)i];
  const double v = base - q;
  part[i] = v < 0.0 ? 0.0 : v;
}

inline unsigned blocks_of(long n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

static_assert(ITER_VAR_CHUNK == 16 * ITER_VAR_NB, "a chunk of the variance kernel is ITER_VAR_NB MFMA blocks of 16 columns");

void launch_ltv(const double* L, long N, int p, const double* R, double* wpart, double* w, hipStream_t st) {
  const unsigned nseg = blocks_of(N, ITER_SEG);
  hipLaunchKernelGGL(ltv_kernel, dim3(blocks_of(p, 16), nseg), dim3(256), 0, st, L, (int)N, p, R, wpart);
  hipLaunchKernelGGL(ltv_reduce_kernel, dim3(blocks_of((long)p * ITER_COLS, 256)), dim3(256), 0, st, wpart, (int)nseg, p, w);
}

void launch_tri_right(const double* In, long N, int r, const double* T, int ldt, int c0, double* Out, hipStream_t st) {
  if (N < 1 || r < 1) return;
  hipLaunchKernelGGL(tri_right_kernel, dim3(blocks_of(N, 256)), dim3(256), 0, st, In, (int)N, r, T, ldt, c0, Out);
}

void launch_kvar(const double* Qs, long M, const double* Xs, long N, int D, int kt, double sigma2, const double* R, long ldr, int rank, double base,
                 double* part, hipStream_t st) {
  if (M < 1 || N < 1 || rank < 1) return;
  const unsigned nchunk = blocks_of(rank, ITER_VAR_CHUNK);
  const auto kern = kt == 0 ? kvar_kernel<0, ITER_VAR_NB> : kvar_kernel<1, ITER_VAR_NB>;
  const size_t lds = sizeof(double) * (256 + (size_t)2 * KM_ROWS * D + (size_t)KM_ROWS * (ITER_VAR_CHUNK + 1));
  prof_begin("kvar", st);
  hipLaunchKernelGGL(kern, dim3(blocks_of(M, KM_ROWS), nchunk), dim3(256), lds, st, Qs, (int)M, Xs, (int)N, D, sigma2, R, (size_t)ldr, rank, part,
                     (size_t)M);
  hipLaunchKernelGGL(kvar_reduce_kernel, dim3(blocks_of(M, 256)), dim3(256), 0, st, part, (int)M, (size_t)M, (int)nchunk, base);
  // algorithmic: every chunk generates its entries again (3 D of the distance, ~20 of the kernel function), then 2 per column of R
  prof_end("kvar", st, (double)M * (double)N * (nchunk * (3.0 * D + 20.0) + 2.0 * ITER_VAR_CHUNK * nchunk),
           8.0 * (double)blocks_of(M, KM_ROWS) * (double)N * nchunk * (D + (double)ITER_VAR_CHUNK));
}

void launch_kmatvec(const double* As, long M, const double* Bs, long N, int D, int kt, double sigma2, double nug, bool same, const double* V,
                    long ldv, int nb, double* Out, long ldo, hipStream_t st) {
  if (M < 1 || N < 1) return;
  const auto kern = kt == 0 ? (nb == 1 ? kmatvec_kernel<0, 1> : kmatvec_kernel<0, 2>) : (nb == 1 ? kmatvec_kernel<1, 1> : kmatvec_kernel<1, 2>);
  const size_t lds = sizeof(double) * (256 + (size_t)2 * KM_ROWS * D + (size_t)KM_ROWS * (16 * nb + 1));
  prof_begin("kmatvec", st);
  hipLaunchKernelGGL(kern, dim3(blocks_of(M, KM_ROWS)), dim3(256), lds, st, As, (int)M, Bs, (int)N, D, sigma2, nug, same ? 1 : 0, V, (size_t)ldv, Out,
                     (size_t)ldo);
  // algorithmic: per entry 3 D operations of the distance and ~20 of the kernel function, then 2 per right-hand side; the staged rows are
  // read once per workgroup
  prof_end("kmatvec", st, (double)M * (double)N * (3.0 * D + 20.0 + 32.0 * nb), 8.0 * (double)blocks_of(M, KM_ROWS) * (double)N * (D + 16.0 * nb));
}

void launch_pchol_init(double* diag, long N, double sigma2, int* state, hipStream_t st) {
  hipLaunchKernelGGL(pchol_init_kernel, dim3(blocks_of(std::max<long>(N, 2), 256)), dim3(256), 0, st, diag, (size_t)N, sigma2, state);
}

void launch_pchol_step(const double* Xs, long N, int D, int kt, double sigma2, int t, double* L, double* diag, int* piv, double* dmax,
                       int* state, double* pval, int* pidx, hipStream_t st) {
  const unsigned nb = blocks_of(N, 1024);
  hipLaunchKernelGGL(pchol_argmax1_kernel, dim3(nb), dim3(256), 0, st, diag, (int)N, state, pval, pidx);
  hipLaunchKernelGGL(pchol_argmax2_kernel, dim3(1), dim3(256), 0, st, pval, pidx, (int)nb, t, state, piv, dmax);
  const auto kern = kt == 0 ? pchol_column_kernel<0> : pchol_column_kernel<1>;
  hipLaunchKernelGGL(kern, dim3(blocks_of(N, 256)), dim3(256), 0, st, Xs, (int)N, D, sigma2, t, L, diag, piv, dmax, state);
}

void launch_pchol_gram(const double* L, long N, int p, double eta, double* G, hipStream_t st) {
  if (p < 1) return;
  const unsigned pt = blocks_of(p, 16);
  prof_begin("pchol_gram", st);
  hipLaunchKernelGGL(gram_kernel, dim3(pt, pt), dim3(256), 0, st, L, (int)N, p, eta, G);
  prof_end("pchol_gram", st, (double)N * p * p, 8.0 * (double)N * p * pt);
}

void launch_precond_apply(const double* L, long N, int p, const double* Ginv, double eta, const double* R, double* Z, double* wpart, double* w,
                          double* w2, hipStream_t st) {
  const unsigned nseg = blocks_of(N, ITER_SEG), ne = blocks_of((long)p * ITER_COLS, 256);
  prof_begin("precond_apply", st);
  hipLaunchKernelGGL(ltv_kernel, dim3(blocks_of(p, 16), nseg), dim3(256), 0, st, L, (int)N, p, R, wpart);
  hipLaunchKernelGGL(ltv_reduce_kernel, dim3(ne), dim3(256), 0, st, wpart, (int)nseg, p, w);
  hipLaunchKernelGGL(ginv_kernel, dim3(ne), dim3(256), 0, st, Ginv, p, w, w2);
  hipLaunchKernelGGL(precond_z_kernel, dim3(blocks_of(N, 256)), dim3(256), 0, st, L, (int)N, p, w2, eta, R, Z);
  prof_end("precond_apply", st, 4.0 * (double)N * p * ITER_COLS + 2.0 * (double)p * p * ITER_COLS, 16.0 * (double)N * p);
}

void launch_cg_dot(const double* A, const double* B, long N, double* part, hipStream_t st) {
  hipLaunchKernelGGL(cg_dot_kernel, dim3(blocks_of(N, ITER_DOT_BLOCK), ITER_COLS), dim3(256), 0, st, A, B, (int)N, part);
}

void launch_cg_scalars(int mode, const double* part, long N, double* sc, int* fl, int it, double rtol, hipStream_t st, double* lg) {
  hipLaunchKernelGGL(cg_scalars_kernel, dim3(1), dim3(64), 0, st, mode, part, (int)blocks_of(N, ITER_DOT_BLOCK), sc, fl, it, rtol, lg);
}

void launch_probes(const double* L, long N, int p, const double* g1, double root, int c_lo, int c_hi, double* Z, hipStream_t st) {
  if (c_hi <= c_lo) return;
  hipLaunchKernelGGL(probe_kernel, dim3(blocks_of(N, 256), c_hi - c_lo), dim3(256), 0, st, L, (int)N, p, g1, root, c_lo, Z);
}

void launch_kgrad_forms(const double* Xs, long N, int D, int kt, double sigma2, const double* U, const double* W, int c_lo, int c_hi, double* part,
                        double* out, hipStream_t st) {
  const unsigned nblk = blocks_of(N, KM_ROWS), nch = blocks_of(D, KGRAD_DC);
  const size_t lds = sizeof(double) * (256 + (size_t)2 * KM_ROWS * D + 2 * KM_ROWS * KG_LDP + 2 * KM_ROWS + 4 * 2 * KGRAD_DC);
  prof_begin("kgrad_forms", st);
  hipLaunchKernelGGL(kt == 0 ? kgrad_forms_kernel<0> : kgrad_forms_kernel<1>, dim3(nblk, nch), dim3(256), lds, st, Xs, (int)N, D, sigma2, U, W,
                     (size_t)N, c_lo, c_hi, part);
  hipLaunchKernelGGL(kgrad_reduce_kernel, dim3(blocks_of(2 * D, 256)), dim3(256), 0, st, part, (int)nblk, 2 * D, out);
  // algorithmic: a slice of KGRAD_DC dimensions generates r2 (3 D) and k' (~20) again; 2 per probe column for S, 6 per dimension and entry
  prof_end("kgrad_forms", st, (double)N * (double)N * (nch * (3.0 * D + 20.0 + 2.0 * (c_hi - c_lo)) + 6.0 * D),
           8.0 * (double)nblk * (double)N * nch * (D + 32.0));
}

void launch_cg_update(double* x, double* xl, double* r, const double* p, const double* q, long N, const double* sc, const int* fl, hipStream_t st) {
  hipLaunchKernelGGL(cg_update_kernel, dim3(blocks_of(N, 256), ITER_COLS), dim3(256), 0, st, x, xl, r, p, q, (int)N, sc, fl);
}

void launch_panel_add(double* x, const double* xl, long N, hipStream_t st) {
  hipLaunchKernelGGL(panel_add_kernel, dim3(blocks_of(N, 256), ITER_COLS), dim3(256), 0, st, x, xl, (int)N);
}

void launch_cg_direction(double* p, const double* z, long N, bool first, const double* sc, const int* fl, hipStream_t st) {
  hipLaunchKernelGGL(cg_direction_kernel, dim3(blocks_of(N, 256), ITER_COLS), dim3(256), 0, st, p, z, (int)N, first ? 1 : 0, sc, fl);
}

void launch_panel_sub(const double* a, const double* b, long N, double* out, hipStream_t st) {
  hipLaunchKernelGGL(panel_sub_kernel, dim3(blocks_of(N, 256), ITER_COLS), dim3(256), 0, st, a, b, (int)N, out);
}

}  // namespace mogp
