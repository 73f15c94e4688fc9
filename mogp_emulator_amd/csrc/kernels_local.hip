// The kernels of LocalGP (engine.h; the handle itself is engine_local.hip) and their launchers.
// Local approximate GP prediction (Emery 2009; Gramacy & Apley 2015): every query is predicted from the GP on its k nearest design points
// alone, at hyperparameters fitted elsewhere.  m independent k x k problems, k <= 126, and no factorisation of the whole design.
//
//   local_scale_kernel   x~ = x_d s_d for the design and for the queries, one rounded multiply per element
//   local_knn_kernel     brute-force search.  One wave per LOCAL_KNN_QW queries, four waves per workgroup; the workgroup sweeps the design in
//                        tiles of LOCAL_KNN_ROWS rows staged in LDS, every lane holds two rows of the tile against the wave's queries.  The
//                        squared distance is ((0 + t_0 t_0) + t_1 t_1) + ... with every operation rounded on its own (contraction is off in
//                        that kernel), so NumPy reproduces every bit.  A query's running best list -- 128 pairs (r2, index), sorted, two per lane
//                        in registers -- takes a candidate only when it beats the pair at position k-1; the candidate is placed by counting
//                        the pairs below it (two ballots) and shifting the rest up one lane.  The list is a function of the SET of pairs
//                        offered, the pairs are unique by their index, so ties go to the lowest index and nothing depends on the order of
//                        the sweep or on which queries share a wave.  After the first tiles an insertion is rare (~ k ln(N / k) per query).
//   local_gp_kernel      a persistent grid of 256-thread workgroups, each with its own 128 x 128 tile (and chol128_dev's pack) in global
//                        memory.  Per query: gather the neighbours' scaled rows and the query into LDS, build_tile the augmented matrix,
//                        factor_tile it once with chol128_dev, read mean and variance off two rows of the factor.  This is why k <= 126.
// The Vecchia likelihood on the same handle (its own head below): local_knn_kernel<true> -- the ordered search, a query sees earlier rows
// only --, vecchia_ll_kernel -- the same three steps per point, then the conditional log-density given its neighbours with the analytic
// gradient --, and vecchia_reduce_kernel -- their sums in an order that depends on N alone.
// This file is compiled with -mllvm -amdgpu-mfma-vgpr-form=1 like kernels_panel.hip: chol128_dev reads its MFMA results back after every MFMA.
#include <algorithm>
#include <climits>

#include "chol128_dev.h"
#include "cov_dev.h"
#include "predict_plan.h"

namespace mogp {

static_assert(LOCAL_WG_DOUBLES == (size_t)128 * 128 + PACK128_STRIDE, "scratch of one workgroup: the tile and chol128_dev's pack");
static_assert(LOCAL_MAX_K + 2 == 128, "neighbours, target row and query row fill one tile");

namespace {

constexpr int KNN_LD = LOCAL_KNN_ROWS + 1;      // row stride of a staged dimension (odd: the transposing stores spread over the banks)

__global__ __launch_bounds__(256) void local_scale_kernel(const double* __restrict__ x, size_t total, int D, const double* __restrict__ s,
                                                          double* __restrict__ out) {
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) out[e] = x[e] * s[e % (size_t)D];
}

__device__ __forceinline__ bool pair_less(double a, int ai, double b, int bi) { return a < b || (a == b && ai < bi); }

// ORD (the Vecchia search, below): the queries ARE the design rows (Qs = Xs, mc = N) and query q is offered the rows < q alone; positions
// behind its min(q, k) neighbours are -1 and no radius is written.  The workgroup stops at the largest limit of its own queries.
template <bool ORD>
__global__ __launch_bounds__(256) void local_knn_kernel(const double* __restrict__ Xs, int N, int D, const double* __restrict__ Qs, int mc, int k,
                                                        int* __restrict__ nbr, double* __restrict__ radius) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) double sm[];      // D x KNN_LD: sm[d * KNN_LD + row of the tile]
  constexpr int QW = LOCAL_KNN_QW;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int q0 = blockIdx.x * LOCAL_KNN_QUERIES + w * QW;
  // the wave's queries: wave-uniform pointers (behind the end of the launch the last query again: computed, not stored)
  const double* qp[QW];
#pragma unroll
  for (int a = 0; a < QW; ++a) qp[a] = Qs + (size_t)min(q0 + a, mc - 1) * D;
  // the best list of every query: position lane in (r0, i0), position 64 + lane in (r1, i1)
  double r0[QW], r1[QW], thr[QW];
  int i0[QW], i1[QW], thi[QW];
  const double inf = __longlong_as_double(0x7FF0000000000000ll);
#pragma unroll
  for (int a = 0; a < QW; ++a) {
    r0[a] = r1[a] = thr[a] = inf;
    i0[a] = i1[a] = thi[a] = INT_MAX;
  }
  const int kl = (k - 1) & 63, kh = (k - 1) >> 6;
  int lim[QW];                                                     // rows below lim[a] are offered to query a
#pragma unroll
  for (int a = 0; a < QW; ++a) lim[a] = ORD ? min(q0 + a, mc - 1) : N;
  const int jend = ORD ? min((int)blockIdx.x * LOCAL_KNN_QUERIES + LOCAL_KNN_QUERIES - 1, mc - 1) : N;
  for (int j0 = 0; j0 < jend; j0 += LOCAL_KNN_ROWS) {
    __syncthreads();                                               // the previous tile has been read
    {
      const int cnt = LOCAL_KNN_ROWS * D;
      const int avail = min(LOCAL_KNN_ROWS, N - j0) * D;
      const double* src = Xs + (size_t)j0 * D;
      for (int e = threadIdx.x; e < cnt; e += 256) {
        const int r = e / D, d = e - r * D;
        sm[d * KNN_LD + r] = (e < avail) ? src[e] : 0.0;
      }
    }
    __syncthreads();
    double acc[2][QW];
#pragma unroll
    for (int a = 0; a < QW; ++a) acc[0][a] = acc[1][a] = 0.0;
    for (int d = 0; d < D; ++d) {
      const double x0 = sm[d * KNN_LD + lane], x1 = sm[d * KNN_LD + 64 + lane];
#pragma unroll
      for (int a = 0; a < QW; ++a) {
        const double qd = qp[a][d];
        const double t0 = x0 - qd, t1 = x1 - qd;
        const double s0 = t0 * t0, s1 = t1 * t1;                   // rounded on their own: no FMA (see the head of the file)
        acc[0][a] = acc[0][a] + s0;
        acc[1][a] = acc[1][a] + s1;
      }
    }
#pragma unroll
    for (int a = 0; a < QW; ++a) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int row = j0 + 64 * h + lane;
        const bool cand = row < lim[a] && pair_less(acc[h][a], row, thr[a], thi[a]);
        unsigned long long todo = __ballot(cand);
        while (todo) {
          const int src = __builtin_ctzll(todo);
          todo &= todo - 1;
          const double cr = readlane_f64(acc[h][a], src);
          const int ci = j0 + 64 * h + src;
          if (!pair_less(cr, ci, thr[a], thi[a])) continue;        // the bar has moved since the ballot (wave-uniform)
          // the list is sorted: the pairs below the candidate are a prefix, and the candidate beats position k-1, so pos <= k-1
          const int pos = __popcll(__ballot(pair_less(r0[a], i0[a], cr, ci))) + __popcll(__ballot(pair_less(r1[a], i1[a], cr, ci)));
          double u0 = __shfl_up(r0[a], 1, 64), u1 = __shfl_up(r1[a], 1, 64);
          int v0 = __shfl_up(i0[a], 1, 64), v1 = __shfl_up(i1[a], 1, 64);
          const double e63 = readlane_f64(r0[a], 63);
          const int f63 = __builtin_amdgcn_readlane(i0[a], 63);
          if (lane == 0) {                                         // position 64 takes position 63 (position 0 is never shifted into)
            u1 = e63;
            v1 = f63;
          }
          const int p0 = lane, p1 = 64 + lane;
          r0[a] = p0 < pos ? r0[a] : (p0 == pos ? cr : u0);
          i0[a] = p0 < pos ? i0[a] : (p0 == pos ? ci : v0);
          r1[a] = p1 < pos ? r1[a] : (p1 == pos ? cr : u1);
          i1[a] = p1 < pos ? i1[a] : (p1 == pos ? ci : v1);
          thr[a] = kh ? readlane_f64(r1[a], kl) : readlane_f64(r0[a], kl);
          thi[a] = kh ? __builtin_amdgcn_readlane(i1[a], kl) : __builtin_amdgcn_readlane(i0[a], kl);
        }
      }
    }
  }
#pragma unroll
  for (int a = 0; a < QW; ++a) {
    const int q = q0 + a;
    if (q < mc) {
      int* out = nbr + (size_t)q * k;
      if (lane < k) out[lane] = (!ORD || lane < q) ? i0[a] : -1;
      if (64 + lane < k) out[64 + lane] = (!ORD || 64 + lane < q) ? i1[a] : -1;
      if (!ORD && lane == 0) radius[q] = thr[a];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// What local_gp_kernel and vecchia_ll_kernel share: one problem is one 128 x 128 tile.  sm is the workgroup's dynamic LDS, carved by
// o = LocalLds(D, grad) (predict_plan.h); A its tile in global memory with chol128_dev's pack behind it.
// ---------------------------------------------------------------------------------------------------------------------------------------
static_assert(LOCAL_CHOL_LDS_DOUBLES == C128_LDS_DOUBLES, "LocalLds starts behind chol128_dev's own LDS");

// Rows 0 .. kn-1 of pts are the design rows nq[0 .. kn-1] (an index outside the design reads row 0), row kn is `last`; yv their targets
// and, with last_y, that of the last row.  Clears chol128_dev's status word and ends with a barrier.
__device__ __forceinline__ void gather(double* sm, const LocalLds& o, const double* Xs, const double* Y, int N, int D, const int* nq, int kn,
                                       const double* last, const double* last_y) {
  const int t = threadIdx.x, DP = o.ld;
  double *yv = sm + o.yv, *pts = sm + o.pts;
  for (int e = t; e < (kn + 1) * D; e += 256) {
    const int r = e / D, d = e - r * D;
    const double* src = last;
    if (r < kn) {
      const int j = nq[r];
      src = Xs + (size_t)((unsigned)j < (unsigned)N ? j : 0) * D;
    }
    pts[r * DP + d] = src[d];
  }
  if (t < kn) {
    const int j = nq[t];
    yv[t] = Y[(unsigned)j < (unsigned)N ? j : 0];
  } else if (last_y && t == kn) {
    yv[t] = *last_y;
  }
  if (t == 0) *reinterpret_cast<int*>(sm + o.info) = 0;
  __syncthreads();                           // (also: the previous problem's factor and its sums in LDS have been read)
}

// The lower triangle of the tile from the gathered points.  Rows i < nm: the matrix, sigma2 k(r2) of rows i and j of pts off the diagonal and
// sigma2 + diag_add on it (GRAD: G_ij = sigma2 k'(r2) beside it).  Row nm: the targets yv, PAD_BIG on the diagonal.  CROSS: row nm + 1 =
// sigma2 k(r2) of row nm of pts against the matrix rows, 0 against the target row, PAD_BIG on the diagonal.  Identity beyond these nr rows.
template <int KT, bool CROSS, bool GRAD>
__device__ __forceinline__ void build_tile(const double* sm, const LocalLds& o, int D, int nm, double sigma2, double diag_add, double* A,
                                           double* G) {
  const int t = threadIdx.x, DP = o.ld;
  const double *tab = sm + o.tab, *yv = sm + o.yv, *pts = sm + o.pts;
  const int nr = nm + (CROSS ? 2 : 1);
  // rows p and nr-1-p together (nr + 1 entries): every lane has an entry
  const int L = nr + 1, np = (nr + 1) / 2;
  for (int e = t; e < np * L; e += 256) {
    const int p = e / L, c = e - p * L;
    int i, j;
    if (c <= p) {
      i = p;
      j = c;
    } else {
      i = nr - 1 - p;
      j = c - p - 1;
      if (i == p) continue;                  // the middle row of an odd count is its own partner
    }
    double val;
    if (j < nm && i != nm) {
      if (i == j) {
        val = sigma2 + diag_add;
      } else {
        const double* a = pts + (CROSS && i == nm + 1 ? nm : i) * DP;
        const double* b = pts + j * DP;
        double r2 = 0.0;
        for (int d = 0; d < D; ++d) {
          const double df = a[d] - b[d];
          r2 = __builtin_fma(df, df, r2);
        }
        val = sigma2 * kern_val<KT>(r2, tab);
        if (GRAD) G[i * 128 + j] = sigma2 * kern_dr2<KT>(r2, tab);      // (the exponential of kern_val: one for both)
      }
    } else if (!CROSS || i == nm) {
      val = (j < nm) ? yv[j] : PAD_BIG;
    } else {
      val = (j == nm) ? 0.0 : PAD_BIG;       // 0 between the two right-hand-side rows
    }
    A[i * 128 + j] = val;
  }
  for (int e = t; e < (128 - nr) * 128; e += 256) {
    const int i = nr + (e >> 7), j = e & 127;
    if (j <= i) A[i * 128 + j] = (i == j) ? 1.0 : 0.0;
  }
}

__device__ __forceinline__ void factor_tile(double* sm, const LocalLds& o, double* A) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();                           // the tile is complete: chol128_dev's waves read what other waves stored
  chol128_dev(A, 128, A + 128 * 128, reinterpret_cast<int*>(sm + o.info), 0, sm);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();                           // the factor's rows (and the info word) are visible to every wave
}

// Prediction: nm = k matrix rows, the query is row k of pts and the CROSS row of the tile.  After the factorisation row k is (L^-1 y)^T and
// row k+1 v^T = (L^-1 k*)^T: mean = <row k, row k+1>, variance = sigma^2 - <v, v>, both summed by wave 0 in a fixed order.
template <int KT>
__global__ __launch_bounds__(256) void local_gp_kernel(const double* __restrict__ Xs, const double* __restrict__ Y, int N, int D,
                                                       const double* __restrict__ Qs, int mc, int k, const int* __restrict__ nbr, double sigma2,
                                                       double diag_add, double var_add, double* __restrict__ scratch, double* __restrict__ mean,
                                                       double* __restrict__ var, int* __restrict__ ok) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const LocalLds o(D, false);
  const int& info = *reinterpret_cast<int*>(sm + o.info);
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  double* A = scratch + (size_t)blockIdx.x * LOCAL_WG_DOUBLES;
  stage_exp_tab(sm + o.tab);
  for (int q = blockIdx.x; q < mc; q += gridDim.x) {
    gather(sm, o, Xs, Y, N, D, nbr + (size_t)q * k, k, Qs + (size_t)q * D, nullptr);
    build_tile<KT, true, false>(sm, o, D, k, sigma2, diag_add, A, nullptr);
    factor_tile(sm, o, A);
    if (w == 0) {
      const double* ry = A + k * 128;
      const double* rv = ry + 128;
      const bool in0 = lane < k, in1 = 64 + lane < k;
      const double a0 = in0 ? ry[lane] : 0.0, b0 = in0 ? rv[lane] : 0.0;
      const double a1 = in1 ? ry[64 + lane] : 0.0, b1 = in1 ? rv[64 + lane] : 0.0;
      double mu = __builtin_fma(a1, b1, a0 * b0), vv = __builtin_fma(b1, b1, b0 * b0);
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        mu += __shfl_xor(mu, off, 64);
        vv += __shfl_xor(vv, off, 64);
      }
      if (lane == 0) {
        const bool good = info == 0;
        const double nan = __longlong_as_double(0x7FF8000000000000ll);
        double s2 = (sigma2 - vv) + var_add;
        s2 = s2 < 0.0 ? 0.0 : s2;            // the floor of predict(): clipped at zero, NaN stays
        mean[q] = good ? mu : nan;
        var[q] = good ? s2 : nan;
        ok[q] = good ? 1 : 0;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// Vecchia likelihood (Vecchia 1988; Datta et al. 2016; Katzfuss et al. 2020): log p(y) ~ sum_t log p(y_t | y_c(t)), c(t) the min(t, k)
// nearest rows BEFORE t (local_knn_kernel<true>).  One persistent workgroup per point t, kt = min(t, k), n = kt + 1:
//   rows 0 .. kt-1 of the tile the neighbours, row kt the point itself (the matrix proper, A = sigma^2 k + (nugget + jitter) I, n x n), row n
//   the targets of those n points with PAD_BIG on the diagonal, identity beyond: n + 1 <= 128 rows carry the problem.
// After chol128_dev, with e = kt the last row of the matrix proper: row n holds z^T = (L^-1 y)^T and
//   l_t = -log L_ee - z_e^2 / 2 - log(2 pi) / 2.
// GRAD: wave 0 solves L^T w = e / L_ee (w = A^-1 e) and wave 1 L^T alpha = z (alpha = A^-1 y), both right-looking -- lane j keeps entry j
// and 64 + j of the right-hand side, step i = n-1 .. 0 broadcasts u_i = b_i / L_ii with one v_readlane and subtracts u_i * (row i of L):
// no reduction across lanes; the rows of L are requested eight steps ahead.  G_ij = sigma^2 k'(r2_ij), written beside the tile while it is built, and the
// gathered points still in LDS then give, per dimension d, a_d = w^T A_d w and b_d = w^T A_d alpha with (A_d)_ij = G_ij (x~_id - x~_jd)^2:
// thread (c, d) owns dimension d and the rows i = c, c + C, ... (C = 256 / D), partial sums meet in LDS and are added in the order of c.
// With w_e = 1 / L_ee^2, rho = w^T y = z_e / L_ee and m = rho / w_e:
//   dl_t/dtheta_p = (rho b_p - a_p / 2) / w_e - m^2 a_p / 2
//   log sigma^2:  a = w_e - (nugget + jitter) w^T w,  b = rho - (nugget + jitter) w^T alpha;    log nugget:  a = nugget w^T w,  b = nugget w^T alpha.
// Results go to out (cols, Ntot) column-major: column 0 the term, 1 .. D the dimensions, D + 1 log sigma^2, D + 2 log nugget; NaN and ok = 0
// where the matrix is not positive definite.  Nothing depends on the grid or on which workgroup takes a point.
constexpr double HALF_LOG_2PI = 0.91893853320467274178;
template <int KT, bool GRAD>
__global__ __launch_bounds__(256) void vecchia_ll_kernel(const double* __restrict__ Xs, const double* __restrict__ Y, int N, int D, int p0, int mc,
                                                         int k, const int* __restrict__ nbr, double sigma2, double diag_add, double nugget,
                                                         double* __restrict__ scratch, double* __restrict__ out, int* __restrict__ ok) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const LocalLds o(D, GRAD);
  double *wv = sm + o.wv, *av = sm + o.av, *reda = sm + o.reda, *redb = sm + o.redb;      // GRAD: w, alpha, the partial sums of a_d and b_d
  const double* pts = sm + o.pts;
  const int DP = o.ld;
  const int& info = *reinterpret_cast<int*>(sm + o.info);
  const int t = threadIdx.x, lane = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  double* A = scratch + (size_t)blockIdx.x * (GRAD ? VECCHIA_WG_DOUBLES : LOCAL_WG_DOUBLES);
  double* G = A + LOCAL_WG_DOUBLES;          // GRAD only: sigma^2 k'(r2_ij), j < i < n
  const double nan = __longlong_as_double(0x7FF8000000000000ll);
  stage_exp_tab(sm + o.tab);
  for (int q = blockIdx.x; q < mc; q += gridDim.x) {
    const int pt = p0 + q;                   // the point; its neighbours are rows < pt
    const int kt = min(pt, k), n = kt + 1;
    gather(sm, o, Xs, Y, N, D, nbr + (size_t)pt * k, kt, Xs + (size_t)pt * D, Y + pt);
    build_tile<KT, false, GRAD>(sm, o, D, n, sigma2, diag_add, A, G);
    factor_tile(sm, o, A);
    double Lee = 1.0, ze = 0.0;              // wave 0 alone needs them (and the info word: thread 0 clears it for the next point)
    if (w == 0) {
      Lee = A[kt * 128 + kt];
      ze = A[n * 128 + kt];
    }
    const double ell = __builtin_fma(-0.5 * ze, ze, -log(Lee)) - HALF_LOG_2PI;
    const bool good = info == 0 && ell == ell && fabs(ell) <= 1.7e308;
    if (t == 0) {
      out[pt] = good ? ell : nan;
      ok[pt] = good ? 1 : 0;
    }
    if (GRAD) {
      if (w < 2) {
        double b0, b1;
        if (w == 0) {
          const double r = 1.0 / Lee;
          b0 = lane == kt ? r : 0.0;
          b1 = 64 + lane == kt ? r : 0.0;
        } else {
          b0 = lane < n ? A[n * 128 + lane] : 0.0;
          b1 = 64 + lane < n ? A[n * 128 + 64 + lane] : 0.0;
        }
        const double ri0 = lane < n ? 1.0 / A[lane * 129] : 0.0;
        const double ri1 = 64 + lane < n ? 1.0 / A[(64 + lane) * 129] : 0.0;
        for (int ib = n - 1; ib >= 0; ib -= 8) {
          double l0[8], l1[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const int i = ib - u;
            l0[u] = (i >= 0 && lane < i) ? A[i * 128 + lane] : 0.0;
            l1[u] = (i >= 0 && 64 + lane < i) ? A[i * 128 + 64 + lane] : 0.0;
          }
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const int i = ib - u;
            if (i >= 0) {                    // (wave-uniform)
              const double s0 = b0 * ri0, s1 = b1 * ri1;
              const double ui = i >= 64 ? readlane_f64(s1, i - 64) : readlane_f64(s0, i);
              b0 = lane == i ? ui : __builtin_fma(-l0[u], ui, b0);
              b1 = 64 + lane == i ? ui : __builtin_fma(-l1[u], ui, b1);
            }
          }
        }
        double* dst = w == 0 ? wv : av;      // entries >= n are exact zeros
        dst[lane] = b0;
        dst[64 + lane] = b1;
      }
      __syncthreads();
      {
        const int C = 256 / D;
        if (t < C * D) {
          const int c = t / D, d = t - c * D;
          double sa = 0.0, sb = 0.0;
          for (int i = c; i < n; i += C) {
            const double xi = pts[i * DP + d];
            const double* Gi = G + i * 128;
            double ta = 0.0, tb = 0.0;
#pragma unroll 8
            for (int j = 0; j < i; ++j) {
              const double df = xi - pts[j * DP + d];
              const double cc = df * df * Gi[j];
              ta = __builtin_fma(cc, wv[j], ta);
              tb = __builtin_fma(cc, av[j], tb);
            }
            sa = __builtin_fma(wv[i], ta, sa);
            sb = __builtin_fma(wv[i], tb, __builtin_fma(av[i], ta, sb));
          }
          reda[t] = sa;
          redb[t] = sb;
        }
      }
      __syncthreads();
      if (w == 0) {
        const double w0 = wv[lane], w1 = wv[64 + lane], a0 = av[lane], a1 = av[64 + lane];
        double ww = __builtin_fma(w1, w1, w0 * w0), wa = __builtin_fma(w1, a1, w0 * a0);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
          ww += __shfl_xor(ww, off, 64);
          wa += __shfl_xor(wa, off, 64);
        }
        const double iw = Lee * Lee;         // 1 / w_e
        const double we = 1.0 / iw, rho = ze / Lee, m = ze * Lee;
        const int C = 256 / D;
        const size_t Nt = (size_t)N;
        for (int d = lane; d < D + 2; d += 64) {
          double a, b;
          if (d < D) {
            double sa = 0.0, sb = 0.0;
            for (int c = 0; c < C; ++c) {
              sa += reda[c * D + d];
              sb += redb[c * D + d];
            }
            a = 2.0 * sa;
            b = sb;
          } else if (d == D) {
            a = __builtin_fma(-diag_add, ww, we);
            b = __builtin_fma(-diag_add, wa, rho);
          } else {
            a = nugget * ww;
            b = nugget * wa;
          }
          const double g = __builtin_fma(iw, __builtin_fma(rho, b, -0.5 * a), -0.5 * (m * m) * a);
          out[(size_t)(1 + d) * Nt + pt] = good ? g : nan;
        }
      }
      __syncthreads();                       // wave 0 has read the sums before the next point's are written
    }
  }
}

// columns of `in` (cols, n) summed in blocks of VECCHIA_REDUCE_BLOCK entries: out (cols, gridDim.x).  Thread i of a block adds its four
// entries i, 256 + i, ... in that order, a binary tree over the 256 threads follows: the order is a function of n alone.
__global__ __launch_bounds__(256) void vecchia_reduce_kernel(const double* __restrict__ in, size_t n, double* __restrict__ out) {
  __shared__ double s[256];
  const int t = threadIdx.x;
  const double* src = in + (size_t)blockIdx.y * n;
  const size_t base = (size_t)blockIdx.x * VECCHIA_REDUCE_BLOCK;
  double acc = 0.0;
#pragma unroll
  for (int u = 0; u < (int)(VECCHIA_REDUCE_BLOCK / 256); ++u) {
    const size_t i = base + (size_t)u * 256 + t;
    acc += i < n ? src[i] : 0.0;
  }
  s[t] = acc;
  for (int off = 128; off > 0; off >>= 1) {
    __syncthreads();
    if (t < off) s[t] += s[t + off];
  }
  if (t == 0) out[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = s[0];
}

}  // namespace
// one body of the two searches; ORD: half of the N x N sweep, workgroup g stops at the largest limit of its own queries
template <bool ORD>
static void launch_knn(const double* Xs, long N, int D, const double* Qs, int mc, int k, int* nbr, double* radius, hipStream_t st) {
  const char* tag = ORD ? "vecchia_knn" : "local_knn";
  const int groups = (mc + LOCAL_KNN_QUERIES - 1) / LOCAL_KNN_QUERIES;
  prof_begin(tag, st);
  hipLaunchKernelGGL(local_knn_kernel<ORD>, dim3(groups), dim3(256), sizeof(double) * (size_t)D * KNN_LD, st, Xs, (int)N, D, Qs, mc, k, nbr, radius);
  // algorithmic: a subtraction, a product and an addition per (query, design point, dimension); the design is read once per workgroup
  prof_end(tag, st, (ORD ? 1.5 : 3.0) * (double)mc * (double)N * D, (ORD ? 4.0 : 8.0) * (double)N * D * groups);
}
void launch_local_knn(const double* Xs, long N, int D, const double* Qs, int mc, int k, int* nbr, double* radius, hipStream_t st) {
  launch_knn<false>(Xs, N, D, Qs, mc, k, nbr, radius, st);
}
void launch_vecchia_knn(const double* Xs, long N, int D, int k, int* nbr, hipStream_t st) {
  launch_knn<true>(Xs, N, D, Xs, (int)N, k, nbr, nullptr, st);
}

// the instantiation is chosen as a pointer; one launch follows
void launch_local_gp(const double* Xs, const double* Y, long N, int D, const double* Qs, int mc, int k, const int* nbr, int kt, double sigma2,
                     double diag_add, double var_add, double* scratch, int grid, double* mean, double* var, int* ok, hipStream_t st) {
  const auto kern = kt == 0 ? local_gp_kernel<0> : local_gp_kernel<1>;
  prof_begin("local_gp", st);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(256), local_lds_bytes(D, false), st, Xs, Y, (int)N, D, Qs, mc, k, nbr, sigma2, diag_add, var_add, scratch,
                     mean, var, ok);
  // the factorisation of one whole tile per query (what chol128_dev executes whatever k is); the tile and the pack written once per query
  prof_end("local_gp", st, (double)mc * 128.0 * 128.0 * 128.0 / 3.0, (double)mc * 8.0 * (double)LOCAL_WG_DOUBLES);
}

void launch_vecchia_ll(const double* Xs, const double* Y, long N, int D, long p0, int mc, int k, const int* nbr, int kt, double sigma2,
                       double diag_add, double nugget, bool grad, double* scratch, int grid, double* out, int* ok, hipStream_t st) {
  const auto kern = kt == 0 ? (grad ? vecchia_ll_kernel<0, true> : vecchia_ll_kernel<0, false>)
                            : (grad ? vecchia_ll_kernel<1, true> : vecchia_ll_kernel<1, false>);
  const char* tag = grad ? "vecchia_ll_grad" : "vecchia_ll";
  prof_begin(tag, st);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(256), local_lds_bytes(D, grad), st, Xs, Y, (int)N, D, (int)p0, mc, k, nbr, sigma2, diag_add, nugget,
                     scratch, out, ok);
  prof_end(tag, st, (double)mc * 128.0 * 128.0 * 128.0 / 3.0, (double)mc * 8.0 * (double)(grad ? VECCHIA_WG_DOUBLES : LOCAL_WG_DOUBLES));
}

// sums of the columns of in (cols, n) into in/out buffers a, b (each cols * ceil(n / VECCHIA_REDUCE_BLOCK) doubles); returns the buffer
// whose first `cols` entries are the sums
double* launch_vecchia_reduce(const double* in, long n, int cols, double* a, double* b, hipStream_t st) {
  const double* src = in;
  double* dst = a;
  size_t cnt = (size_t)n;
  for (;;) {
    const size_t nb = (cnt + VECCHIA_REDUCE_BLOCK - 1) / VECCHIA_REDUCE_BLOCK;
    hipLaunchKernelGGL(vecchia_reduce_kernel, dim3((unsigned)nb, (unsigned)cols), dim3(256), 0, st, src, cnt, dst);
    if (nb == 1) return dst;
    src = dst;
    dst = dst == a ? b : a;
    cnt = nb;
  }
}

void launch_local_scale(const double* x, long rows, int D, const double* s, double* out, hipStream_t st) {
  const size_t total = (size_t)rows * D;
  if (total == 0) return;
  const unsigned grid = (unsigned)std::min<size_t>((total + 255) / 256, 8192);
  hipLaunchKernelGGL(local_scale_kernel, dim3(grid), dim3(256), 0, st, x, total, D, s, out);
}


}  // namespace mogp
