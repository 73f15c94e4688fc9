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
//                        memory.  Per query: the neighbours' scaled rows and the query are gathered into LDS, the lower triangle of the
//                        augmented matrix is built -- K + (nugget + jitter) I in rows < k, the residual targets in row k, sigma^2 k(x*, .)
//                        in row k+1, PAD_BIG on the diagonal of those two and 0 between them, identity beyond -- and chol128_dev factors it
//                        once.  Row k is then (L^-1 y)^T and row k+1 v^T = (L^-1 k*)^T: mean = <row k, row k+1>, variance = sigma^2 -
//                        <v, v>, both summed by one wave in a fixed order.  This is why k <= 126.
// The Vecchia likelihood on the same handle (its own head below): local_knn_kernel<true> -- the ordered search, a query sees earlier rows
// only --, vecchia_ll_kernel -- the conditional log-density of every point given its neighbours, with the analytic gradient --, and
// vecchia_reduce_kernel -- their sums in an order that depends on N alone.
// This file is compiled with -mllvm -amdgpu-mfma-vgpr-form=1 like kernels_panel.hip: chol128_dev reads its MFMA results back after every MFMA.
#include <algorithm>
#include <climits>
#include <cmath>
#include <stdexcept>
#include <string>

#include "chol128_dev.h"
#include "cov_dev.h"
#include "engine.h"
#include "predict_plan.h"

namespace mogp {

#define HIPCK(x) hip_check((x), #x)

static_assert(LOCAL_WG_DOUBLES == (size_t)128 * 128 + PACK128_STRIDE, "scratch of one workgroup: the tile and chol128_dev's pack");
static_assert(LOCAL_MAX_K + 2 == 128, "neighbours, target row and query row fill one tile");

namespace {

constexpr int KNN_LD = LOCAL_KNN_ROWS + 1;      // row stride of a staged dimension (odd: the transposing stores spread over the banks)
constexpr long LOCAL_MAX_N = 2147483647L - 256; // a tile's row index j0 + 127 stays an int

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

// LDS of local_gp_kernel in doubles: chol128_dev's own, the exponential's table, the targets of the neighbours, the gathered points, the status word
__host__ __device__ constexpr int local_pts_ld(int D) { return D | 1; }        // odd row stride: rows a lane apart fall on different banks
size_t local_gp_lds_bytes(int D) { return sizeof(double) * ((size_t)C128_LDS_DOUBLES + 256 + 128 + (size_t)128 * local_pts_ld(D) + 2); }

template <int KT>
__global__ __launch_bounds__(256) void local_gp_kernel(const double* __restrict__ Xs, const double* __restrict__ Y, int N, int D,
                                                       const double* __restrict__ Qs, int mc, int k, const int* __restrict__ nbr, double sigma2,
                                                       double diag_add, double var_add, double* __restrict__ scratch, double* __restrict__ mean,
                                                       double* __restrict__ var, int* __restrict__ ok) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  double* lds = sm;                          // chol128_dev
  double* tab = sm + C128_LDS_DOUBLES;       // 2^(j/256)
  double* yv = tab + 256;                    // residual targets of the neighbours
  double* pts = yv + 128;                    // rows 0 .. k-1 the neighbours, row k the query, row stride DP
  const int DP = local_pts_ld(D);
  int& info = *reinterpret_cast<int*>(pts + 128 * DP);      // chol128_dev's status word (in the dynamic region: a static one would misalign it)
  const int t = threadIdx.x, lane = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  double* A = scratch + (size_t)blockIdx.x * LOCAL_WG_DOUBLES;
  double* pk = A + 128 * 128;
  const int nr = k + 2;                      // rows that carry the problem
  stage_exp_tab(tab);
  for (int q = blockIdx.x; q < mc; q += gridDim.x) {
    const int* nq = nbr + (size_t)q * k;
    for (int e = t; e < (k + 1) * D; e += 256) {
      const int r = e / D, d = e - r * D;
      const double* src;
      if (r < k) {
        const int j = nq[r];
        src = Xs + (size_t)((unsigned)j < (unsigned)N ? j : 0) * D;
      } else {
        src = Qs + (size_t)q * D;
      }
      pts[r * DP + d] = src[d];
    }
    if (t < k) {
      const int j = nq[t];
      yv[t] = Y[(unsigned)j < (unsigned)N ? j : 0];
    }
    if (t == 0) info = 0;
    __syncthreads();                         // (also: wave 0 has read rows k, k+1 of the previous query's factor)
    // rows i < nr of the lower triangle, rows p and nr-1-p together (nr + 1 entries): every lane has an entry
    {
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
          if (i == p) continue;              // the middle row of an odd count is its own partner
        }
        double val;
        if (j < k && i != k) {
          if (i == j) {
            val = sigma2 + diag_add;
          } else {
            const double* a = pts + (i == k + 1 ? k : i) * DP;
            const double* b = pts + j * DP;
            double r2 = 0.0;
            for (int d = 0; d < D; ++d) {
              const double df = a[d] - b[d];
              r2 = __builtin_fma(df, df, r2);
            }
            val = sigma2 * kern_val<KT>(r2, tab);
          }
        } else if (i == k) {
          val = (j < k) ? yv[j] : PAD_BIG;
        } else {
          val = (j == k) ? 0.0 : PAD_BIG;    // i == k+1: 0 between the two right-hand-side rows
        }
        A[i * 128 + j] = val;
      }
      for (int e = t; e < (128 - nr) * 128; e += 256) {
        const int i = nr + (e >> 7), j = e & 127;
        if (j <= i) A[i * 128 + j] = (i == j) ? 1.0 : 0.0;
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                         // the tile is complete: chol128_dev's waves read what other waves stored
    chol128_dev(A, 128, pk, &info, 0, lds);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                         // the factor's rows (and the info word) are visible to wave 0
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
size_t vecchia_lds_bytes(int D, bool grad) {
  return sizeof(double) * ((size_t)C128_LDS_DOUBLES + 256 + 128 + (grad ? 2 * 128 + 2 * 256 : 0) + (size_t)128 * local_pts_ld(D) + 2);
}

// (k(r2), dk/dr2) with one exponential
template <int KT>
__device__ __forceinline__ void kern_val_dr2(double r2, const double* tab, double& kv, double& dk) {
  if (KT == 0) {
    kv = lean_exp_neg<true>(r2, tab);
    dk = -0.5 * kv;
  } else {
    const double s = sqrt(5.0 * r2);
    const double e = lean_exp_neg<false>(s, tab);
    kv = (1.0 + s + (5.0 / 3.0) * r2) * e;
    dk = -(5.0 / 6.0) * (1.0 + s) * e;
  }
}

template <int KT, bool GRAD>
__global__ __launch_bounds__(256) void vecchia_ll_kernel(const double* __restrict__ Xs, const double* __restrict__ Y, int N, int D, int p0, int mc,
                                                         int k, const int* __restrict__ nbr, double sigma2, double diag_add, double nugget,
                                                         double* __restrict__ scratch, double* __restrict__ out, int* __restrict__ ok) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  double* lds = sm;                          // chol128_dev
  double* tab = sm + C128_LDS_DOUBLES;       // 2^(j/256)
  double* yv = tab + 256;                    // targets of the neighbours and of the point
  double* wv = yv + 128;                     // GRAD: w, alpha, the partial sums of a_d and b_d
  double* av = wv + (GRAD ? 128 : 0);
  double* reda = av + (GRAD ? 128 : 0);
  double* redb = reda + (GRAD ? 256 : 0);
  double* pts = redb + (GRAD ? 256 : 0);     // rows 0 .. kt-1 the neighbours, row kt the point, row stride DP
  const int DP = local_pts_ld(D);
  int& info = *reinterpret_cast<int*>(pts + 128 * DP);
  const int t = threadIdx.x, lane = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  double* A = scratch + (size_t)blockIdx.x * (GRAD ? VECCHIA_WG_DOUBLES : LOCAL_WG_DOUBLES);
  double* pk = A + 128 * 128;
  double* G = A + LOCAL_WG_DOUBLES;          // GRAD only: sigma^2 k'(r2_ij), j < i < n
  const double nan = __longlong_as_double(0x7FF8000000000000ll);
  stage_exp_tab(tab);
  for (int q = blockIdx.x; q < mc; q += gridDim.x) {
    const int pt = p0 + q;                   // the point; its neighbours are rows < pt
    const int kt = min(pt, k), n = kt + 1, nr = n + 1;
    const int* nq = nbr + (size_t)pt * k;
    for (int e = t; e < n * D; e += 256) {
      const int r = e / D, d = e - r * D;
      int j = pt;
      if (r < kt) {
        j = nq[r];
        j = (unsigned)j < (unsigned)N ? j : 0;
      }
      pts[r * DP + d] = Xs[(size_t)j * D + d];
    }
    if (t < n) {
      int j = pt;
      if (t < kt) {
        j = nq[t];
        j = (unsigned)j < (unsigned)N ? j : 0;
      }
      yv[t] = Y[j];
    }
    if (t == 0) info = 0;
    __syncthreads();
    // rows i < nr of the lower triangle, rows p and nr-1-p together (as local_gp_kernel)
    {
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
          if (i == p) continue;
        }
        double val;
        if (i < n) {
          if (i == j) {
            val = sigma2 + diag_add;
          } else {
            const double* a = pts + i * DP;
            const double* b = pts + j * DP;
            double r2 = 0.0;
            for (int d = 0; d < D; ++d) {
              const double df = a[d] - b[d];
              r2 = __builtin_fma(df, df, r2);
            }
            double kv, dk;
            kern_val_dr2<KT>(r2, tab, kv, dk);
            val = sigma2 * kv;
            if (GRAD) G[i * 128 + j] = sigma2 * dk;
          }
        } else {
          val = (j < n) ? yv[j] : PAD_BIG;   // i == n: the targets ride along
        }
        A[i * 128 + j] = val;
      }
      for (int e = t; e < (128 - nr) * 128; e += 256) {
        const int i = nr + (e >> 7), j = e & 127;
        if (j <= i) A[i * 128 + j] = (i == j) ? 1.0 : 0.0;
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    chol128_dev(A, 128, pk, &info, 0, lds);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                         // the factor (and the info word) are visible to every wave
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

void launch_vecchia_knn(const double* Xs, long N, int D, int k, int* nbr, hipStream_t st) {
  const size_t lds = sizeof(double) * (size_t)D * KNN_LD;
  const int mc = (int)N;
  prof_begin("vecchia_knn", st);
  hipLaunchKernelGGL(local_knn_kernel<true>, dim3((mc + LOCAL_KNN_QUERIES - 1) / LOCAL_KNN_QUERIES), dim3(256), lds, st, Xs, mc, D, Xs, mc, k, nbr,
                     (double*)nullptr);
  // half of the N x N sweep: workgroup g stops at the largest limit of its own queries
  prof_end("vecchia_knn", st, 1.5 * (double)N * (double)N * D, 4.0 * (double)N * D * ((mc + LOCAL_KNN_QUERIES - 1) / LOCAL_KNN_QUERIES));
}

void launch_vecchia_ll(const double* Xs, const double* Y, long N, int D, long p0, int mc, int k, const int* nbr, int kt, double sigma2,
                       double diag_add, double nugget, bool grad, double* scratch, int grid, double* out, int* ok, hipStream_t st) {
  const size_t lds = vecchia_lds_bytes(D, grad);
  const char* tag = grad ? "vecchia_ll_grad" : "vecchia_ll";
  prof_begin(tag, st);
#define MOGP_VLL(KT, GR)                                                                                                                      \
  hipLaunchKernelGGL((vecchia_ll_kernel<KT, GR>), dim3(grid), dim3(256), lds, st, Xs, Y, (int)N, D, (int)p0, mc, k, nbr, sigma2, diag_add, nugget, \
                     scratch, out, ok)
  if (kt == 0) {
    if (grad) MOGP_VLL(0, true);
    else MOGP_VLL(0, false);
  } else {
    if (grad) MOGP_VLL(1, true);
    else MOGP_VLL(1, false);
  }
#undef MOGP_VLL
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

void launch_local_knn(const double* Xs, long N, int D, const double* Qs, int mc, int k, int* nbr, double* radius, hipStream_t st) {
  const size_t lds = sizeof(double) * (size_t)D * KNN_LD;
  prof_begin("local_knn", st);
  hipLaunchKernelGGL(local_knn_kernel<false>, dim3((mc + LOCAL_KNN_QUERIES - 1) / LOCAL_KNN_QUERIES), dim3(256), lds, st, Xs, (int)N, D, Qs, mc, k,
                     nbr, radius);
  // algorithmic: a subtraction, a product and an addition per (query, design point, dimension); the design is read once per workgroup
  prof_end("local_knn", st, 3.0 * (double)mc * (double)N * D, 8.0 * (double)N * D * ((mc + LOCAL_KNN_QUERIES - 1) / LOCAL_KNN_QUERIES));
}

void launch_local_gp(const double* Xs, const double* Y, long N, int D, const double* Qs, int mc, int k, const int* nbr, int kt, double sigma2,
                     double diag_add, double var_add, double* scratch, int grid, double* mean, double* var, int* ok, hipStream_t st) {
  const size_t lds = local_gp_lds_bytes(D);
  prof_begin("local_gp", st);
  if (kt == 0)
    hipLaunchKernelGGL((local_gp_kernel<0>), dim3(grid), dim3(256), lds, st, Xs, Y, (int)N, D, Qs, mc, k, nbr, sigma2, diag_add, var_add, scratch,
                       mean, var, ok);
  else
    hipLaunchKernelGGL((local_gp_kernel<1>), dim3(grid), dim3(256), lds, st, Xs, Y, (int)N, D, Qs, mc, k, nbr, sigma2, diag_add, var_add, scratch,
                       mean, var, ok);
  // the factorisation of one whole tile per query (what chol128_dev executes whatever k is); the tile and the pack written once per query
  prof_end("local_gp", st, (double)mc * 128.0 * 128.0 * 128.0 / 3.0, (double)mc * 8.0 * (double)LOCAL_WG_DOUBLES);
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// the handle
// ---------------------------------------------------------------------------------------------------------------------------------------
LocalGP::LocalGP(const double* inputs, long N_, int D_, const double* resid, int E_) : N(N_), D(D_), E(E_) {
  if (!inputs || !resid) throw std::runtime_error("predict_local: null pointer");
  if (D < 1 || D > MAX_D) throw std::runtime_error("predict_local: number of input dimensions must be between 1 and " + std::to_string(MAX_D));
  if (N < 1 || N > LOCAL_MAX_N) throw std::runtime_error("predict_local: the design must have between 1 and " + std::to_string(LOCAL_MAX_N) + " points");
  if (E < 1) throw std::runtime_error("predict_local: at least one row of targets is needed");
  HIPCK(hipGetDevice(&device));
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) n_cu = cus;
  const size_t nd = (size_t)N * D;
  dX.reserve(nd);
  dXs.reserve(nd);
  dY.reserve((size_t)E * N);
  dScale.reserve(D);
  HIPCK(hipMemcpy(dX, inputs, nd * sizeof(double), hipMemcpyHostToDevice));
  HIPCK(hipMemcpy(dY, resid, (size_t)E * N * sizeof(double), hipMemcpyHostToDevice));
}

void LocalGP::ensure_scaled(const double* scale, hipStream_t st) {
  if (hScale.size() == (size_t)D && std::equal(hScale.begin(), hScale.end(), scale)) return;
  hScale.clear();
  HIPCK(hipMemcpyAsync(dScale, scale, D * sizeof(double), hipMemcpyHostToDevice, st));
  launch_local_scale(dX, N, D, dScale, dXs, st);
  HIPCK(hipGetLastError());
  HIPCK(hipStreamSynchronize(st));
  hScale.assign(scale, scale + D);
}

void LocalGP::vecchia_neighbours(const double* scale, int k, int* nbr_out) {
  if (!scale) throw std::runtime_error("vecchia_neighbours: null pointer");
  if (N < 2 || k < 1 || k > LOCAL_MAX_K || k > N - 1)
    throw std::runtime_error("vecchia_neighbours: n_neighbours must be between 1 and " + std::to_string(std::min<long>(N - 1, LOCAL_MAX_K)));
  for (int d = 0; d < D; ++d)
    if (!(scale[d] > 0.) || !std::isfinite(scale[d])) throw std::runtime_error("vecchia_neighbours: the scales must be positive and finite");
  DeviceGuard guard(device);
  hipStream_t st = nullptr;
  SyncOnUnwind sync{st};
  vk = 0;
  dVnbr.reserve((size_t)N * k);
  ensure_scaled(scale, st);
  launch_vecchia_knn(dXs, N, D, k, dVnbr, st);
  HIPCK(hipGetLastError());
  if (nbr_out) HIPCK(hipMemcpyAsync(nbr_out, dVnbr, (size_t)N * k * sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCK(hipStreamSynchronize(st));
  vk = k;
}

void LocalGP::vecchia_loglik(int e, int kt, const double* scale, double sigma2, double nugget, double jitter, int k, bool want_grad, int max_points,
                             double* value_out, double* grad_out, double* terms_out, int* ok_out) {
  if (!scale || !value_out || (want_grad && !grad_out)) throw std::runtime_error("vecchia_loglik: null pointer");
  if (e < 0 || e >= E) throw std::runtime_error("vecchia_loglik: emulator index out of range");
  if (kt != 0 && kt != 1) throw std::runtime_error("vecchia_loglik: the kernel must be a function of one scaled distance (squared exponential or Matern 5/2)");
  if (vk == 0) throw std::runtime_error("vecchia_loglik: the neighbour lists have not been built (vecchia_neighbours)");
  if (k != vk) throw std::runtime_error("vecchia_loglik: the neighbour lists were built for n_neighbours = " + std::to_string(vk));
  if (!(sigma2 > 0.) || !std::isfinite(sigma2) || !(nugget >= 0.) || !std::isfinite(nugget) || !(jitter >= 0.) || !std::isfinite(jitter))
    throw std::runtime_error("vecchia_loglik: sigma^2 must be positive and finite, nugget and jitter finite and not negative");
  for (int d = 0; d < D; ++d)
    if (!(scale[d] > 0.) || !std::isfinite(scale[d])) throw std::runtime_error("vecchia_loglik: the scales must be positive and finite");
  DeviceGuard guard(device);
  hipStream_t st = nullptr;
  size_t free_b = 0, total_b = 0;
  HIPCK(hipMemGetInfo(&free_b, &total_b));
  const size_t wg = want_grad ? VECCHIA_WG_DOUBLES : LOCAL_WG_DOUBLES;
  const int cols = want_grad ? D + 3 : 1;
  // what the handle holds from earlier calls is not free any more but is reused
  const double held = 8.0 * ((double)dVout.size() + (double)dVred.size() + (double)dVscratch.size()) + 4.0 * (double)dVok.size();
  const VecchiaPlan plan = vecchia_plan(N, D, want_grad, n_cu, (double)free_b + held, max_points, (double)wg * sizeof(double));
  SyncOnUnwind sync{st};
  dVout.reserve((size_t)cols * N);
  dVok.reserve((size_t)N);
  dVred.reserve((size_t)2 * cols * plan.blocks);
  dVscratch.reserve((size_t)plan.grid * wg);
  ensure_scaled(scale, st);
  const double* dYe = dY.get() + (size_t)e * N;
  for (long c0 = 0; c0 < N; c0 += plan.points) {
    const int mc = (int)std::min<long>(plan.points, N - c0);
    launch_vecchia_ll(dXs, dYe, N, D, c0, mc, k, dVnbr, kt, sigma2, nugget + jitter, nugget, want_grad, dVscratch, std::min(plan.grid, mc), dVout,
                      dVok, st);
  }
  HIPCK(hipGetLastError());
  double* half = dVred.get() + (size_t)cols * plan.blocks;
  const double* sums = launch_vecchia_reduce(dVout, N, cols, dVred, half, st);
  HIPCK(hipGetLastError());
  std::vector<double> h(cols);
  HIPCK(hipMemcpyAsync(h.data(), sums, (size_t)cols * sizeof(double), hipMemcpyDeviceToHost, st));
  if (terms_out) HIPCK(hipMemcpyAsync(terms_out, dVout, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, st));
  if (ok_out) HIPCK(hipMemcpyAsync(ok_out, dVok, (size_t)N * sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCK(hipStreamSynchronize(st));
  *value_out = h[0];
  if (want_grad) std::copy(h.begin() + 1, h.end(), grad_out);
}

void LocalGP::predict(int e, int kt, const double* scale, double sigma2, double nugget, double jitter, bool include_nugget, const double* testing,
                      long m, int k, int max_points, double* mean, double* var, int* ok, double* radius, int* nbr) {
  if (!scale || !testing || !mean || !ok || !radius) throw std::runtime_error("predict_local: null pointer");
  if (e < 0 || e >= E) throw std::runtime_error("predict_local: emulator index out of range");
  if (kt != 0 && kt != 1) throw std::runtime_error("predict_local: the kernel must be a function of one scaled distance (squared exponential or Matern 5/2)");
  if (k < 1 || k > LOCAL_MAX_K || k > N)
    throw std::runtime_error("predict_local: n_neighbours must be between 1 and " + std::to_string(std::min<long>(N, LOCAL_MAX_K)));
  if (m < 1 || m > INT_MAX) throw std::runtime_error("predict_local: at least one testing point is needed");
  if (!(sigma2 > 0.) || !std::isfinite(sigma2) || !(nugget >= 0.) || !std::isfinite(nugget) || !(jitter >= 0.) || !std::isfinite(jitter))
    throw std::runtime_error("predict_local: sigma^2 must be positive and finite, nugget and jitter finite and not negative");
  for (int d = 0; d < D; ++d)
    if (!(scale[d] > 0.) || !std::isfinite(scale[d])) throw std::runtime_error("predict_local: the scales must be positive and finite");
  DeviceGuard guard(device);
  hipStream_t st = nullptr;
  size_t free_b = 0, total_b = 0;
  HIPCK(hipMemGetInfo(&free_b, &total_b));
  const LocalPlan plan = local_plan(m, D, k, n_cu, (double)free_b, max_points, (double)LOCAL_WG_DOUBLES * sizeof(double));
  const size_t P = (size_t)plan.points;
  DevBuf<double> dQ(P * D), dQs(P * D), dRad(P), dMean(P), dVar(P), dScratch((size_t)plan.grid * LOCAL_WG_DOUBLES);
  DevBuf<int> dNbr(P * k), dOk(P);
  SyncOnUnwind sync{st};
  ensure_scaled(scale, st);
  const double* dYe = dY.get() + (size_t)e * N;
  for (long c0 = 0; c0 < m; c0 += plan.points) {
    const int mc = (int)std::min<long>(plan.points, m - c0);
    const int grid = std::min(plan.grid, mc);
    HIPCK(hipMemcpyAsync(dQ, testing + (size_t)c0 * D, (size_t)mc * D * sizeof(double), hipMemcpyHostToDevice, st));
    launch_local_scale(dQ, mc, D, dScale, dQs, st);
    launch_local_knn(dXs, N, D, dQs, mc, k, dNbr, dRad, st);
    launch_local_gp(dXs, dYe, N, D, dQs, mc, k, dNbr, kt, sigma2, nugget + jitter, include_nugget ? nugget : 0., dScratch, grid, dMean, dVar, dOk, st);
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(mean + c0, dMean, (size_t)mc * sizeof(double), hipMemcpyDeviceToHost, st));
    if (var) HIPCK(hipMemcpyAsync(var + c0, dVar, (size_t)mc * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCK(hipMemcpyAsync(ok + c0, dOk, (size_t)mc * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCK(hipMemcpyAsync(radius + c0, dRad, (size_t)mc * sizeof(double), hipMemcpyDeviceToHost, st));
    if (nbr) HIPCK(hipMemcpyAsync(nbr + (size_t)c0 * k, dNbr, (size_t)mc * k * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
  }
}

}  // namespace mogp
