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
  for (int j0 = 0; j0 < N; j0 += LOCAL_KNN_ROWS) {
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
        const bool cand = row < N && pair_less(acc[h][a], row, thr[a], thi[a]);
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
      if (lane < k) out[lane] = i0[a];
      if (64 + lane < k) out[64 + lane] = i1[a];
      if (lane == 0) radius[q] = thr[a];
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

}  // namespace

void launch_local_scale(const double* x, long rows, int D, const double* s, double* out, hipStream_t st) {
  const size_t total = (size_t)rows * D;
  if (total == 0) return;
  const unsigned grid = (unsigned)std::min<size_t>((total + 255) / 256, 8192);
  hipLaunchKernelGGL(local_scale_kernel, dim3(grid), dim3(256), 0, st, x, total, D, s, out);
}

void launch_local_knn(const double* Xs, long N, int D, const double* Qs, int mc, int k, int* nbr, double* radius, hipStream_t st) {
  const size_t lds = sizeof(double) * (size_t)D * KNN_LD;
  prof_begin("local_knn", st);
  hipLaunchKernelGGL(local_knn_kernel, dim3((mc + LOCAL_KNN_QUERIES - 1) / LOCAL_KNN_QUERIES), dim3(256), lds, st, Xs, (int)N, D, Qs, mc, k, nbr,
                     radius);
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
  if (hScale.size() != (size_t)D || !std::equal(hScale.begin(), hScale.end(), scale)) {
    hScale.clear();
    HIPCK(hipMemcpyAsync(dScale, scale, D * sizeof(double), hipMemcpyHostToDevice, st));
    launch_local_scale(dX, N, D, dScale, dXs, st);
    HIPCK(hipGetLastError());
    HIPCK(hipStreamSynchronize(st));
    hScale.assign(scale, scale + D);
  }
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
