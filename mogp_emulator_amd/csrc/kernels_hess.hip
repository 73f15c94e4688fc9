// Hessian of the negative log-posterior F with respect to theta = [corr_raw | log sigma^2 | log eta (fit only)] (DESIGN.md section 3,
// "Hessian").  Q = sigma^2 C + eta I, alpha = Q^-1 t, s_p(a, b) = e_p (x_ap - x_bp)^2, r2 = sum_p s_p, W = Q^-1 - alpha alpha^T:
//   F_pq = alpha^T Q_p Q^-1 Q_q alpha - 1/2 tr(Q^-1 Q_p Q^-1 Q_q) + 1/2 sum W o Q_pq  -  delta_pq d2 log prior
//   Q_p = sigma^2 k'(r2) s_p                                     Q_pq = sigma^2 (k''(r2) s_p s_q + delta_pq k'(r2) s_p)
// The kernels here give the pieces that involve the D correlation planes; the covariance and nugget planes follow from them, from
// K^-1 and from the gradient's sums on the host (Engine::hessian):
//   hess_scale     Xs = X sqrt(e_d), zero rows up to a multiple of 64 (the operand generators read it)
//   hess_gemm      M_p = Q^-1 Q_p, an MFMA GEMM whose B operand never exists in memory: every 16 x 64 tile of sigma^2 k'(r2) is
//                  generated ONCE per k-step from Xs and multiplied by s_p for each of the PG planes the workgroup carries
//   hess_trace     T[p][q] = sum_ab M_p[a,b] M_q[b,a], with Q^-1 and I as two extra "planes" (tr(M_p Q^-1), tr(M_p), tr(Q^-2))
//   hess_pair      A[p][q] = sum_ab W[a,b] sigma^2 k''(r2) s_p s_q over the lower triangle (the gradient kernel's tiling)
//   hess_matvec    v_p = M_p^T t (= Q_p alpha) and u_p = M_p alpha (= Q^-1 Q_p alpha);  hess_symv  z = Q^-1 alpha
// K^-1 is valid in its lower triangle only (launch.h): every reader takes entry (max(a, b), min(a, b)) and nothing at or beyond row n.
//
// Reductions: a wave adds by xor-shuffles (every lane ends with the same sum), the four waves meet in LDS in a fixed order, a workgroup
// walks its tiles in ascending order into an LDS table and writes the table into a scratch slot of its own; hess_sum adds the slots in
// ascending order.  No atomics: the same inputs give the same bits in every call.
#include <algorithm>
#include <stdexcept>

#include "cov_dev.h"
#include "gemm_dev.h"
#include "launch.h"

namespace mogp {

namespace {

__device__ __forceinline__ int hess_emu(const int* idx, int z) { return idx ? idx[z] : z; }

// d2k / d(r2)^2
template <int KT>
__device__ __forceinline__ double kern_d2r2(double r2, const double* tab) {
  if (KT == 0) return 0.25 * lean_exp_neg<true>(r2, tab);
  const double s = sqrt(5.0 * r2);
  return (25.0 / 12.0) * lean_exp_neg<false>(s, tab);
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// entry (a, b) of Q^-1 from its lower triangle; 0 outside the n x n block
__device__ __forceinline__ double kinv_sym(const double* __restrict__ Ki, int ld, int n, int a, int b) {
  const int hi = max(a, b), lo = min(a, b);
  return hi < n ? Ki[(size_t)hi * ld + lo] : 0.0;
}

// Xs[z][r][d] = X[r][d] sqrt(e_d) for r < n, 0 for n <= r < NPh (the product stage_rows<true> forms)
__global__ __launch_bounds__(256) void hess_scale_kernel(BatchView v, int NPh, double* __restrict__ Xs) {
  const int z = blockIdx.y, emu = hess_emu(v.idx, z);
  const double* P = v.P + (size_t)emu * v.PS;
  const double* X = v.X + (size_t)emu * v.XS;
  const int total = NPh * v.D, live = v.n * v.D;
  double* out = Xs + (size_t)z * total;
  for (int e = blockIdx.x * 256 + threadIdx.x; e < total; e += gridDim.x * 256) out[e] = e < live ? X[e] * sqrt(P[e % v.D]) : 0.0;
}

// ---------------------------------------------------------------------------------------------
// M_p[64 i-tile, 64 j-tile] for the planes p0 .. p0 + PG - 1.  2 x 2 waves, 32 x 32 per wave; the k-step of mainloop_w (operand tiles
// [row][16 + 2] in LDS, two stages, one barrier per step) with both operands produced in registers first:
//   A: rows of Q^-1, mirrored from the lower triangle -- a k-step left of the tile's diagonal block reads rows, one right of it reads
//      columns (either way a wave reads whole segments), the steps across the diagonal block choose per entry;
//   B: thread (kk, jb) = (t & 15, t >> 4) owns k-row kk and the columns jb + 16 e: r2 over all D dimensions and sigma^2 k'(r2) once, then
//      s_p per plane.  k-rows and columns at or beyond n are zero, so the padding of M is exact zeros.
// ---------------------------------------------------------------------------------------------
template <int KT, int PG>
__global__ __launch_bounds__(256) void hess_gemm_kernel(BatchView v, const double* __restrict__ Xs, int NPh, double* __restrict__ M) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  __shared__ double etab[256];
  stage_exp_tab(etab);
  constexpr int OP = 64 * LDK;
  double* sA = sm;                    // [2][OP]
  double* sB = sm + 2 * OP;           // [2][PG][OP]
  double* sxj = sB + 2 * PG * OP;     // [D][64]
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wr = wave >> 1, wc = wave & 1, fr = lane & 15, fk = lane >> 4;
  const int z = blockIdx.z, emu = hess_emu(v.idx, z);
  const int nt = NPh / 64;
  const int ti = blockIdx.x / nt, tj = blockIdx.x - ti * nt;
  const int i0 = ti * 64, j0 = tj * 64, p0 = blockIdx.y * PG;
  const int n = v.n, D = v.D, ld = v.LD;
  const double* Ki = v.Kinv + (size_t)emu * v.MS;
  const double* xs = Xs + (size_t)z * NPh * D;
  const double sig2 = v.P[(size_t)emu * v.PS + D];
  for (int e = t; e < 64 * D; e += 256) {
    const int r = e / D, d = e - r * D;
    sxj[d * 64 + r] = xs[(size_t)(j0 + r) * D + d];
  }
  __syncthreads();
  v4d acc[PG][2][2];
#pragma unroll
  for (int q = 0; q < PG; ++q)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[q][i][j] = (v4d){0., 0., 0., 0.};
  double ra[4], rb[PG][4];
  const int kk = t & 15, jb = t >> 4;
  // A entries of the thread: (row, k) = ((t >> 4) + 16 e, t & 15), or ((t & 63), (t >> 6) + 4 e) where the step reads columns of Q^-1
  auto by_cols = [&](int k0) { return k0 >= i0 + 64; };
  auto loadA = [&](int k0) {
    if (k0 + BK <= i0) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int i = i0 + jb + 16 * e, k = k0 + kk;
        ra[e] = (i < n) ? Ki[(size_t)i * ld + k] : 0.0;       // k < i
      }
    } else if (by_cols(k0)) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int i = i0 + (t & 63), k = k0 + (t >> 6) + 4 * e;
        ra[e] = (k < n) ? Ki[(size_t)k * ld + i] : 0.0;       // i < k
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) ra[e] = kinv_sym(Ki, ld, n, i0 + jb + 16 * e, k0 + kk);
    }
  };
  auto genB = [&](int k0) {
    const int krow = k0 + kk;
    const double* xk = xs + (size_t)krow * D;
    double r2[4] = {0., 0., 0., 0.};
    for (int d = 0; d < D; ++d) {
      const double xkd = xk[d];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double df = xkd - sxj[d * 64 + jb + 16 * e];
        r2[e] = __builtin_fma(df, df, r2[e]);
      }
    }
    double g[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) g[e] = (krow < n && j0 + jb + 16 * e < n) ? sig2 * kern_dr2<KT>(r2[e], etab) : 0.0;
#pragma unroll
    for (int q = 0; q < PG; ++q) {
      const int p = min(p0 + q, D - 1);                        // (a plane past the last one repeats it; it is not stored)
      const double xkp = xk[p];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double df = xkp - sxj[p * 64 + jb + 16 * e];
        rb[q][e] = g[e] * (df * df);
      }
    }
  };
  auto store = [&](int k0, int stage) {
    double* dA = sA + stage * OP;
    double* dB = sB + stage * PG * OP;
    if (by_cols(k0)) {
#pragma unroll
      for (int e = 0; e < 4; ++e) dA[(t & 63) * LDK + (t >> 6) + 4 * e] = ra[e];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) dA[(jb + 16 * e) * LDK + kk] = ra[e];
    }
#pragma unroll
    for (int q = 0; q < PG; ++q)
#pragma unroll
      for (int e = 0; e < 4; ++e) dB[q * OP + (jb + 16 * e) * LDK + kk] = rb[q][e];
  };
  const int nk = NPh / BK;
  loadA(0);
  genB(0);
  store(0, 0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const double* cA = sA + (kt & 1) * OP;
    const double* cB = sB + (kt & 1) * PG * OP;
    const bool more = kt + 1 < nk;
    if (more) {
      loadA((kt + 1) * BK);
      genB((kt + 1) * BK);
    }
#pragma unroll
    for (int k4 = 0; k4 < 4; ++k4) {
      const int k = k4 * 4 + fk;
      double a[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) a[i] = cA[(wr * 32 + i * 16 + fr) * LDK + k];
#pragma unroll
      for (int q = 0; q < PG; ++q) {
        double b[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) b[j] = cB[q * OP + (wc * 32 + j * 16 + fr) * LDK + k];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[q][i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[q][i][j], 0, 0, 0);
      }
    }
    if (more) store((kt + 1) * BK, (kt + 1) & 1);
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < PG; ++q) {
    if (p0 + q >= D) continue;
    double* Mp = M + ((size_t)z * D + p0 + q) * NPh * NPh;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          Mp[(size_t)(i0 + wr * 32 + i * 16 + fk + 4 * r) * NPh + j0 + wc * 32 + j * 16 + fr] = acc[q][i][j][r];
  }
}

// ---------------------------------------------------------------------------------------------
// tab[p][q] = sum_ab P_p[a, b] P_q[b, a] with the planes P_0 .. P_{D-1} = M_p, P_D = Q^-1, P_{D+1} = I: rows p < D hold q = p .. D + 1,
// row D holds q = D (the squared Frobenius norm of Q^-1); the other entries of the (D + 1) x (D + 2) table stay zero.
// Workgroup g walks the 64 x 64 tiles g, g + G, ...; per tile and p the tile of P_p is parked in LDS and every P_q tile streams past it.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hess_trace_kernel(BatchView v, const double* __restrict__ M, int NPh, double* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int n = v.n, D = v.D, ld = v.LD, TQ = D + 2, TS = (D + 1) * TQ;
  double* tab = sm;                   // [D + 1][D + 2]
  double* sM = tab + TS;              // [64][65]
  double* wacc = sM + 64 * 65;        // [D + 2][4]
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int z = blockIdx.y, emu = hess_emu(v.idx, z);
  const double* Ki = v.Kinv + (size_t)emu * v.MS;
  const double* Mz = M + (size_t)z * D * NPh * NPh;
  const int nt = NPh / 64, ntiles = nt * nt;
  for (int e = t; e < TS; e += 256) tab[e] = 0.0;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int ti = tile / nt, tj = tile - ti * nt;
    const int i0 = ti * 64, j0 = tj * 64;
    for (int p = 0; p <= D; ++p) {
      const double* Mp = Mz + (size_t)p * NPh * NPh;
#pragma unroll 4
      for (int e = 0; e < 16; ++e) {
        const int r = wave + 4 * e;
        sM[r * 65 + lane] = p < D ? Mp[(size_t)(i0 + r) * NPh + j0 + lane] : kinv_sym(Ki, ld, n, i0 + r, j0 + lane);
      }
      __syncthreads();
      const int q1 = p < D ? D + 1 : D;
      for (int q = p; q <= q1; ++q) {
        const double* Mq = Mz + (size_t)q * NPh * NPh;
        double s = 0.;
#pragma unroll 4
        for (int e = 0; e < 16; ++e) {
          const int r = j0 + wave + 4 * e, c = i0 + lane;        // entry (r, c) of P_q meets entry (c, r) of P_p
          double b;
          if (q < D) b = Mq[(size_t)r * NPh + c];
          else if (q == D) b = kinv_sym(Ki, ld, n, r, c);
          else b = (r == c && r < n) ? 1.0 : 0.0;
          s = __builtin_fma(sM[lane * 65 + wave + 4 * e], b, s);
        }
        s = wave_sum(s);
        if (lane == 0) wacc[q * 4 + wave] = s;
      }
      __syncthreads();
      if (t >= p && t <= q1) tab[p * TQ + t] += (wacc[t * 4] + wacc[t * 4 + 1]) + (wacc[t * 4 + 2] + wacc[t * 4 + 3]);
      // (the next tile of P_p is written behind the barrier above, the next wacc behind the barrier that follows it)
    }
  }
  __syncthreads();
  double* out = partial + ((size_t)z * gridDim.x + blockIdx.x) * TS;
  for (int e = t; e < TS; e += 256) out[e] = tab[e];
}

// ---------------------------------------------------------------------------------------------
// tab[p][q] = sum_ab w_ab W[a,b] sigma^2 k''(r2_ab) s_p(a,b) s_q(a,b), p <= q < D, over the lower triangle (w = 2 below the diagonal, 1 on
// it): 64 x 64 tiles, 4 x 4 entries per thread as in the gradient kernel.
// ---------------------------------------------------------------------------------------------
template <int KT>
__global__ __launch_bounds__(256) void hess_pair_kernel(BatchView v, const double* __restrict__ Xs, int NPh, double* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  __shared__ double etab[256];
  stage_exp_tab(etab);
  const int n = v.n, D = v.D, ld = v.LD, TS = D * D;
  double* tab = sm;                   // [D][D]
  double* si = tab + TS;              // [D][64]
  double* sj = si + 64 * D;
  double* wacc = sj + 64 * D;         // [D][4]
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, ty = t >> 4, tx = t & 15;
  const int z = blockIdx.y, emu = hess_emu(v.idx, z);
  const double* Ki = v.Kinv + (size_t)emu * v.MS;
  const double* alpha = v.alpha + (size_t)emu * v.RA * ld;
  const double* xs = Xs + (size_t)z * NPh * D;
  const double sig2 = v.P[(size_t)emu * v.PS + D];
  const int nt = NPh / 64, ntiles = nt * (nt + 1) / 2;
  for (int e = t; e < TS; e += 256) tab[e] = 0.0;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    int ti = (int)((sqrt(8.0 * tile + 1.0) - 1.0) * 0.5);
    while (ti * (ti + 1) / 2 > tile) --ti;
    while ((ti + 1) * (ti + 2) / 2 <= tile) ++ti;
    const int tj = tile - ti * (ti + 1) / 2;
    const int i0 = ti * 64, j0 = tj * 64;
    __syncthreads();                  // the previous tile's readers of si / sj are done (and etab / tab are published)
    for (int e = t; e < 64 * D; e += 256) {
      const int r = e / D, d = e - r * D;
      si[d * 64 + r] = xs[(size_t)(i0 + r) * D + d];
      sj[d * 64 + r] = xs[(size_t)(j0 + r) * D + d];
    }
    __syncthreads();
    double G[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) G[a][b] = 0.0;
    for (int d = 0; d < D; ++d) {
      double xi[4], xj[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) xi[a] = si[d * 64 + 4 * ty + a];
#pragma unroll
      for (int b = 0; b < 4; ++b) xj[b] = sj[d * 64 + 4 * tx + b];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const double df = xi[a] - xj[b];
          G[a][b] = __builtin_fma(df, df, G[a][b]);
        }
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int i = i0 + 4 * ty + a;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int j = j0 + 4 * tx + b;
        const bool live = i < n && j <= i;
        const double W = live ? Ki[(size_t)i * ld + j] - alpha[i] * alpha[j] : 0.0;
        const double w = live ? (j < i ? 2.0 : 1.0) : 0.0;
        G[a][b] = w * W * sig2 * kern_d2r2<KT>(G[a][b], etab);
      }
    }
    for (int p = 0; p < D; ++p) {
      double gp[4][4];
      {
        double xi[4], xj[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) xi[a] = si[p * 64 + 4 * ty + a];
#pragma unroll
        for (int b = 0; b < 4; ++b) xj[b] = sj[p * 64 + 4 * tx + b];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            const double df = xi[a] - xj[b];
            gp[a][b] = G[a][b] * (df * df);
          }
      }
      for (int q = p; q < D; ++q) {
        double xi[4], xj[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) xi[a] = si[q * 64 + 4 * ty + a];
#pragma unroll
        for (int b = 0; b < 4; ++b) xj[b] = sj[q * 64 + 4 * tx + b];
        double s = 0.;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            const double df = xi[a] - xj[b];
            s = __builtin_fma(gp[a][b], df * df, s);
          }
        s = wave_sum(s);
        if (lane == 0) wacc[q * 4 + wave] = s;
      }
      __syncthreads();
      if (t >= p && t < D) tab[p * D + t] += (wacc[t * 4] + wacc[t * 4 + 1]) + (wacc[t * 4 + 2] + wacc[t * 4 + 3]);
      __syncthreads();
    }
  }
  __syncthreads();
  double* out = partial + ((size_t)z * gridDim.x + blockIdx.x) * TS;
  for (int e = t; e < TS; e += 256) out[e] = tab[e];
}

// out[z][e] = sum over the G slots of partial[z][g][e], g ascending
__global__ __launch_bounds__(256) void hess_sum_kernel(const double* __restrict__ partial, int G, int TS, double* __restrict__ out) {
  const int z = blockIdx.y, e = blockIdx.x * 256 + threadIdx.x;
  if (e >= TS) return;
  const double* p = partial + (size_t)z * G * TS + e;
  double s = 0.;
  for (int g = 0; g < G; ++g) s += p[(size_t)g * TS];
  out[(size_t)z * TS + e] = s;
}

// V[z][p][b] = sum_a M_p[a, b] t_a (64 columns per workgroup: four row phases, added in a fixed order);
// U[z][p][a] = sum_b M_p[a, b] alpha_b (64 rows per workgroup, a wave per row)
__global__ __launch_bounds__(256) void hess_matvec_kernel(BatchView v, const double* __restrict__ M, int NPh, double* __restrict__ V,
                                                          double* __restrict__ U) {
  __shared__ double sv[4][64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int z = blockIdx.z, p = blockIdx.y, b0 = blockIdx.x * 64;
  const int emu = hess_emu(v.idx, z), n = v.n;
  const double* Mp = M + ((size_t)z * v.D + p) * NPh * NPh;
  const double* tt = v.T + (size_t)emu * n;
  const double* alpha = v.alpha + (size_t)emu * v.RA * v.LD;
  double s = 0.;
  for (int a = wave; a < n; a += 4) s = __builtin_fma(Mp[(size_t)a * NPh + b0 + lane], tt[a], s);
  sv[wave][lane] = s;
  __syncthreads();
  if (t < 64) V[((size_t)z * v.D + p) * NPh + b0 + t] = (sv[0][t] + sv[1][t]) + (sv[2][t] + sv[3][t]);
  for (int r = wave; r < 64; r += 4) {
    const double* row = Mp + (size_t)(b0 + r) * NPh;
    double u = 0.;
    for (int b = lane; b < n; b += 64) u = __builtin_fma(row[b], alpha[b], u);
    u = wave_sum(u);
    if (lane == 0) U[((size_t)z * v.D + p) * NPh + b0 + r] = u;
  }
}

// Zv[z][a] = sum_b Q^-1[a, b] alpha_b, a < NPh (0 beyond n): a wave per row
__global__ __launch_bounds__(256) void hess_symv_kernel(BatchView v, int NPh, double* __restrict__ Zv) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int z = blockIdx.y, emu = hess_emu(v.idx, z), n = v.n, ld = v.LD;
  const double* Ki = v.Kinv + (size_t)emu * v.MS;
  const double* alpha = v.alpha + (size_t)emu * v.RA * ld;
  const int a = blockIdx.x * 4 + wave;
  if (a >= NPh) return;
  double s = 0.;
  for (int b = lane; b < n; b += 64) s = __builtin_fma(kinv_sym(Ki, ld, n, a, b), alpha[b], s);
  s = wave_sum(s);
  if (lane == 0) Zv[(size_t)z * NPh + a] = s;
}

}  // namespace

int hess_np(int n) { return (n + 63) / 64 * 64; }
int hess_trace_groups(int n) {
  const int nt = hess_np(n) / 64;
  return std::min(nt * nt, HESS_MAX_GROUPS);
}
int hess_pair_groups(int n) {
  const int nt = hess_np(n) / 64;
  return std::min(nt * (nt + 1) / 2, HESS_MAX_GROUPS);
}

void launch_hess_scale(const BatchView& v, double* Xs, hipStream_t s) {
  const int NPh = hess_np(v.n);
  const int g = std::max(1, std::min(1024, (NPh * v.D + 255) / 256));
  hipLaunchKernelGGL(hess_scale_kernel, dim3(g, v.nb), dim3(256), 0, s, v, NPh, Xs);
}

void launch_hess_planes(const BatchView& v, const double* Xs, double* M, hipStream_t s) {
  if (v.kernel_type != 0 && v.kernel_type != 1) throw std::runtime_error("hessian: kernel not supported");
  const int NPh = hess_np(v.n), nt = NPh / 64, D = v.D;
  const int PG = D >= 4 ? 4 : (D >= 2 ? 2 : 1);
  const size_t smem = (size_t)(2 * 64 * LDK * (1 + PG) + 64 * D) * sizeof(double);
  const dim3 grid(nt * nt, (D + PG - 1) / PG, v.nb);
  prof_begin("hess_planes", s);
#define CALL(K, G) hipLaunchKernelGGL((hess_gemm_kernel<K, G>), grid, dim3(256), smem, s, v, Xs, NPh, M)
  if (v.kernel_type == 0) {
    if (PG == 4) CALL(0, 4); else if (PG == 2) CALL(0, 2); else CALL(0, 1);
  } else {
    if (PG == 4) CALL(1, 4); else if (PG == 2) CALL(1, 2); else CALL(1, 1);
  }
#undef CALL
  prof_end("hess_planes", s, 2.0 * v.nb * (double)D * v.n * (double)v.n * v.n, 0.);
}

void launch_hess_trace(const BatchView& v, const double* M, double* partial, double* out, hipStream_t s) {
  const int NPh = hess_np(v.n), D = v.D, G = hess_trace_groups(v.n), TS = (D + 1) * (D + 2);
  const size_t smem = (size_t)(TS + 64 * 65 + 4 * (D + 2)) * sizeof(double);
  prof_begin("hess_trace", s);
  hipLaunchKernelGGL(hess_trace_kernel, dim3(G, v.nb), dim3(256), smem, s, v, M, NPh, partial);
  hipLaunchKernelGGL(hess_sum_kernel, dim3((TS + 255) / 256, v.nb), dim3(256), 0, s, (const double*)partial, G, TS, out);
  prof_end("hess_trace", s, 0., 8.0 * v.nb * (double)NPh * NPh * (D + 1.0) * (D + 2.0) / 2.0);
}

void launch_hess_pair(const BatchView& v, const double* Xs, double* partial, double* out, hipStream_t s) {
  if (v.kernel_type != 0 && v.kernel_type != 1) throw std::runtime_error("hessian: kernel not supported");
  const int NPh = hess_np(v.n), D = v.D, G = hess_pair_groups(v.n), TS = D * D;
  const size_t smem = (size_t)(TS + 128 * D + 4 * D) * sizeof(double);
  prof_begin("hess_pair", s);
  if (v.kernel_type == 0) hipLaunchKernelGGL(hess_pair_kernel<0>, dim3(G, v.nb), dim3(256), smem, s, v, Xs, NPh, partial);
  else hipLaunchKernelGGL(hess_pair_kernel<1>, dim3(G, v.nb), dim3(256), smem, s, v, Xs, NPh, partial);
  hipLaunchKernelGGL(hess_sum_kernel, dim3((TS + 255) / 256, v.nb), dim3(256), 0, s, (const double*)partial, G, TS, out);
  prof_end("hess_pair", s, 0., 8.0 * v.nb * (double)v.n * v.n / 2.0);
}

void launch_hess_vectors(const BatchView& v, const double* M, double* V, double* U, double* Zv, hipStream_t s) {
  const int NPh = hess_np(v.n);
  prof_begin("hess_vectors", s);
  hipLaunchKernelGGL(hess_matvec_kernel, dim3(NPh / 64, v.D, v.nb), dim3(256), 0, s, v, M, NPh, V, U);
  hipLaunchKernelGGL(hess_symv_kernel, dim3(NPh / 4, v.nb), dim3(256), 0, s, v, NPh, Zv);
  prof_end("hess_vectors", s, 0., 16.0 * v.nb * (double)NPh * NPh * v.D);
}

}  // namespace mogp
