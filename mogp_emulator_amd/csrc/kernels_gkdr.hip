// gKDR dimension reduction (Fukumizu and Leng; mogp_emulator/DimensionReduction.py:132-236): the M x M matrix R of every
// (X_scale, Y_scale) pair of a tuning grid in one call.  Per input scale s (SGX^2) the Gram matrix Kx and A = Kx + N EPS I are built on
// the device, A = L L^T is factored and L^-1 formed by the engine's batched Cholesky and trtri (a ScratchFactor, engine_internal.h); per output
// scale Ky is built the same way.  R is formed WITHOUT the N x N x M tensor of the reference, from the identity (Xc = X - mean(X); R does
// not change when X is shifted)
//   s^2 R = Xc^T (F o KxKx) Xc - Xc^T T Xc - (Xc^T T Xc)^T + Xc^T diag(c) Xc,   F = A^-1 Ky A^-1, G = F Kx, T = Kx o G, c_j = sum_i T_ij
// which is s^2 R = Q + Q^T with Q = Xc^T W Xc and W = F o KxKx / 2 - T + diag(c) / 2.  F is formed in the L^-1 form
// F = L^-T (L^-1 Ky L^-T) L^-1: four triangular-times-full MFMA products (half the flops of full ones).  Through the explicit inverse,
// F = A^-1 Ky A^-1, R was up to 24 cond(A) eps from the exact value; in the L^-1 form it stays within a few cond(A) eps, as the
// reference's does.  Then F Kx with W and T formed in its epilogue, and the two sandwiches with Xc; Kx Kx once per input scale.
// Every reduction has a fixed order (no atomics): R of a pair is bitwise the same whatever else is in the call or the pass.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "cov_dev.h"
#include "engine_internal.h"
#include "gemm_dev.h"

namespace mogp {

namespace {

constexpr int GT = 64;      // Gram tile (64 x 64, 256 threads, 4 x 4 entries each)
constexpr int GC = 16;      // input dimensions staged per step

// out[b] (NP x NP, row stride NP): exp(-|x_i - x_j|^2 / (2 s2[is[b]])) for i, j < n, 0 elsewhere; the squared distance is the
// difference form sum_d (x_id - x_jd)^2, summed in order of d.  eng (optional): the engine's factor matrix of slot b (launch.h
// layout, one right-hand side): the same plus `shift` on the diagonal, a zero target row n with PAD_BIG on its diagonal, identity
// padding beyond.
__global__ __launch_bounds__(256) void gkdr_gram_kernel(const double* __restrict__ X, int n, int m, const double* __restrict__ s2,
                                                        const int* __restrict__ is, double* __restrict__ out, int NP, double shift,
                                                        double* __restrict__ eng, size_t estride) {
  __shared__ double xi[GC][GT + 1], xj[GC][GT + 1];
  __shared__ double etab[256];
  stage_exp_tab(etab);
  const int b = blockIdx.z;
  const int i0 = blockIdx.y * GT, j0 = blockIdx.x * GT;
  const int t = threadIdx.x, ty = t >> 4, tx = t & 15;
  double r2[4][4] = {};
  if (i0 < n && j0 < n) {
    for (int d0 = 0; d0 < m; d0 += GC) {
      __syncthreads();
      for (int e = t; e < GC * GT; e += 256) {
        const int r = e / GC, d = e % GC;
        const bool ok = d0 + d < m;
        xi[d][r] = (ok && i0 + r < n) ? X[(size_t)(i0 + r) * m + d0 + d] : 0.0;
        xj[d][r] = (ok && j0 + r < n) ? X[(size_t)(j0 + r) * m + d0 + d] : 0.0;
      }
      __syncthreads();
      const int dn = min(GC, m - d0);
      for (int d = 0; d < dn; ++d) {
        double a[4], c[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          a[u] = xi[d][ty + 16 * u];
          c[u] = xj[d][tx + 16 * u];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int w = 0; w < 4; ++w) {
            const double df = a[u] - c[w];
            r2[u][w] = __builtin_fma(df, df, r2[u][w]);
          }
      }
    }
  } else {
    __syncthreads();
  }
  const double inv = 1.0 / s2[is ? is[b] : b];
  double* o = out + (size_t)b * NP * NP;
  double* g = eng ? eng + (size_t)b * estride : nullptr;
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int i = i0 + ty + 16 * u, j = j0 + tx + 16 * w;
      const bool in = i < n && j < n;
      // exp(-r2 / (2 s2)) = lean_exp_neg<true>(r2 / s2): the factor 1/2 is folded in exactly (exp_dev.h)
      const double k = in ? lean_exp_neg<true>(r2[u][w] * inv, etab) : 0.0;
      o[(size_t)i * NP + j] = k;
      if (g) g[(size_t)i * NP + j] = in ? (i == j ? k + shift : k) : (i == j ? (i == n ? PAD_BIG : 1.0) : 0.0);
    }
}

// lo[b] = L^-1 of slot sl[b] (its lower triangle, rows / columns < n), up[b] = its transpose; zeros elsewhere
__global__ __launch_bounds__(256) void gkdr_linv_kernel(const double* __restrict__ Li, size_t lstride, const int* __restrict__ sl, int n, int NP,
                                                        double* __restrict__ lo, double* __restrict__ up) {
  const int b = blockIdx.y;
  const double* l = Li + (size_t)sl[b] * lstride;
  const size_t total = (size_t)NP * NP, o = (size_t)b * total;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const int i = (int)(e / NP), j = (int)(e % NP);
    lo[o + e] = (i < n && j <= i) ? l[(size_t)i * NP + j] : 0.0;
    up[o + e] = (j < n && i <= j) ? l[(size_t)j * NP + i] : 0.0;
  }
}

// C[ic[p]] = A[ia[p]] B[ib[p]]^T (index arrays null: p); operands K-major (row-major, k contiguous), rows padded to 128, K a multiple of 128.
// tri: the k range of a tile skips what is structurally zero -- TRI_A_LO: A lower triangular (k < i0 + 128), TRI_A_UP: A upper
// triangular (k >= i0), TRI_B_LO / TRI_B_UP the same for B's rows j.  The skipped products are exact zeros and the k-steps that remain
// run in the same order, so the result is that of the full product.
// EPI 1 (gKDR): the product is G = F Kx (A = F, B = Kx); C receives W = F o KK / 2 - Kx o G and T receives Kx o G (KK and Kx indexed
// like B, F like A, all with row stride ldc).
struct GemmArgs {
  const double* A = nullptr; size_t sA = 0; int lda = 0; const int* ia = nullptr;
  const double* B = nullptr; size_t sB = 0; int ldb = 0; const int* ib = nullptr;
  double* C = nullptr; size_t sC = 0; int ldc = 0; const int* ic = nullptr;
  int K = 0;
  int tri = 0;
  const double* KK = nullptr;
  double* T = nullptr; size_t sT = 0;
};

using GCfg = WCfg<128, 128, 2, 4>;
constexpr int TRI_A_LO = 1, TRI_A_UP = 2, TRI_B_LO = 4, TRI_B_UP = 8;

template <int EPI>
__global__ __launch_bounds__(GCfg::NT) void gkdr_gemm_kernel(GemmArgs g) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int p = blockIdx.z;
  const int i0 = blockIdx.y * 128, j0 = blockIdx.x * 128;
  const size_t ao = (size_t)(g.ia ? g.ia[p] : p) * g.sA, bo = (size_t)(g.ib ? g.ib[p] : p) * g.sB;
  const double* A = g.A + ao;
  const double* B = g.B + bo;
  double* C = g.C + (size_t)(g.ic ? g.ic[p] : p) * g.sC;
  int k0 = 0, k1 = g.K;
  if (g.tri & TRI_A_LO) k1 = min(k1, i0 + 128);
  if (g.tri & TRI_A_UP) k0 = max(k0, i0);
  if (g.tri & TRI_B_LO) k1 = min(k1, j0 + 128);
  if (g.tri & TRI_B_UP) k0 = max(k0, j0);
  v4d acc[GCfg::TI][GCfg::TJ];
  mainloop_w<128, 128, 2, 4>(A + (size_t)i0 * g.lda + k0, g.lda, B + (size_t)j0 * g.ldb + k0, g.ldb, max(0, k1 - k0) / BK, acc, smem);
  if (EPI == 0) {
    for_each_acc_w<4>(acc, [&](int r, int c, double x) { C[(size_t)(i0 + r) * g.ldc + j0 + c] = x; });
  } else {
    double* T = g.T + (size_t)p * g.sT;
    const double* KK = g.KK + bo;
    for_each_acc_w<4>(acc, [&](int r, int c, double x) {
      const size_t e = (size_t)(i0 + r) * g.ldc + j0 + c;
      const double t = B[e] * x;
      T[e] = t;
      C[e] = 0.5 * A[e] * KK[e] - t;
    });
  }
}

// c_j = sum_i T_ij (in order of i), W_jj += c_j / 2
__global__ __launch_bounds__(256) void gkdr_colsum_kernel(const double* __restrict__ T, double* __restrict__ W, int n, int NP) {
  const int b = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const double* t = T + (size_t)b * NP * NP;
  double c = 0.;
  for (int i = 0; i < n; ++i) c += t[(size_t)i * NP + j];
  W[(size_t)b * NP * NP + (size_t)j * NP + j] += 0.5 * c;
}

// R[p] (m x m) = (Q + Q^T) / s2 / s2, s2 = sgx2[iz[p]]
__global__ __launch_bounds__(256) void gkdr_finish_kernel(const double* __restrict__ Q, int MP, int m, const double* __restrict__ sgx2,
                                                          const int* __restrict__ iz, double* __restrict__ R) {
  const int p = blockIdx.y;
  const double s2 = sgx2[iz[p]];
  const double* q = Q + (size_t)p * MP * MP;
  const size_t total = (size_t)m * m;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const int a = (int)(e / m), c = (int)(e % m);
    R[(size_t)p * total + e] = (q[(size_t)a * MP + c] + q[(size_t)c * MP + a]) / s2 / s2;
  }
}

template <int EPI>
void gemm(const GemmArgs& g, int rows, int cols, int nb, hipStream_t s) {
  const size_t sm = (size_t)GCfg::SMEM_DOUBLES * sizeof(double);
  hipLaunchKernelGGL((gkdr_gemm_kernel<EPI>), dim3(cols / 128, rows / 128, nb), dim3(GCfg::NT), sm, s, g);
  HIPCK(hipGetLastError());
}

unsigned elem_blocks(size_t total) { return (unsigned)std::min<size_t>((total + 255) / 256, 4096); }

}  // namespace

void gkdr_R(const double* X, int n, int m, const double* y, int nx, const double* sgx2, int ny, const double* sgy2, double eps,
            int max_pairs_per_pass, double* R_out, int* info_out) {
  if (n < 1 || m < 1) throw std::runtime_error("gkdr: X must have shape (N, M) with N, M >= 1");
  if (nx < 1 || ny < 1) throw std::runtime_error("gkdr: at least one input and one output scale are needed");
  if (!(eps >= 0.0) || !std::isfinite(eps)) throw std::runtime_error("gkdr: EPS must be a finite number >= 0");
  if (max_pairs_per_pass < 0) throw std::runtime_error("gkdr: max_pairs_per_pass must be >= 0 (0 = automatic)");
  for (int i = 0; i < nx; ++i)
    if (!(sgx2[i] > 0.0) || !std::isfinite(sgx2[i])) throw std::runtime_error("gkdr: SGX^2 must be positive and finite");
  for (int i = 0; i < ny; ++i)
    if (!(sgy2[i] > 0.0) || !std::isfinite(sgy2[i])) throw std::runtime_error("gkdr: SGY^2 must be positive and finite");
  // factors and inverts A; it never sees X (the Gram kernel below stands where its covariance build would)
  ScratchFactor eng(n, nx);
  hipStream_t st = eng.stream();
  const int NP = eng.NP;
  const int MP = (m + 127) / 128 * 128;
  const size_t MS = eng.MS;
  DevBuf<double> dX((size_t)n * m);
  DevBuf<double> dY(n);
  DevBuf<double> dXt((size_t)MP * NP);
  DevBuf<double> dSx(nx);
  DevBuf<double> dSy(ny);
  DevBuf<double> dKx((size_t)nx * MS);
  HIPCK(hipMemcpyAsync(dX, X, (size_t)n * m * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCK(hipMemcpyAsync(dY, y, (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCK(hipMemcpyAsync(dSx, sgx2, (size_t)nx * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCK(hipMemcpyAsync(dSy, sgy2, (size_t)ny * sizeof(double), hipMemcpyHostToDevice, st));
  {
    // Xc^T (MP x NP, zero padding): the columns of X about their means, summed in order of the rows
    std::vector<double> xt((size_t)MP * NP, 0.0);
    for (int d = 0; d < m; ++d) {
      double mu = 0.;
      for (int i = 0; i < n; ++i) mu += X[(size_t)i * m + d];
      mu /= n;
      for (int i = 0; i < n; ++i) xt[(size_t)d * NP + i] = X[(size_t)i * m + d] - mu;
    }
    HIPCK(hipMemcpyAsync(dXt, xt.data(), xt.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCK(hipStreamSynchronize(st));
  }
  const double shift = (double)n * eps;   // N * EPS, as the reference adds it
  const int gt = NP / GT;
  const CovFill fill = [&](const BatchView& v) {
    if (v.nb != nx) throw std::runtime_error("gkdr: the factorisation must cover every input scale");
    hipLaunchKernelGGL(gkdr_gram_kernel, dim3(gt, gt, nx), dim3(256), 0, st, dX.get(), n, m, dSx.get(), nullptr, dKx.get(), NP, shift, v.A, v.MS);
    HIPCK(hipGetLastError());
  };
  std::vector<int> info;
  eng.factor(fill, info);
  std::vector<int> okx;
  for (int i = 0; i < nx; ++i) {
    info_out[i] = info[i] != 0 ? 1 : 0;
    if (!info[i]) okx.push_back(i);
  }
  const size_t RS = (size_t)m * m;
  for (int i = 0; i < nx; ++i)
    if (info[i]) std::fill(R_out + (size_t)i * ny * RS, R_out + (size_t)(i + 1) * ny * RS, std::numeric_limits<double>::quiet_NaN());
  if (okx.empty()) return;
  const int nz = (int)okx.size();
  // per factored input scale (position k of okx): L^-1 and L^-T (zero padding); per input scale Kx Kx
  DevBuf<double> dLI((size_t)nz * MS);
  DevBuf<double> dLT((size_t)nz * MS);
  DevBuf<double> dKK((size_t)nx * MS);
  DevBuf<int> dOk(nz);
  HIPCK(hipMemcpyAsync(dOk, okx.data(), nz * sizeof(int), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(gkdr_linv_kernel, dim3(elem_blocks(MS), nz), dim3(256), 0, st, eng.linv(), MS, dOk, n, NP, dLI, dLT);
  HIPCK(hipGetLastError());
  {
    GemmArgs g;
    g.A = dKx; g.sA = MS; g.lda = NP; g.ia = dOk;
    g.B = dKx; g.sB = MS; g.ldb = NP; g.ib = dOk;
    g.C = dKK; g.sC = MS; g.ldc = NP; g.ic = dOk;
    g.K = NP;
    gemm<0>(g, NP, NP, nz, st);
  }
  // pairs (input scale, output scale) of the factored input scales, row-major; processed in passes of P pairs
  std::vector<int> pz, pw, pk;
  for (int k = 0; k < nz; ++k)
    for (int w = 0; w < ny; ++w) {
      pk.push_back(k);
      pz.push_back(okx[k]);
      pw.push_back(w);
    }
  const int npairs = (int)pz.size();
  const size_t per_pair = (4 * MS + (size_t)MP * NP + (size_t)MP * MP + RS) * sizeof(double) + 3 * sizeof(int);
  int P = max_pairs_per_pass;
  if (P == 0) {
    size_t fr = 0, tot = 0;
    HIPCK(hipMemGetInfo(&fr, &tot));
    P = (int)std::max<size_t>(1, std::min<size_t>((size_t)npairs, fr / 2 / per_pair));
  }
  P = std::min(P, npairs);
  DevBuf<double> dKy((size_t)P * MS);
  DevBuf<double> dT((size_t)P * MS);
  DevBuf<double> dF((size_t)P * MS);
  DevBuf<double> dW((size_t)P * MS);
  DevBuf<double> dYt((size_t)P * MP * NP);
  DevBuf<double> dQ((size_t)P * MP * MP);
  DevBuf<double> dR((size_t)P * RS);
  DevBuf<int> dPz(P);
  DevBuf<int> dPw(P);
  DevBuf<int> dPk(P);
  for (int p0 = 0; p0 < npairs; p0 += P) {
    const int nb = std::min(P, npairs - p0);
    HIPCK(hipMemcpyAsync(dPz, pz.data() + p0, nb * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCK(hipMemcpyAsync(dPw, pw.data() + p0, nb * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCK(hipMemcpyAsync(dPk, pk.data() + p0, nb * sizeof(int), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(gkdr_gram_kernel, dim3(gt, gt, nb), dim3(256), 0, st, dY, n, 1, dSy, dPw, dKy, NP, 0.0, nullptr, (size_t)0);
    HIPCK(hipGetLastError());
    GemmArgs g;
    g.K = NP;
    g.lda = g.ldb = g.ldc = NP;
    g.sA = g.sB = g.sC = MS;
    // S = L^-1 Ky -> dT
    g.A = dLI; g.ia = dPk; g.B = dKy; g.ib = nullptr; g.C = dT; g.tri = TRI_A_LO;
    gemm<0>(g, NP, NP, nb, st);
    // S L^-T = L^-1 Ky L^-T -> dF
    g.A = dT; g.ia = nullptr; g.B = dLI; g.ib = dPk; g.C = dF; g.tri = TRI_B_LO;
    gemm<0>(g, NP, NP, nb, st);
    // P = L^-T (L^-1 Ky L^-T)^T -> dT
    g.A = dLT; g.ia = dPk; g.B = dF; g.ib = nullptr; g.C = dT; g.tri = TRI_A_UP;
    gemm<0>(g, NP, NP, nb, st);
    // F = P L^-1 -> dF
    g.A = dT; g.ia = nullptr; g.B = dLT; g.ib = dPk; g.C = dF; g.tri = TRI_B_UP;
    gemm<0>(g, NP, NP, nb, st);
    // G = F Kx -> W = F o KxKx / 2 - T, T = Kx o G
    g.A = dF; g.ia = nullptr;
    g.B = dKx; g.ib = dPz; g.tri = 0;
    g.C = dW;
    g.KK = dKK; g.T = dT; g.sT = MS;
    gemm<1>(g, NP, NP, nb, st);
    hipLaunchKernelGGL(gkdr_colsum_kernel, dim3((n + 255) / 256, nb), dim3(256), 0, st, dT, dW, n, NP);
    HIPCK(hipGetLastError());
    // Yt <- Xc^T W^T, Q <- Xc^T Yt^T = Xc^T W Xc
    GemmArgs h;
    h.K = NP;
    h.A = dXt; h.sA = 0; h.lda = NP;
    h.B = dW; h.sB = MS; h.ldb = NP;
    h.C = dYt; h.sC = (size_t)MP * NP; h.ldc = NP;
    gemm<0>(h, MP, NP, nb, st);
    h.B = dYt; h.sB = (size_t)MP * NP; h.ldb = NP;
    h.C = dQ; h.sC = (size_t)MP * MP; h.ldc = MP;
    gemm<0>(h, MP, MP, nb, st);
    hipLaunchKernelGGL(gkdr_finish_kernel, dim3(elem_blocks(RS), nb), dim3(256), 0, st, dQ, MP, m, dSx, dPz, dR);
    HIPCK(hipGetLastError());
    std::vector<double> hr((size_t)nb * RS);
    HIPCK(hipMemcpyAsync(hr.data(), dR, hr.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    for (int q = 0; q < nb; ++q) {
      const size_t pair = (size_t)pz[p0 + q] * ny + pw[p0 + q];
      std::memcpy(R_out + pair * RS, hr.data() + (size_t)q * RS, RS * sizeof(double));
    }
  }
}

}  // namespace mogp
