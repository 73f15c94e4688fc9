// The kernels of the pathwise posterior draws (engine_rff.hip; DESIGN.md section 3 "Pathwise posterior draws") and their launchers: the
// product of a random-Fourier-feature matrix that is generated and never stored with a panel of weights, the weights' and the noise's
// normals, and the right-hand sides of the solves.  A panel is a set of columns stored one after another, entry (i, c) at [c * ld + i].
//
//   rff_kernel           Out = amp Phi(P) W with Phi_if = cos(t_if), t_if = b_f then fma(omega_fd, P_id, t) over d ascending.  The tiling and the
//                        lane layout are kgen_sweep's (kernels_iter.hip): a workgroup of four waves owns 64 points, a wave 16 of them, and sweeps
//                        the features f in ascending tiles of 64 whose frequencies (D x 64), phases and rows of W (64 x (16 NB + 1)) are staged
//                        in LDS.  One v_mfma_f64_16x16x4_f64 takes 16 points x 4 features as its A operand -- one cosine per lane, generated
//                        by that lane -- and 4 rows of W x 16 columns as its B operand.  No atomics and no split of f across workgroups: the
//                        sum of a row runs over f in one fixed order, and the MFMA keeps its columns apart.  Entries of rows >= M and of
//                        features >= F are exact zeros; amp multiplies once, in the store.
//   rff_inderiv_kernel   Out = d/dx_d [amp Phi(P) W] = -amp s_d sum_f sin(t_if) omega_fd W_f for a group of INDERIV_DG dimensions per workgroup: the
//                        same tiling and the same argument, the sine as the A operand shared by the dimensions, omega_fd W_fc as the B operand
//   rff_normals_kernel   W[c][f] = normal(seed, stream, draw0 + c, f) of philox_dev.h, one thread per pair of features
//   rff_rhs_kernel       B[c][i] = y_i - g[c][i] - root * noise, one row per thread; the noise is the panel E or, without one,
//                        normal(seed, stream, draw0 + c, i); columns >= cols are exact zeros
// Every launch is a plain grid that ends by itself.
#include "cov_dev.h"
#include "philox_dev.h"
#include "predict_plan.h"

namespace mogp {

namespace {

typedef double v4d __attribute__((ext_vector_type(4)));

constexpr int RF_ROWS = 64;             // points of a workgroup and features of a staged tile

// dynamic LDS of rff_kernel: sa (D x 64) | so (D x 64) | sp (64) | sv (64 x (16 nb + 1)); below kgen_lds_bytes(D, nb) by the table's 192 doubles
constexpr size_t rff_lds_bytes(int D, int nb) { return sizeof(double) * ((size_t)2 * RF_ROWS * D + RF_ROWS + (size_t)RF_ROWS * (16 * nb + 1)); }

template <int NB>
__global__ __launch_bounds__(256) void rff_kernel(const double* __restrict__ Ps, int M, const double* __restrict__ Om, const double* __restrict__ Ph,
                                                  int F, int D, const double* __restrict__ W, size_t ldw, double amp, double* __restrict__ Out,
                                                  size_t ldo) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  constexpr int LDV = 16 * NB + 1;      // odd row stride of the staged rows of W
  double* sa = sm;
  double* so = sa + (size_t)RF_ROWS * D;
  double* sp = so + (size_t)RF_ROWS * D;
  double* sv = sp + RF_ROWS;
  const int t = threadIdx.x, lane = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int i0 = blockIdx.x * RF_ROWS;
  const int il = w * 16 + (lane & 15), jq = lane >> 4, cl = lane & 15;
  const int gi = i0 + il;
  stage_rows(Ps, M, D, i0, sa);
  v4d acc[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) acc[b] = v4d{0.0, 0.0, 0.0, 0.0};
  for (int f0 = 0; f0 < F; f0 += RF_ROWS) {
    __syncthreads();                                         // the previous tile has been read
    stage_rows(Om, F, D, f0, so);
    if (t < RF_ROWS) sp[t] = (f0 + t < F) ? Ph[f0 + t] : 0.0;
    for (int e = t; e < RF_ROWS * 16 * NB; e += 256) {
      const int f = e & 63, c = e >> 6;
      sv[f * LDV + c] = (f0 + f < F) ? W[(size_t)c * ldw + (size_t)(f0 + f)] : 0.0;
    }
    __syncthreads();
#pragma unroll 1
    for (int g = 0; g < 4; ++g) {                            // 16 features: four MFMA steps of four
      double ph[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) ph[u] = sp[(g * 4 + u) * 4 + jq];
      for (int d = 0; d < D; ++d) {
        const double a = sa[d * 64 + il];
#pragma unroll
        for (int u = 0; u < 4; ++u) ph[u] = __builtin_fma(so[d * 64 + (g * 4 + u) * 4 + jq], a, ph[u]);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int fl = (g * 4 + u) * 4 + jq;
        double cv = cos(ph[u]);
        if (f0 + fl >= F || gi >= M) cv = 0.0;
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(cv, sv[fl * LDV + b * 16 + cl], acc[b], 0, 0, 0);
      }
    }
  }
  // register reg of a C fragment is row i0 + 16 w + jq + 4 reg, column cl
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int i = i0 + w * 16 + jq + 4 * reg;
      if (i < M) Out[(size_t)(b * 16 + cl) * ldo + (size_t)i] = amp * acc[b][reg];
    }
}

// Out[(d * 16 NB + c) * ldo + i] = -amp s_d sum_f sin(t_if) (omega_fd W_fc): rff_kernel with the sine of the same argument -- t_if built by the
// same FMAs in the same order -- as the A operand, which the DG dimensions of group blockIdx.y share: the columns (d, c) of the operand
// omega_fd W_fc are just more column blocks.  The operand's entry is one rounded product of the staged frequency and the staged weight, formed
// by the lane that feeds it to the MFMA (staging the products would take 64 x 16 NB DG doubles of LDS, 131 KB, for the same bits); the
// sines are never stored.  A group repeats the arguments and the sines.  -amp s_d multiplies once, in the store.  LDS: rff_lds_bytes(D, NB).
template <int NB, int DG>
__global__ __launch_bounds__(256, 2) void rff_inderiv_kernel(const double* __restrict__ Ps, int M, const double* __restrict__ Om,
                                                          const double* __restrict__ Ph, int F, int D, const double* __restrict__ W, size_t ldw,
                                                          double amp, const double* __restrict__ scale, double* __restrict__ Out, size_t ldo) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  constexpr int LDV = 16 * NB + 1;
  double* sa = sm;
  double* so = sa + (size_t)RF_ROWS * D;
  double* sp = so + (size_t)RF_ROWS * D;
  double* sv = sp + RF_ROWS;
  const int t = threadIdx.x, lane = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int i0 = blockIdx.x * RF_ROWS, d0 = blockIdx.y * DG;
  const int il = w * 16 + (lane & 15), jq = lane >> 4, cl = lane & 15;
  const int gi = i0 + il;
  stage_rows(Ps, M, D, i0, sa);
  v4d acc[DG][NB];
#pragma unroll
  for (int dd = 0; dd < DG; ++dd)
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[dd][b] = v4d{0.0, 0.0, 0.0, 0.0};
  for (int f0 = 0; f0 < F; f0 += RF_ROWS) {
    __syncthreads();                                         // the previous tile has been read
    stage_rows(Om, F, D, f0, so);
    if (t < RF_ROWS) sp[t] = (f0 + t < F) ? Ph[f0 + t] : 0.0;
    for (int e = t; e < RF_ROWS * 16 * NB; e += 256) {
      const int f = e & 63, c = e >> 6;
      sv[f * LDV + c] = (f0 + f < F) ? W[(size_t)c * ldw + (size_t)(f0 + f)] : 0.0;
    }
    __syncthreads();
#pragma unroll 1
    for (int g = 0; g < 4; ++g) {                            // 16 features: four MFMA steps of four
      double ph[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) ph[u] = sp[(g * 4 + u) * 4 + jq];
      for (int d = 0; d < D; ++d) {
        const double a = sa[d * 64 + il];
#pragma unroll
        for (int u = 0; u < 4; ++u) ph[u] = __builtin_fma(so[d * 64 + (g * 4 + u) * 4 + jq], a, ph[u]);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int fl = (g * 4 + u) * 4 + jq;
        double sn = sin(ph[u]);
        if (f0 + fl >= F || gi >= M) sn = 0.0;
        double wv[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) wv[b] = sv[fl * LDV + b * 16 + cl];
#pragma unroll
        for (int dd = 0; dd < DG; ++dd) {
          if (d0 + dd < D) {                                 // (the same for the whole workgroup)
            const double om = so[(d0 + dd) * 64 + fl];
#pragma unroll
            for (int b = 0; b < NB; ++b) acc[dd][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(sn, om * wv[b], acc[dd][b], 0, 0, 0);
          }
        }
      }
    }
  }
  // register reg of a C fragment is row i0 + 16 w + jq + 4 reg, column cl
#pragma unroll
  for (int dd = 0; dd < DG; ++dd) {
    if (d0 + dd < D) {
      const double coef = -(amp * scale[d0 + dd]);
#pragma unroll
      for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int i = i0 + w * 16 + jq + 4 * reg;
          if (i < M) Out[((size_t)(d0 + dd) * (16 * NB) + (size_t)(b * 16 + cl)) * ldo + (size_t)i] = coef * acc[dd][b][reg];
        }
    }
  }
}

__global__ __launch_bounds__(256) void rff_normals_kernel(unsigned long long seed, unsigned stream, unsigned draw0, int n, double* __restrict__ W,
                                                          size_t ldw) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (2 * p >= n) return;
  double z0, z1;
  philox_normal_pair(seed, stream, draw0 + blockIdx.y, (uint32_t)p, z0, z1);
  double* col = W + (size_t)blockIdx.y * ldw;
  col[2 * p] = z0;
  if (2 * p + 1 < n) col[2 * p + 1] = z1;
}

__global__ __launch_bounds__(256) void rff_rhs_kernel(const double* __restrict__ y, const double* __restrict__ g, const double* __restrict__ E, int N,
                                                      int cols, double root, unsigned long long seed, unsigned stream, unsigned draw0,
                                                      double* __restrict__ B) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const int c = blockIdx.y;
  const size_t o = (size_t)c * N + i;
  if (c >= cols) {
    B[o] = 0.0;
    return;
  }
  double z;
  if (E) {
    z = E[o];
  } else {
    double z0, z1;
    philox_normal_pair(seed, stream, draw0 + c, (uint32_t)(i >> 1), z0, z1);
    z = (i & 1) ? z1 : z0;
  }
  B[o] = __builtin_fma(-root, z, y[i] - g[o]);
}

inline unsigned rf_blocks(long n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

void launch_rff(const double* Ps, long M, const double* omega, const double* phase, int F, int D, const double* W, long ldw, int nb, double amp,
                double* Out, long ldo, hipStream_t st) {
  if (M < 1 || F < 1) return;
  prof_begin("rff", st);
  hipLaunchKernelGGL(nb == 1 ? rff_kernel<1> : rff_kernel<2>, dim3(rf_blocks(M, RF_ROWS)), dim3(256), rff_lds_bytes(D, nb), st, Ps, (int)M, omega, phase,
                     F, D, W, (size_t)ldw, amp, Out, (size_t)ldo);
  // algorithmic: per entry 2 D operations of the argument and ~40 of the cosine, then 2 per column; the staged tiles are read once per workgroup
  prof_end("rff", st, (double)M * (double)F * (2.0 * D + 40.0 + 32.0 * nb), 8.0 * (double)rf_blocks(M, RF_ROWS) * (double)F * (D + 1.0 + 16.0 * nb));
}

void launch_rff_inderiv(const double* Ps, long M, const double* omega, const double* phase, int F, int D, const double* W, long ldw, int nb, double amp,
                        const double* scale, double* Out, long ldo, hipStream_t st) {
  if (M < 1 || F < 1) return;
  const unsigned groups = rf_blocks(D, INDERIV_DG);
  prof_begin("rff_inderiv", st);
  const auto kern = nb == 1 ? rff_inderiv_kernel<1, INDERIV_DG> : rff_inderiv_kernel<2, INDERIV_DG>;
  hipLaunchKernelGGL(kern, dim3(rf_blocks(M, RF_ROWS), groups), dim3(256), rff_lds_bytes(D, nb), st, Ps, (int)M, omega, phase, F, D, W, (size_t)ldw, amp, scale, Out, (size_t)ldo);
  // algorithmic: every group of dimensions forms its arguments and sines again (2 D and ~40), then per dimension and column 1 of the operand and 2
  prof_end("rff_inderiv", st, (double)M * (double)F * (groups * (2.0 * D + 40.0) + D * 48.0 * nb),
           8.0 * (double)rf_blocks(M, RF_ROWS) * (double)F * groups * (D + 1.0 + 16.0 * nb));
}

void launch_rff_normals(unsigned long long seed, unsigned stream, unsigned draw0, int cols, long n, double* W, long ldw, hipStream_t st) {
  if (cols < 1 || n < 1) return;
  hipLaunchKernelGGL(rff_normals_kernel, dim3(rf_blocks((n + 1) / 2, 256), cols), dim3(256), 0, st, seed, stream, draw0, (int)n, W, (size_t)ldw);
}

void launch_rff_rhs(const double* y, const double* g, const double* E, long N, int cols, double root, unsigned long long seed, unsigned stream,
                    unsigned draw0, double* B, hipStream_t st) {
  hipLaunchKernelGGL(rff_rhs_kernel, dim3(rf_blocks(N, 256), ITER_PLAN_COLS), dim3(256), 0, st, y, g, E, (int)N, cols, root, seed, stream, draw0, B);
}

}  // namespace mogp
