// Active learning (Engine::alc, Engine::predict_cov; DESIGN.md section 3 "Active learning"): the posterior covariance between two point sets,
//     c(x, x') = sigma^2 k(x, x') - v(x)^T v(x'),   v(x) = L^-1 k(x),
// and the ALC criterion built on it, ALC(c) = sum_j w_j c(r_j, c)^2 / (s^2(c) + tau).
//   alc_cross_kernel<KT, STORE>  one 128 x 128 tile of V_1^T V_2 on fp64 MFMA (fullcov_kernel's loop on two different operands), then
//                                sigma^2 k of the tile in the accumulator's own layout and x = sigma^2 k - acc;
//                                STORE: x written out; otherwise w_j x^2 summed along the tile's columns into ONE partial per row
//   alc_finish_kernel            the partials of a candidate in ascending reference-tile order, the division, the floor rule
// The m_1 x m_2 matrix of the criterion never exists.  One writer per output, fixed orders, no atomics: the same call returns the same bits,
// and neither the chunk of reference points nor the group of emulators a tile is computed in changes any.
#include "engine.h"
#include "cov_dev.h"
#include "gemm_loop_dev.h"

namespace mogp {

#define HIPCK(x) hip_check((x), #x)

namespace {

// The epilogue lives in the operand buffers of the main loop (free behind its last barrier), so that the kernel keeps two workgroups per CU:
// four 64-row coordinate blocks [ALC_DS][64] (two of the rows, two of the columns), the tile's 128 weights, and red[2][128].  A wider input
// goes in slices of ALC_DS dimensions.
constexpr int ALC_LDS = Cfg<4>::SMEM_DOUBLES;
constexpr int ALC_DS = (ALC_LDS - 128 - 256) / 256;
static_assert(4 * 64 * ALC_DS + 128 + 256 <= ALC_LDS, "the epilogue must fit the operand buffers");

// Workgroup = (slot z, row tile ti, column tile tj), row tiles fastest: neighbours in dispatch order share the column operand.
// Accumulator acc[i][j][r] of wave (wr, wc) is row wr 64 + 16 i + (lane >> 4) + 4 r, column wc 64 + 16 j + (lane & 15) of the tile: a lane
// holds 16 rows x 4 columns, and the epilogue goes through them one column block j at a time (16 squared distances live per lane).
// sigma^2 k follows the rule of the covariance kernels: inputs scaled by sqrt(e_d) at staging, the sum over ascending d with FMA,
// kern_val<KT>; KT == 2 the product form of micro_k.
template <int KT, bool STORE>
__global__ __launch_bounds__(256, 2) void alc_cross_kernel(BatchView v, const double* __restrict__ V1, int MP1, int m1,
                                                           const double* __restrict__ X1, const double* __restrict__ V2, int MP2, int m2,
                                                           const double* __restrict__ X2, const double* __restrict__ w, int nt1, int nt2,
                                                           int kend, int tile0, int tiles_r, double* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  __shared__ double etab[256];
  stage_exp_tab(etab);                  // (published by the barriers of the main loop: kend >= 16)
  int z, tile;
  decode_block(v.nb, nt1 * nt2, z, tile);
  if (z >= v.nb) return;
  const int ti = tile % nt1, tj = tile / nt1;
  const int emu = slot_to_emu(v.idx, z);
  const int D = v.D;
  const double* P = v.P + (size_t)emu * v.PS;
  const int i0 = ti * 128, j0 = tj * 128;
  v4d acc[4][4];
  gemm_mainloop<4, false, false>(V1 + (size_t)z * v.NP * MP1 + i0, MP1, V2 + (size_t)z * v.NP * MP2 + j0, MP2, kend / BK, acc, smem);

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wr = wave >> 1, wc = wave & 1;
  const int rl = lane >> 4, cl = lane & 15;
  constexpr bool SC = KT < 2;
  double* s1 = smem;                          // [2][ALC_DS][64]
  double* s2 = smem + 2 * 64 * ALC_DS;        // [2][ALC_DS][64]
  double* sw = smem + 4 * 64 * ALC_DS;        // [128]
  double* red = sw + 128;                     // [2][128]
  const double sig2 = P[D];
  if (!STORE && t < 128) sw[t] = (j0 + t < m2) ? w[j0 + t] : 0.0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    double r2[16], pk[KT == 2 ? 16 : 1];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      r2[e] = 0.0;
      // (behind the fences of the previous column block: its values are finished before this one's distances start -- left to itself the
      // compiler interleaves the blocks and spills)
      asm volatile("" : "+v"(r2[e]));
    }
    if (KT == 2) {
#pragma unroll
      for (int e = 0; e < 16; ++e) pk[KT == 2 ? e : 0] = 1.0;
    }
    for (int d0 = 0; d0 < D; d0 += ALC_DS) {
      const int ds = min(ALC_DS, D - d0);
      if (j == 0 || D > ALC_DS) {             // one slice: staged once for the four column blocks
        __syncthreads();
        stage_rows_slice<SC>(X1, m1, D, i0, d0, ds, s1, P);
        stage_rows_slice<SC>(X1, m1, D, i0 + 64, d0, ds, s1 + 64 * ALC_DS, P);
        stage_rows_slice<SC>(X2, m2, D, j0, d0, ds, s2, P);
        stage_rows_slice<SC>(X2, m2, D, j0 + 64, d0, ds, s2 + 64 * ALC_DS, P);
        __syncthreads();
      }
      const double* ci = s1 + wr * 64 * ALC_DS + rl;
      const double* rj = s2 + wc * 64 * ALC_DS + j * 16 + cl;
      for (int d = 0; d < ds; ++d) {
        const double xj = rj[d * 64];
        const double e = SC ? 1.0 : P[d0 + d];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const double df = ci[d * 64 + i * 16 + 4 * r] - xj;
            if (KT < 2) {
              r2[i * 4 + r] = __builtin_fma(df, df, r2[i * 4 + r]);
            } else {
              const double q = e * df * df;
              const double sd = sqrt(5.0 * q);
              pk[KT == 2 ? i * 4 + r : 0] *= 1.0 + sd + (5.0 / 3.0) * q;
              r2[i * 4 + r] += sd;
            }
          }
      }
    }
    const double wj = STORE ? 0.0 : sw[wc * 64 + j * 16 + cl];
    const int col = j0 + wc * 64 + j * 16 + cl;
    // four values at a time (micro_k's group_fence: an exponential has about ten live registers)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      double x[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double k = KT < 2 ? kern_val<KT>(r2[i * 4 + r], etab) : pk[KT == 2 ? i * 4 + r : 0] * lean_exp_neg<false>(r2[i * 4 + r], etab);
        x[r] = __builtin_fma(sig2, k, -acc[i][j][r]);
      }
      if (i < 3) asm volatile("" : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]), "+v"(r2[4 * i + 4]), "+v"(r2[4 * i + 5]), "+v"(r2[4 * i + 6]), "+v"(r2[4 * i + 7]));
      else asm volatile("" : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]));
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (STORE) {
          const int row = i0 + wr * 64 + i * 16 + rl + 4 * r;
          if (row < m1 && col < m2) out[((size_t)z * m1 + row) * m2 + col] = x[r];
        } else {
          acc[i][j][r] = wj * x[r] * x[r];        // the accumulator's own registers carry the weighted square
        }
      }
    }
  }
  if (STORE) return;
  // per row: the lane's four column blocks in ascending order, the 16 lanes of a row group, then the two wave columns
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int i = e >> 2, r = e & 3;
    double s = ((acc[i][0][r] + acc[i][1][r]) + acc[i][2][r]) + acc[i][3][r];
    s += __shfl_xor(s, 1);
    s += __shfl_xor(s, 2);
    s += __shfl_xor(s, 4);
    s += __shfl_xor(s, 8);
    if (cl == 0) red[wc * 128 + wr * 64 + i * 16 + rl + 4 * r] = s;
  }
  __syncthreads();
  if (t < 128) out[((size_t)z * tiles_r + tile0 + tj) * MP1 + i0 + t] = red[t] + red[128 + t];
}

__global__ __launch_bounds__(256) void alc_finish_kernel(BatchView v, int m1, int MP1, int tiles_r, const double* __restrict__ part,
                                                         double* __restrict__ var, int var_ld, const double* __restrict__ tau,
                                                         double* __restrict__ redu, int* __restrict__ deg) {
  const int z = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m1) return;
  const int emu = slot_to_emu(v.idx, z);
  double s = 0.;
  for (int g = 0; g < tiles_r; ++g) s += part[((size_t)z * tiles_r + g) * MP1 + i];
  double s2 = var[(size_t)z * var_ld + i];
  s2 = s2 < 0. ? 0. : s2;
  var[(size_t)z * var_ld + i] = s2;
  const double d = s2 + tau[z];
  const double floor_d = (double)(v.n + 2) * 0x1p-52 * v.P[(size_t)emu * v.PS + v.D];
  const bool good = d > floor_d;                // (false for NaN as well)
  redu[(size_t)z * m1 + i] = good ? s / d : 0.;
  deg[(size_t)z * m1 + i] = good ? 0 : 1;
}

template <bool STORE>
void launch_cross(const BatchView& v, const double* V1, int MP1, int m1, const double* X1, const double* V2, int MP2, int m2, const double* X2,
                  const double* w, int tile0, int tiles_r, double* out, hipStream_t s) {
  if (v.nb <= 0 || m1 <= 0 || m2 <= 0) return;
  const int nt1 = MP1 / 128, nt2 = MP2 / 128, kend = (v.n + 15) / 16 * 16;
  const long grid = (long)v.nb * nt1 * nt2;
  if (grid >= (1L << 31)) throw std::runtime_error("alc: too many tiles for one launch; use fewer points per call");
  const size_t lds = (size_t)ALC_LDS * sizeof(double);
  prof_begin("alc_cross", s);
#define CALL(K)                                                                                                                           \
  hipLaunchKernelGGL((alc_cross_kernel<K, STORE>), dim3((unsigned)grid), dim3(256), lds, s, v, V1, MP1, m1, X1, V2, MP2, m2, X2, w, nt1, nt2, \
                     kend, tile0, tiles_r, out)
  if (v.kernel_type == 0) CALL(0);
  else if (v.kernel_type == 1) CALL(1);
  else CALL(2);
#undef CALL
  HIPCK(hipGetLastError());
  prof_end("alc_cross", s, (double)v.nb * 2.0 * v.n * (double)m1 * (double)m2, 0.);
}

}  // namespace

void launch_alc_store(const BatchView& v, const double* V1, int MP1, int m1, const double* X1, const double* V2, int MP2, int m2, const double* X2,
                      double* out, hipStream_t s) {
  launch_cross<true>(v, V1, MP1, m1, X1, V2, MP2, m2, X2, nullptr, 0, 0, out, s);
}

void launch_alc_cross(const BatchView& v, const double* V1, int MP1, int m1, const double* X1, const double* V2, int MP2, int m2, const double* X2,
                      const double* w, int tile0, int tiles_r, double* part, hipStream_t s) {
  launch_cross<false>(v, V1, MP1, m1, X1, V2, MP2, m2, X2, w, tile0, tiles_r, part, s);
}

void launch_alc_finish(const BatchView& v, int m1, int MP1, int tiles_r, const double* part, double* var, int var_ld, const double* tau,
                       double* red, int* deg, hipStream_t s) {
  if (v.nb <= 0 || m1 <= 0) return;
  hipLaunchKernelGGL(alc_finish_kernel, dim3((m1 + 255) / 256, v.nb), dim3(256), 0, s, v, m1, MP1, tiles_r, part, var, var_ld, tau, red, deg);
  HIPCK(hipGetLastError());
}

}  // namespace mogp
