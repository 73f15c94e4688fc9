// Active learning (alc, predict_cov; DESIGN.md section 3 "Active learning"): the posterior covariance between two point sets,
//     c(x, x') = sigma^2 k(x, x') - v(x)^T v(x'),   v(x) = L^-1 k(x),
// and the ALC criterion built on it, ALC(c) = sum_j w_j c(r_j, c)^2 / (s^2(c) + tau).
//   alc_cross_kernel<KT, STORE>  one 128 x 128 tile of V_1^T V_2 on fp64 MFMA (fullcov_kernel's loop on two different operands), then
//                                sigma^2 k of the tile in the accumulator's own layout and x = sigma^2 k - acc;
//                                STORE: x written out; otherwise w_j x^2 summed along the tile's columns into ONE partial per row
//   alc_finish_kernel            the partials of a candidate in ascending reference-tile order, the division, the floor rule
// and, for greedy batches (AlcBatch; DESIGN.md section 3 "Active learning: batches"), the conditioning on a pick: a run at p with noise
// tau gives every stored v(x) one more entry u(x) = c(x, p) / sqrt(s^2(p) + tau), so V carries room for those rows behind its base rows and
// alc_cross_kernel takes the rows per slot and the end of its K range from its caller:
//   alc_argmax_kernel            per slot the unmasked candidate with the largest score (ties: the lowest index), the stopping rule, the mask
//   alc_condition_kernel<KT>     row n16 + t of V of one point set and its tracked variances; bandwidth bound, one owner per output
// The m_1 x m_2 matrix of the criterion never exists.  One writer per output, fixed orders, no atomics: the same call returns the same bits,
// and neither the chunk of reference points nor the group of emulators a tile is computed in changes any.
#include "launch.h"
#include "devmem.h"
#include "cov_dev.h"
#include "gemm_loop_dev.h"

namespace mogp {

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
                                                           int rows, int kend, int tile0, int tiles_r, double* __restrict__ out) {
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
  gemm_mainloop<4, false, false>(V1 + (size_t)z * rows * MP1 + i0, MP1, V2 + (size_t)z * rows * MP2 + j0, MP2, kend / BK, acc, smem);

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

__global__ __launch_bounds__(256) void alc_finish_kernel(BatchView v, int nrows, int m1, int MP1, int tiles_r, const double* __restrict__ part,
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
  const double floor_d = (double)(nrows + 2) * 0x1p-52 * v.P[(size_t)emu * v.PS + v.D];
  const bool good = d > floor_d;                // (false for NaN as well)
  redu[(size_t)z * m1 + i] = good ? s / d : 0.;
  deg[(size_t)z * m1 + i] = good ? 0 : 1;
}

// ---- greedy batches: the pick of a step and the rank-one update it brings (launch.h has the contracts) -------------------------------------

// (value, index) pairs ordered by the larger value, then the lower index: the order of a reduction over them changes nothing
__device__ __forceinline__ void take_better(double& bv, int& bi, double ov, int oi) {
  if (ov > bv || (ov == bv && oi < bi)) {
    bv = ov;
    bi = oi;
  }
}

constexpr int ALC_NO_PICK = 0x7fffffff;

// One workgroup per slot: a strided scan (ascending indices per thread, strict >: the lowest index of equal scores; a NaN compares false
// and never wins), a 64-lane butterfly, the four waves through LDS; thread 0 applies the stopping rule and writes the step's words.
__global__ __launch_bounds__(256) void alc_argmax_kernel(BatchView v, int t, int T, int forced, int m, const double* __restrict__ red,
                                                         const double* __restrict__ var, int var_ld, const double* __restrict__ tau,
                                                         int* __restrict__ mask, int* __restrict__ picks, double* __restrict__ pick_red,
                                                         double* __restrict__ pick_d) {
  __shared__ double sv[4];
  __shared__ int si[4];
  const int z = blockIdx.x, tid = threadIdx.x;
  const double* r = red + (size_t)z * m;
  int* mk = mask + (size_t)z * m;
  double bv = -INFINITY;
  int bi = ALC_NO_PICK;
  if (forced < 0) {
    for (int i = tid; i < m; i += 256) {
      const double x = r[i];
      if (mk[i] == 0 && x > bv) {
        bv = x;
        bi = i;
      }
    }
    for (int o = 1; o < 64; o <<= 1) {
      const double ov = __shfl_xor(bv, o);
      const int oi = __shfl_xor(bi, o);
      take_better(bv, bi, ov, oi);
    }
    if ((tid & 63) == 0) {
      sv[tid >> 6] = bv;
      si[tid >> 6] = bi;
    }
    __syncthreads();
  }
  if (tid != 0) return;
  if (forced >= 0) {
    bi = forced < m ? forced : ALC_NO_PICK;
    bv = forced < m ? r[forced] : 0.;
  } else {
    for (int w = 1; w < 4; ++w) take_better(bv, bi, sv[w], si[w]);
  }
  bool ok = bi != ALC_NO_PICK;
  double d = 1.;
  if (ok) {
    const int emu = slot_to_emu(v.idx, z);
    double s2 = var[(size_t)z * var_ld + bi];
    s2 = s2 < 0. ? 0. : s2;
    d = s2 + tau[z];
    const double floor_d = (double)(v.n + t + 2) * 0x1p-52 * v.P[(size_t)emu * v.PS + v.D];
    ok = (forced >= 0 || bv > 0.) && d > floor_d;           // (false for NaN as well)
    mk[bi] = 1;
  }
  picks[(size_t)z * T + t] = ok ? bi : -1;
  pick_red[(size_t)z * T + t] = ok ? bv : 0.;
  pick_d[(size_t)z * T + t] = ok ? d : 1.;
}

// Workgroup = (64 points, slot): lane = point, so a row of V is one 512-byte run per wave; the K range goes through LDS in chunks of
// ALC_KC entries of column p (gathered once per workgroup), each chunk in four contiguous quarters, one per wave, every quarter in ascending
// k with FMA; the four partial sums meet in LDS in wave order.  Wave 0 then forms sigma^2 k(x, x_p) by the rule of the covariance kernels
// (inputs scaled by sqrt(e_d), ascending d with FMA, kern_val<KT>; KT == 2 the product form), divides and writes row n16 + t and s^2.
// V and Vc are the same buffer when the candidates themselves are updated (rows below n16 + t are read, row n16 + t is written): no restrict.
constexpr int ALC_KC = 2048;
template <int KT>
__global__ __launch_bounds__(256) void alc_condition_kernel(BatchView v, int t, int T, int rows, const int* __restrict__ picks,
                                                            const double* __restrict__ pick_d, const double* Vc, int MPc,
                                                            const double* __restrict__ Xc, double* V, int MP, int m,
                                                            const double* __restrict__ X, double* __restrict__ var, int var_ld) {
  __shared__ double colp[ALC_KC];
  __shared__ double part[4][64];
  const int z = blockIdx.y;
  const int p = picks[(size_t)z * T + t];
  if (p < 0) return;                              // (the whole workgroup: nothing was picked in this slot)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int x = blockIdx.x * 64 + lane;           // < MP: the grid has MP / 64 workgroups per slot
  const int K = (v.n + 15) / 16 * 16 + t;         // rows [0, K) are written; row K is this step's
  const double* Vz = V + (size_t)z * rows * MP + x;
  const double* Vcz = Vc + (size_t)z * rows * MPc + p;
  double s = 0.;
  for (int k0 = 0; k0 < K; k0 += ALC_KC) {
    const int kc = min(ALC_KC, K - k0);
    __syncthreads();
    for (int k = tid; k < kc; k += 256) colp[k] = Vcz[(size_t)(k0 + k) * MPc];
    __syncthreads();
    const int q4 = (kc + 3) / 4, ka = wave * q4, kb = min(kc, ka + q4);
    const double* vp = Vz + (size_t)(k0 + ka) * MP;
#pragma unroll 8
    for (int k = ka; k < kb; ++k) {
      s = __builtin_fma(vp[0], colp[k], s);
      vp += MP;
    }
  }
  part[wave][lane] = s;
  __syncthreads();
  if (wave != 0 || x >= m) return;
  const double dot = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
  const int emu = slot_to_emu(v.idx, z);
  const int D = v.D;
  const double* P = v.P + (size_t)emu * v.PS;
  const double* xi = X + (size_t)x * D;
  const double* xp = Xc + (size_t)p * D;
  double r2 = 0., pk = 1.;
  for (int d = 0; d < D; ++d) {
    if (KT < 2) {
      const double sc = sqrt(P[d]);
      const double df = xi[d] * sc - xp[d] * sc;
      r2 = __builtin_fma(df, df, r2);
    } else {
      const double df = xi[d] - xp[d];
      const double q = P[d] * df * df;
      const double sd = sqrt(5.0 * q);
      pk *= 1.0 + sd + (5.0 / 3.0) * q;
      r2 += sd;
    }
  }
  const double k = KT < 2 ? kern_val<(KT < 2 ? KT : 0)>(r2, EXP_TAB_G) : pk * lean_exp_neg<false>(r2, EXP_TAB_G);
  const double u = __builtin_fma(P[D], k, -dot) / sqrt(pick_d[(size_t)z * T + t]);
  V[((size_t)z * rows + K) * MP + x] = u;
  var[(size_t)z * var_ld + x] -= u * u;
}

template <bool STORE>
void launch_cross(const BatchView& v, const double* V1, int MP1, int m1, const double* X1, const double* V2, int MP2, int m2, const double* X2,
                  const double* w, int rows, int kend, int tile0, int tiles_r, double* out, hipStream_t s) {
  if (v.nb <= 0 || m1 <= 0 || m2 <= 0) return;
  const int nt1 = MP1 / 128, nt2 = MP2 / 128;
  const long grid = (long)v.nb * nt1 * nt2;
  if (grid >= (1L << 31)) throw std::runtime_error("alc: too many tiles for one launch; use fewer points per call");
  const size_t lds = (size_t)ALC_LDS * sizeof(double);
  prof_begin("alc_cross", s);
#define CALL(K)                                                                                                                           \
  hipLaunchKernelGGL((alc_cross_kernel<K, STORE>), dim3((unsigned)grid), dim3(256), lds, s, v, V1, MP1, m1, X1, V2, MP2, m2, X2, w, nt1, nt2, \
                     rows, kend, tile0, tiles_r, out)
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
  launch_cross<true>(v, V1, MP1, m1, X1, V2, MP2, m2, X2, nullptr, v.NP, alc_kend(v.n), 0, 0, out, s);
}

void launch_alc_cross(const BatchView& v, const double* V1, int MP1, int m1, const double* X1, const double* V2, int MP2, int m2, const double* X2,
                      const double* w, int rows, int kend, int tile0, int tiles_r, double* part, hipStream_t s) {
  if (rows < kend || kend % 16 || kend < 16) throw std::runtime_error("alc: the K range must be whole 16-row steps inside a slot");
  launch_cross<false>(v, V1, MP1, m1, X1, V2, MP2, m2, X2, w, rows, kend, tile0, tiles_r, part, s);
}

void launch_alc_finish(const BatchView& v, int nrows, int m1, int MP1, int tiles_r, const double* part, double* var, int var_ld, const double* tau,
                       double* red, int* deg, hipStream_t s) {
  if (v.nb <= 0 || m1 <= 0) return;
  hipLaunchKernelGGL(alc_finish_kernel, dim3((m1 + 255) / 256, v.nb), dim3(256), 0, s, v, nrows, m1, MP1, tiles_r, part, var, var_ld, tau, red, deg);
  HIPCK(hipGetLastError());
}

void launch_alc_argmax(const BatchView& v, int t, int T, int forced, int m, const double* red, const double* var, int var_ld, const double* tau,
                       int* mask, int* picks, double* pick_red, double* pick_d, hipStream_t s) {
  if (v.nb <= 0 || m <= 0) return;
  if (t < 0 || t >= T || forced >= m) throw std::runtime_error("alc_batch: a step or a forced pick outside its range");
  hipLaunchKernelGGL(alc_argmax_kernel, dim3(v.nb), dim3(256), 0, s, v, t, T, forced, m, red, var, var_ld, tau, mask, picks, pick_red, pick_d);
  HIPCK(hipGetLastError());
}

void launch_alc_condition(const BatchView& v, int t, int T, int rows, const int* picks, const double* pick_d, const double* Vc, int MPc,
                          const double* Xc, double* V, int MP, int m, const double* X, double* var, int var_ld, hipStream_t s) {
  if (v.nb <= 0 || m <= 0) return;
  if (t < 0 || t >= T || alc_kend(v.n) + t >= rows || MP % 64 || m > MP || v.nb > 65535)
    throw std::runtime_error("alc_batch: a conditioning row outside the slot");
  prof_begin("alc_condition", s);
#define CALL(K)                                                                                                                               \
  hipLaunchKernelGGL((alc_condition_kernel<K>), dim3(MP / 64, v.nb), dim3(256), 0, s, v, t, T, rows, picks, pick_d, Vc, MPc, Xc, V, MP, m, X, \
                     var, var_ld)
  if (v.kernel_type == 0) CALL(0);
  else if (v.kernel_type == 1) CALL(1);
  else CALL(2);
#undef CALL
  HIPCK(hipGetLastError());
  prof_end("alc_condition", s, (double)v.nb * 2.0 * (alc_kend(v.n) + t) * (double)m, (double)v.nb * 8.0 * (alc_kend(v.n) + t) * ((double)MP + 1.0));
}

}  // namespace mogp
