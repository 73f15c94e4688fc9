// Optimised maximin Latin hypercubes: column-swap threshold accepting on Morris & Mitchell's phi (DESIGN.md section 3 "Design").  Every bit
// of a chain is specified, so that tests/lhs_restate.py restates it in NumPy:
//   state      P (n, D) integer levels, every column a permutation of 0 .. n-1;  R_ij = sum_d (P_id - P_jd)^2, exact in 64-bit integers
//   g(R)       x = (double)R;  q - 1 times x = x * R (rounded, left to right);  g = 1.0 / x (IEEE division).  No pow, no FMA
//   proposal t of chain c: philox4x32_10(t & 0xffffffff, t >> 32, stream + c, 0; seed) -> d = (w0 D) >> 32, a = (w1 n) >> 32,
//              b = (w2 (n - 1)) >> 32, b += (b >= a), u = w3 2^-32; rows a and b exchange their entries of column d
//   Delta      term_j = (g(R'_aj) - g(R_aj)) + (g(R'_bj) - g(R_bj)) for j not in {a, b}.  Summing thread k of 256 adds its terms j = k, k + 256, ...
//              in ascending j to 0.0; every wave of 64 halves its lanes six times (lane i += lane i + 32, 16, 8, 4, 2, 1);
//              Delta = (w0 + w1) + (w2 + w3) of the four wave sums
//   accept     iff Delta <= (theta u) Phi_cur;  then Phi_cur += Delta.  theta *= rho after every `stage` proposals
//   best       the state of smallest running Phi_cur (strictly smaller replaces: the first on a tie), kept in global memory
//   Phi(P)     from scratch: rows sorted by their level in column 0 (l = 0 .. n-1); row sum r_l = sum over m = l+1 .. n-1, ascending, from 0.0,
//              of g(R_lm); Phi = the same thread-strided sum and tree over r_0 .. r_{n-1}.  Computed by kernels of their own over many
//              workgroups: it is needed twice per chain (start and best), not per proposal.
// One workgroup per chain, persistent over all proposals, P in LDS (layout and limits: lhs_plan.h).  Nothing crosses workgroups.
#include <algorithm>
#include <climits>
#include <stdexcept>
#include <string>
#include <vector>

#include "engine.h"
#include "lhs_plan.h"
#include "philox_dev.h"

namespace mogp {

namespace {

__device__ __forceinline__ double lhs_g(long long R, int q) {
#pragma clang fp contract(off)
  const double r = (double)R;            // exact: R < 2^53
  double x = r;
  for (int k = 1; k < q; ++k) x = x * r;
  return 1.0 / x;
}

template <bool WIDE>
__device__ __forceinline__ int lv_get(const unsigned short* lo, const unsigned* hi, int idx) {
  int v = lo[idx];
  if (WIDE) v |= (int)((hi[idx >> 5] >> (idx & 31)) & 1u) << 16;
  return v;
}

// one thread at a time per 32 cells (the bit plane is read, changed and written back)
template <bool WIDE>
__device__ __forceinline__ void lv_set(unsigned short* lo, unsigned* hi, int idx, int v) {
  lo[idx] = (unsigned short)v;
  if (WIDE) {
    const unsigned bit = 1u << (idx & 31), w = hi[idx >> 5];
    hi[idx >> 5] = (v >> 16) ? (w | bit) : (w & ~bit);
  }
}

// the sum of a wave's 64 values in lane 0, in the fixed order of the head of the file
__device__ __forceinline__ double wave_tree(double s) {
#pragma clang fp contract(off)
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s = s + __shfl_down(s, off, 64);
  return s;
}

// The chain's workgroup has LHS_HW = 1024 hardware threads (16 waves, four per SIMD: the dependent chains of the fp64 division need the
// other waves to hide behind), but the sum keeps the order of 256 summing threads: hardware thread h computes the term of row
// j = k + 256 (4 batch + part), k = h & 255, part = h >> 8, and the threads of part 0 add the four terms of their k in ascending j --
// their own and three read from LDS (a row that takes no part contributes +0.0, which changes no partial sum: none is -0.0).  The term
// buffer alternates between two halves, so one barrier per batch is enough: a half is written again only after the barrier that its
// readers reach after reading.
template <bool WIDE, bool SMALL>
__global__ __launch_bounds__(LHS_HW) void lhs_anneal_kernel(const int* __restrict__ start, int n, int D, long long n_steps, int q,
                                                            double theta0, double rho, long long stage, uint32_t k0, uint32_t k1,
                                                            uint32_t stream0, const double* __restrict__ phi_start, int hi_offset,
                                                            int* __restrict__ best, long long* __restrict__ accepted) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) unsigned char lhs_sm[];
  __shared__ double wsum[2][LHS_THREADS / 64];
  __shared__ double tbuf[2][LHS_HW / LHS_THREADS - 1][LHS_THREADS];
  unsigned short* lo = reinterpret_cast<unsigned short*>(lhs_sm);
  unsigned* hi = reinterpret_cast<unsigned*>(lhs_sm + hi_offset);
  const int tid = threadIdx.x, k = tid & (LHS_THREADS - 1), part = tid >> 8, c = blockIdx.x, nd = n * D;
  const int* S = start + (size_t)c * nd;
  int* B = best + (size_t)c * nd;
  if (WIDE) {
    for (int w = tid; w < (nd + 31) / 32; w += LHS_HW) {
      unsigned bits = 0;
      for (int i = 0; i < 32; ++i) {
        const int idx = 32 * w + i;
        if (idx < nd) {
          const int v = S[(idx % n) * D + idx / n];
          lo[idx] = (unsigned short)v;
          bits |= (unsigned)((v >> 16) & 1) << i;
        }
      }
      hi[w] = bits;
    }
  } else {
    for (int j = tid; j < n; j += LHS_HW)
      for (int d = 0; d < D; ++d) lo[d * n + j] = (unsigned short)S[j * D + d];
  }
  for (int idx = tid; idx < nd; idx += LHS_HW) B[idx] = S[idx];
  __syncthreads();

  const int batches = (n + LHS_HW - 1) / LHS_HW;
  double phi = phi_start[c], best_phi = phi, theta = theta0;
  long long acc = 0, left = stage;
  int slot = 0;
  for (long long t = 0; t < n_steps; ++t) {
    const PhiloxWords w = philox4x32_10((uint32_t)t, (uint32_t)((unsigned long long)t >> 32), stream0 + (uint32_t)c, 0u, k0, k1);
    const int d = (int)(((uint64_t)w.x[0] * (uint64_t)D) >> 32);
    const int a = (int)(((uint64_t)w.x[1] * (uint64_t)n) >> 32);
    int b = (int)(((uint64_t)w.x[2] * (uint64_t)(n - 1)) >> 32);
    b += (b >= a);
    const double u = (double)w.x[3] * 2.3283064365386962890625e-10;      // 2^-32, exact
    const int pad = lv_get<WIDE>(lo, hi, d * n + a), pbd = lv_get<WIDE>(lo, hi, d * n + b);
    double s = 0.0;
    for (int bi = 0; bi < batches; ++bi) {
      const int j = k + LHS_THREADS * (4 * bi + part);
      double term = 0.0;
      if (j < n && j != a && j != b) {
        long long Ra, Rb;
        if (SMALL) {                // D (n - 1)^2 < 2^32: the sums fit 32 bits, the products of differences below 2^23 the 24-bit multiplier
          unsigned ra = 0, rb = 0;
          for (int dd = 0; dd < D; ++dd) {
            const int pj = lv_get<WIDE>(lo, hi, dd * n + j);
            const int da = lv_get<WIDE>(lo, hi, dd * n + a) - pj, db = lv_get<WIDE>(lo, hi, dd * n + b) - pj;
            ra += (unsigned)__mul24(da, da);
            rb += (unsigned)__mul24(db, db);
          }
          Ra = ra;
          Rb = rb;
        } else {
          Ra = 0;
          Rb = 0;
          for (int dd = 0; dd < D; ++dd) {
            const int pj = lv_get<WIDE>(lo, hi, dd * n + j);
            const int da = lv_get<WIDE>(lo, hi, dd * n + a) - pj, db = lv_get<WIDE>(lo, hi, dd * n + b) - pj;
            Ra += (long long)da * da;
            Rb += (long long)db * db;
          }
        }
        const int pj = lv_get<WIDE>(lo, hi, d * n + j);
        const int ea = pad - pj, eb = pbd - pj;
        const long long qa = (long long)ea * ea, qb = (long long)eb * eb;
        const long long Ra2 = Ra - qa + qb, Rb2 = Rb - qb + qa;          // row a now holds b's entry of column d, and b a's
        term = (lhs_g(Ra2, q) - lhs_g(Ra, q)) + (lhs_g(Rb2, q) - lhs_g(Rb, q));
      }
      if (part) tbuf[slot][part - 1][k] = term;
      __syncthreads();
      if (part == 0) {
        s = s + term;
#pragma unroll
        for (int pp = 0; pp < LHS_HW / LHS_THREADS - 1; ++pp) s = s + tbuf[slot][pp][k];
      }
      slot ^= 1;
    }
    const int buf = (int)(t & 1);
    if (part == 0) {
      s = wave_tree(s);
      if ((tid & 63) == 0) wsum[buf][tid >> 6] = s;
    }
    __syncthreads();
    const double delta = (wsum[buf][0] + wsum[buf][1]) + (wsum[buf][2] + wsum[buf][3]);
    // every thread decides by the same rule on the same values; a rejected proposal leaves LDS alone and needs no further barrier
    // (wsum alternates, so the next proposal's sums do not overwrite these before every thread has read them)
    if (delta <= (theta * u) * phi) {
      if (tid == 0) {
        lv_set<WIDE>(lo, hi, d * n + a, pbd);
        lv_set<WIDE>(lo, hi, d * n + b, pad);
      }
      phi = phi + delta;
      ++acc;
      __syncthreads();
      if (phi < best_phi) {
        best_phi = phi;
        for (int j = tid; j < n; j += LHS_HW)
          for (int dd = 0; dd < D; ++dd) B[j * D + dd] = lv_get<WIDE>(lo, hi, dd * n + j);
      }
    }
    if (--left == 0) {
      theta = theta * rho;
      left = stage;
    }
  }
  if (tid == 0) accepted[c] = acc;
}

// rows in the order of their level in column 0: Pc[l] = the row whose first entry is l
__global__ __launch_bounds__(256) void lhs_canon_kernel(const int* __restrict__ P, int n, int D, int* __restrict__ Pc) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int* row = P + ((size_t)blockIdx.y * n + i) * D;
  int* dst = Pc + ((size_t)blockIdx.y * n + row[0]) * D;
  for (int d = 0; d < D; ++d) dst[d] = row[d];
}

constexpr int LHS_ROW_THREADS = 128;

// r[l] = sum over m > l, ascending, of g(R_lm) over the sorted rows; rmin[l] / rcnt[l] = the smallest R_lm, m > l, and how many m have it
__global__ __launch_bounds__(LHS_ROW_THREADS) void lhs_rowsum_kernel(const int* __restrict__ Pc, int n, int D, int q, double* __restrict__ r,
                                                                     long long* __restrict__ rmin, long long* __restrict__ rcnt) {
#pragma clang fp contract(off)
  extern __shared__ int own[];      // (D, 128): every thread's own row
  const int tid = threadIdx.x, l0 = blockIdx.x * LHS_ROW_THREADS, l = l0 + tid;
  const int* P = Pc + (size_t)blockIdx.y * n * D;
  const int lc = min(l, n - 1);
  for (int d = 0; d < D; ++d) own[d * LHS_ROW_THREADS + tid] = P[(size_t)lc * D + d];
  double s = 0.0;
  long long mn = LLONG_MAX, cnt = 0;
  for (int m = l0 + 1; m < n; ++m) {
    long long R = 0;
    for (int d = 0; d < D; ++d) {
      const int df = own[d * LHS_ROW_THREADS + tid] - P[(size_t)m * D + d];
      R += (long long)df * df;
    }
    if (m > l) {
      s = s + lhs_g(R, q);
      if (R < mn) {
        mn = R;
        cnt = 1;
      } else if (R == mn) {
        ++cnt;
      }
    }
  }
  if (l < n) {
    const size_t o = (size_t)blockIdx.y * n + l;
    r[o] = s;
    rmin[o] = mn;
    rcnt[o] = cnt;
  }
}

// Phi = thread-strided sums of r and the fixed tree; the exact minimum of R and the number of pairs at it
__global__ __launch_bounds__(LHS_THREADS) void lhs_reduce_kernel(const double* __restrict__ r, const long long* __restrict__ rmin,
                                                                 const long long* __restrict__ rcnt, int n, double* __restrict__ phi,
                                                                 long long* __restrict__ minr, long long* __restrict__ pairs) {
#pragma clang fp contract(off)
  __shared__ double ws[LHS_THREADS / 64];
  __shared__ long long wm[LHS_THREADS / 64];
  __shared__ unsigned long long total;
  const int tid = threadIdx.x;
  const size_t o = (size_t)blockIdx.x * n;
  double s = 0.0;
  long long mn = LLONG_MAX;
  for (int l = tid; l < n; l += LHS_THREADS) {
    s = s + r[o + l];
    mn = min(mn, rmin[o + l]);
  }
  s = wave_tree(s);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mn = min(mn, __shfl_down(mn, off, 64));
  if ((tid & 63) == 0) {
    ws[tid >> 6] = s;
    wm[tid >> 6] = mn;
  }
  if (tid == 0) total = 0;
  __syncthreads();
  mn = min(min(wm[0], wm[1]), min(wm[2], wm[3]));
  unsigned long long cnt = 0;
  for (int l = tid; l < n; l += LHS_THREADS)
    if (rmin[o + l] == mn) cnt += (unsigned long long)rcnt[o + l];
  if (cnt) atomicAdd(&total, cnt);           // integers: the order does not matter
  __syncthreads();
  if (tid == 0) {
    phi[blockIdx.x] = (ws[0] + ws[1]) + (ws[2] + ws[3]);
    minr[blockIdx.x] = mn;
    pairs[blockIdx.x] = (long long)total;
  }
}

// Phi, min R and the pairs at it of nb level matrices on the device
void lhs_criteria(const int* dP, int nb, int n, int D, int q, int* dPc, double* dR, long long* dRmin, long long* dRcnt, double* dPhi,
                  long long* dMin, long long* dPairs, hipStream_t st) {
  hipLaunchKernelGGL(lhs_canon_kernel, dim3((n + 255) / 256, nb), dim3(256), 0, st, dP, n, D, dPc);
  hipLaunchKernelGGL(lhs_rowsum_kernel, dim3((n + LHS_ROW_THREADS - 1) / LHS_ROW_THREADS, nb), dim3(LHS_ROW_THREADS),
                     (size_t)D * LHS_ROW_THREADS * sizeof(int), st, (const int*)dPc, n, D, q, dR, dRmin, dRcnt);
  hipLaunchKernelGGL(lhs_reduce_kernel, dim3(nb), dim3(LHS_THREADS), 0, st, (const double*)dR, (const long long*)dRmin,
                     (const long long*)dRcnt, n, dPhi, dMin, dPairs);
  HIPCK(hipGetLastError());
}

}  // namespace

void design_anneal_lhs(const int* start, int C, int n, int D, long long n_steps, int q, double theta0, double rho, long long stage,
                       unsigned long long seed, unsigned stream, int* best_out, double* phi_out, long long* minr_out, long long* pairs_out,
                       long long* accepted_out) {
  const std::string me = "design_anneal_lhs: ";
  if (!start || !best_out || !phi_out || !minr_out || !pairs_out || !accepted_out) throw std::runtime_error(me + "null pointer");
  if (C < 1) throw std::runtime_error(me + "at least one chain is needed");
  if (n < 2) throw std::runtime_error(me + "a design needs at least two points");
  if (D < 1 || D > LHS_MAX_D) throw std::runtime_error(me + "number of input dimensions must be between 1 and " + std::to_string(LHS_MAX_D));
  if (n_steps < 0) throw std::runtime_error(me + "n_steps must not be negative");
  if (q < 1) throw std::runtime_error(me + "q must be at least 1");
  if (!(theta0 >= 0.0) || !(theta0 <= 1.7976931348623157e308)) throw std::runtime_error(me + "theta0 must be finite and not negative");
  if (!(rho > 0.0) || !(rho <= 1.0)) throw std::runtime_error(me + "rho must be in (0, 1]");
  if (stage < 1) throw std::runtime_error(me + "stage must be at least 1");
  const LhsLayout lay = lhs_layout(n, D);
  if (!lay.fits)
    throw std::runtime_error(me + "the level matrix does not fit the LDS of one workgroup: n * D must be at most " +
                             std::to_string(LHS_NARROW_MAX_ND) + " for n <= " + std::to_string(LHS_NARROW_MAX_N) + " and at most " +
                             std::to_string(LHS_WIDE_MAX_ND) + " above (n = " + std::to_string(n) + ", D = " + std::to_string(D) + ")");
  if (lhs_power_overflows(n, D, q))
    throw std::runtime_error(me + "(D (n - 1)^2)^q reaches 2^" + std::to_string(LHS_POWER_BITS) + ": the criterion would overflow (lower q)");
  const size_t nd = (size_t)n * D;
  {
    std::vector<unsigned char> seen(n);
    for (int c = 0; c < C; ++c)
      for (int d = 0; d < D; ++d) {
        std::fill(seen.begin(), seen.end(), 0);
        for (int i = 0; i < n; ++i) {
          const int v = start[(size_t)c * nd + (size_t)i * D + d];
          if (v < 0 || v >= n || seen[v])
            throw std::runtime_error(me + "column " + std::to_string(d) + " of start " + std::to_string(c) +
                                     " is not a permutation of 0 .. n-1");
          seen[v] = 1;
        }
      }
  }
  const bool small = (unsigned long long)D * (unsigned long long)(n - 1) * (unsigned long long)(n - 1) < (1ull << 32);
  auto kern = lay.wide ? (small ? &lhs_anneal_kernel<true, true> : &lhs_anneal_kernel<true, false>)
                       : (small ? &lhs_anneal_kernel<false, true> : &lhs_anneal_kernel<false, false>);
  HIPCK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lay.bytes));
  // chains per pass: DESIGN_SCRATCH_BYTES of level matrices (one chain where a single one is larger); chains are independent, so the split
  // changes no bit
  const int chunk = (int)std::max<size_t>(1, std::min<size_t>({(size_t)C, DESIGN_SCRATCH_BYTES / (nd * sizeof(int)), (size_t)DESIGN_MAX_PASS}));
  DevBuf<int> dStart((size_t)chunk * nd), dBest((size_t)chunk * nd), dPc((size_t)chunk * nd);
  DevBuf<double> dR((size_t)chunk * n), dPhi0(chunk), dPhi(chunk);
  DevBuf<long long> dRmin((size_t)chunk * n), dRcnt((size_t)chunk * n), dMin(chunk), dPairs(chunk), dAcc(chunk);
  hipStream_t st = nullptr;
  SyncOnUnwind guard{st};
  for (int c0 = 0; c0 < C; c0 += chunk) {
    const int nb = std::min(chunk, C - c0);
    HIPCK(hipMemcpyAsync(dStart, start + (size_t)c0 * nd, (size_t)nb * nd * sizeof(int), hipMemcpyHostToDevice, st));
    lhs_criteria(dStart, nb, n, D, q, dPc, dR, dRmin, dRcnt, dPhi0, dMin, dPairs, st);
    prof_begin("design_anneal_lhs", st);
    hipLaunchKernelGGL(kern, dim3(nb), dim3(LHS_HW), (size_t)lay.bytes, st, (const int*)dStart.get(), n, D, n_steps, q, theta0, rho, stage,
                       (uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32), (uint32_t)(stream + (unsigned)c0), (const double*)dPhi0.get(),
                       (int)lay.hi_offset, dBest.get(), dAcc.get());
    HIPCK(hipGetLastError());
    // algorithmic: per proposal and row j, 2 D differences, squares and additions, and four g of q operations each; LDS only
    prof_end("design_anneal_lhs", st, (double)nb * (double)n_steps * (double)n * (6.0 * D + 4.0 * q + 4.0), 0.0);
    lhs_criteria(dBest, nb, n, D, q, dPc, dR, dRmin, dRcnt, dPhi, dMin, dPairs, st);
    HIPCK(hipMemcpyAsync(best_out + (size_t)c0 * nd, dBest, (size_t)nb * nd * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCK(hipMemcpyAsync(phi_out + c0, dPhi, (size_t)nb * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCK(hipMemcpyAsync(minr_out + c0, dMin, (size_t)nb * sizeof(long long), hipMemcpyDeviceToHost, st));
    HIPCK(hipMemcpyAsync(pairs_out + c0, dPairs, (size_t)nb * sizeof(long long), hipMemcpyDeviceToHost, st));
    HIPCK(hipMemcpyAsync(accepted_out + c0, dAcc, (size_t)nb * sizeof(long long), hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
  }
}

}  // namespace mogp
