// Host-side O(D) scalar pieces of the path: priors, mean functions, parameter transforms.
// Counterparts of mogp_gpu/src/gppriors.hpp, meanfunc.hpp, gpparams.hpp (arithmetic follows the
// CPU oracle: Priors.py:291-354, 842-1128; GPParams.py:35-147).
#pragma once
#include <algorithm>
#include <cmath>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

namespace mogp {

enum { PRIOR_INVGAMMA = 0, PRIOR_GAMMA = 1, PRIOR_LOGNORMAL = 2, PRIOR_WEAK = 3 };
enum { NUG_ADAPTIVE = 0, NUG_FIT = 1, NUG_FIXED = 2, NUG_PIVOT = 3 };

struct Prior {
  int type = PRIOR_WEAK;
  double shape = 0., scale = 0.;

  double logp(double x) const {
    switch (type) {
      case PRIOR_INVGAMMA: return shape * std::log(scale) - std::lgamma(shape) - (shape + 1.) * std::log(x) - scale / x;
      case PRIOR_GAMMA: return -shape * std::log(scale) - std::lgamma(shape) + (shape - 1.) * std::log(x) - x / scale;
      case PRIOR_LOGNORMAL: {
        const double u = std::log(x / scale) / shape;
        return -0.5 * u * u - 0.5 * std::log(2. * M_PI) - std::log(x) - std::log(shape);
      }
      default: return 0.;
    }
  }
  double dlogpdx(double x) const {
    switch (type) {
      case PRIOR_INVGAMMA: return -(shape + 1.) / x + scale / (x * x);
      case PRIOR_GAMMA: return (shape - 1.) / x - 1. / scale;
      case PRIOR_LOGNORMAL: return -std::log(x / scale) / (shape * shape) / x - 1. / x;
      default: return 0.;
    }
  }
  double d2logpdx2(double x) const {
    switch (type) {
      case PRIOR_INVGAMMA: return (shape + 1.) / (x * x) - 2. * scale / (x * x * x);
      case PRIOR_GAMMA: return -(shape - 1.) / (x * x);
      case PRIOR_LOGNORMAL: return (-1. / (shape * shape) + std::log(x / scale) / (shape * shape) + 1.) / (x * x);
      default: return 0.;
    }
  }
  // draw of the scaled variable (Priors.py sample_x); weak priors sample the RAW variable
  template <class RNG>
  double sample_x(RNG& rng) const {
    switch (type) {
      case PRIOR_INVGAMMA: { std::gamma_distribution<double> g(shape, 1.0); return scale / g(rng); }
      case PRIOR_GAMMA: { std::gamma_distribution<double> g(shape, scale); return g(rng); }
      case PRIOR_LOGNORMAL: { std::normal_distribution<double> nd(std::log(scale), shape); return std::exp(nd(rng)); }
      default: return 0.;
    }
  }
};

// theta_data layout: [corr_raw (D) | log sigma^2 | log nugget (fit only)]
struct Priors {
  std::vector<Prior> corr;
  Prior cov, nug;
  bool created = false;

  double logp(const std::vector<double>& th, int D, int nug_type) const {
    if (!created) return 0.;
    double lp = 0.;
    for (int d = 0; d < D; ++d) lp += corr[d].logp(std::exp(-0.5 * th[d]));
    lp += cov.logp(std::exp(th[D]));
    if (nug_type == NUG_FIT) lp += nug.logp(std::exp(th[D + 1]));
    return lp;
  }
  void dlogpdtheta(const std::vector<double>& th, int D, int nug_type, double* out) const {
    const int nd = D + 1 + (nug_type == NUG_FIT ? 1 : 0);
    for (int i = 0; i < nd; ++i) out[i] = 0.;
    if (!created) return;
    for (int d = 0; d < D; ++d) {
      const double l = std::exp(-0.5 * th[d]);
      out[d] = corr[d].dlogpdx(l) * (-0.5 * l);
    }
    const double s2 = std::exp(th[D]);
    out[D] = cov.dlogpdx(s2) * s2;
    if (nug_type == NUG_FIT) {
      const double eta = std::exp(th[D + 1]);
      out[D + 1] = nug.dlogpdx(eta) * eta;
    }
  }
  // diagonal of the second derivative with respect to the raw parameters (Priors.py:356-391, 648-666): d2p/dx2 (dx/dtheta)^2 + dp/dx d2x/dtheta2
  // with x = exp(-theta/2) for a correlation length (dx = -x/2, d2x = x/4) and x = exp(theta) for sigma^2 and the nugget (dx = d2x = x)
  void d2logpdtheta2(const std::vector<double>& th, int D, int nug_type, double* out) const {
    const int nd = D + 1 + (nug_type == NUG_FIT ? 1 : 0);
    for (int i = 0; i < nd; ++i) out[i] = 0.;
    if (!created) return;
    for (int d = 0; d < D; ++d) {
      const double l = std::exp(-0.5 * th[d]);
      out[d] = corr[d].d2logpdx2(l) * (0.25 * l * l) + corr[d].dlogpdx(l) * (0.25 * l);
    }
    const double s2 = std::exp(th[D]);
    out[D] = cov.d2logpdx2(s2) * (s2 * s2) + cov.dlogpdx(s2) * s2;
    if (nug_type == NUG_FIT) {
      const double eta = std::exp(th[D + 1]);
      out[D + 1] = nug.d2logpdx2(eta) * (eta * eta) + nug.dlogpdx(eta) * eta;
    }
  }
  template <class RNG>
  void sample(RNG& rng, int D, int nug_type, double* out) const {
    std::uniform_real_distribution<double> U(0., 1.);
    auto draw = [&](const Prior& p, bool corr_tr) {
      if (!created || p.type == PRIOR_WEAK) return 5. * (U(rng) - 0.5);     // WeakPrior.sample, Priors.py:636-649
      const double x = p.sample_x(rng);
      return corr_tr ? -2. * std::log(x) : std::log(x);
    };
    for (int d = 0; d < D; ++d) out[d] = draw(created ? corr[d] : Prior(), true);
    out[D] = draw(cov, false);
    if (nug_type == NUG_FIT) out[D + 1] = draw(nug, false);
  }
};

// Mean functions evaluated on the host (meanfunc.hpp).  kind: 0 zero, 1 fixed, 2 const, 3 poly.
struct MeanFunc {
  int kind = 0;
  double value = 0.;
  std::vector<int> dims, powers;

  int n_params() const { return kind == 2 ? 1 : (kind == 3 ? 1 + (int)dims.size() : 0); }
  void check(int np, int D) const {
    if (np != n_params()) throw std::runtime_error("Expected params list of length " + std::to_string(n_params()));
    for (int d : dims)
      if (d >= D) throw std::runtime_error("Dimension index must be less than D");
  }
  void mean_f(const double* xs, int m, int D, const double* p, int np, double* out) const {
    check(np, D);
    for (int i = 0; i < m; ++i) {
      double v = 0.;
      if (kind == 1) v = value;
      else if (kind == 2) v = p[0];
      else if (kind == 3) {
        v = p[0];
        for (size_t t = 0; t < dims.size(); ++t) v += p[t + 1] * std::pow(xs[(size_t)i * D + dims[t]], powers[t]);
      }
      out[i] = v;
    }
  }
  // out (n_params, m)
  void mean_deriv(const double* xs, int m, int D, const double* p, int np, double* out) const {
    check(np, D);
    if (kind == 2) for (int i = 0; i < m; ++i) out[i] = 1.;
    if (kind == 3) {
      for (int i = 0; i < m; ++i) out[i] = 1.;
      for (size_t t = 0; t < dims.size(); ++t)
        for (int i = 0; i < m; ++i) out[(t + 1) * m + i] = std::pow(xs[(size_t)i * D + dims[t]], powers[t]);
    }
  }
  // out (D, m)
  void mean_inputderiv(const double* xs, int m, int D, const double* p, int np, double* out) const {
    check(np, D);
    for (size_t e = 0; e < (size_t)D * m; ++e) out[e] = 0.;
    if (kind == 3)
      for (size_t t = 0; t < dims.size(); ++t)
        for (int i = 0; i < m; ++i)
          out[(size_t)dims[t] * m + i] += p[t + 1] * powers[t] * std::pow(xs[(size_t)i * D + dims[t]], powers[t] - 1);
  }
};

// Analytic mean with priors beta ~ N(b, B) (weak: B^-1 = 0, b = 0), from the Gram matrix G = [t,H]^T K^-1 [t,H] (row stride rmax):
//   A = H^T K^-1 H + B^-1 (calc_Ainv, linalg_utils.py:5-40),  r = H^T K^-1 (t - H b),
//   beta_hat = A^-1 (r + B^-1 b) (calc_mean_params, :88-121),  quadratic form (t-Hb)^T K^-1 (t-Hb) - r^T A^-1 r
struct AnalyticMean {
  bool ok = false;               // A is positive definite; false: only LA (as far as the factorisation got) is written
  double quad = 0., logdetA = 0.;   // the quadratic form; log|A| (+ log|B| with informative priors)
  int n_coeff = 0;               // n - q with weak priors, n otherwise (GaussianProcess.py:674-677)
  std::vector<double> beta, LA;  // beta_hat (q); q x q lower Cholesky factor of A
  // combination matrix over Z = K^-1 [t, h_1..h_q], (q + 2) rows of rmax:
  //   row 0 -> K^-1 (t - H beta_hat) (predictions);  row c -> g_c = sum_d (LA^-1)[c][d] K^-1 h_d  (d log|A|);
  //   row R = q + 1 -> K^-1 (t - H (b + beta')) (gradient of the quadratic form; = row 0 with weak priors)
  std::vector<double> M;
};
// mp_*: the emulator's mean priors (GPState; mp_b empty = weak).  `out` is the caller's so that its vectors keep their storage from one
// emulator to the next.
inline void analytic_mean(const double* G, int rmax, int q, int n, const std::vector<double>& mp_b, const std::vector<double>& mp_Binv,
                          const std::vector<double>& mp_Binvb, double mp_logdetB, AnalyticMean& out) {
  const int R = 1 + q;
  const bool weak = mp_b.empty();
  std::vector<double>& LA = out.LA;
  out.ok = true;
  out.quad = G[0];
  out.logdetA = 0.;
  out.n_coeff = n;
  std::vector<double> Am((size_t)q * q), rv(q), bb(q, 0.);
  if (!weak) bb = mp_b;
  for (int r = 0; r < q; ++r) {
    double s = G[(1 + r) * rmax];
    for (int c = 0; c < q; ++c) {
      s -= G[(1 + r) * rmax + (1 + c)] * bb[c];
      Am[r * q + c] = G[(1 + r) * rmax + (1 + c)] + (weak ? 0. : mp_Binv[r * q + c]);
    }
    rv[r] = s;
  }
  if (!weak) {
    double bSb = 0., bv = 0.;
    for (int r = 0; r < q; ++r) {
      bv += bb[r] * G[(1 + r) * rmax];
      for (int c = 0; c < q; ++c) bSb += bb[r] * G[(1 + r) * rmax + (1 + c)] * bb[c];
    }
    out.quad = G[0] - 2. * bv + bSb;
  }
  LA.assign((size_t)q * q, 0.);
  for (int r = 0; r < q && out.ok; ++r)
    for (int c = 0; c <= r; ++c) {
      double s = Am[r * q + c];
      for (int p = 0; p < c; ++p) s -= LA[r * q + p] * LA[c * q + p];
      if (r == c) {
        if (!(s > 0.)) { out.ok = false; break; }
        LA[r * q + r] = std::sqrt(s);
      } else {
        LA[r * q + c] = s / LA[c * q + c];
      }
    }
  if (!out.ok) return;
  auto solveA = [&](std::vector<double> x) {          // A^-1 x by the two triangular solves with LA
    for (int r = 0; r < q; ++r) {
      double s = x[r];
      for (int p = 0; p < r; ++p) s -= LA[r * q + p] * x[p];
      x[r] = s / LA[r * q + r];
    }
    for (int r = q - 1; r >= 0; --r) {
      double s = x[r];
      for (int p = r + 1; p < q; ++p) s -= LA[p * q + r] * x[p];
      x[r] = s / LA[r * q + r];
    }
    return x;
  };
  std::vector<double> w(q), Linv((size_t)q * q, 0.);
  for (int r = 0; r < q; ++r) {               // w = LA^-1 r
    double s = rv[r];
    for (int p = 0; p < r; ++p) s -= LA[r * q + p] * w[p];
    w[r] = s / LA[r * q + r];
    out.quad -= w[r] * w[r];
    out.logdetA += 2. * std::log(LA[r * q + r]);
  }
  const std::vector<double> bgrad = solveA(rv);           // beta' = A^-1 r: residual of the gradient's quadratic form
  std::vector<double> rhs(rv);
  if (!weak)
    for (int r = 0; r < q; ++r) rhs[r] += mp_Binvb[r];
  out.beta = solveA(rhs);
  for (int c = 0; c < q; ++c) {               // LA^-1 (lower), column by column
    for (int r = c; r < q; ++r) {
      double s = (r == c) ? 1. : 0.;
      for (int p = c; p < r; ++p) s -= LA[r * q + p] * Linv[p * q + c];
      Linv[r * q + c] = s / LA[r * q + r];
    }
  }
  std::vector<double>& M = out.M;
  M.assign((size_t)(R + 1) * rmax, 0.);
  M[0] = 1.;
  M[R * rmax] = 1.;
  for (int c = 0; c < q; ++c) {
    M[1 + c] = -out.beta[c];
    M[R * rmax + 1 + c] = -(bb[c] + bgrad[c]);
  }
  for (int c = 0; c < q; ++c)
    for (int d = 0; d <= c; ++d) M[(1 + c) * rmax + (1 + d)] = Linv[c * q + d];
  if (weak) out.n_coeff = n - q;
  else out.logdetA += mp_logdetB;             // + log|B| (priors.mean.logdet_cov)
}

// The analytic mean's terms of predict(full_cov=True) at m points (GaussianProcess.py:899-911; calc_R, linalg_utils.py:123-168), with
// R = H*^T - H^T K^-1 k*:  mu += h(x*)^T beta,  rm = LA^-1 R,  C += rm^T rm.  Hs (q x m): basis columns at the test points; dots ((1 + q) x m):
// row 1 + c = k*^T K^-1 h_c; beta (q), LA (q x q) of the fit.  mu (m) and C (m x m) are updated in place; rm (q x m) is the caller's scratch.
inline void fullcov_mean_terms(int q, int m, const double* beta, const double* LA, const double* Hs, const double* dots, double* mu,
                               double* rm, double* C) {
  for (int j = 0; j < m; ++j) {
    for (int c = 0; c < q; ++c) {
      mu[j] += beta[c] * Hs[(size_t)c * m + j];
      double s = Hs[(size_t)c * m + j] - dots[(size_t)(1 + c) * m + j];
      for (int p = 0; p < c; ++p) s -= LA[c * q + p] * rm[(size_t)p * m + j];
      rm[(size_t)c * m + j] = s / LA[c * q + c];
    }
  }
  for (int i = 0; i < m; ++i)
    for (int c = 0; c < q; ++c) {
      const double ri = rm[(size_t)c * m + i];
      const double* rc = rm + (size_t)c * m;
      double* row = C + (size_t)i * m;
      for (int j = 0; j < m; ++j) row[j] += ri * rc[j];
    }
}

// The host algebra of Engine::hessian (engine_hessian.hip) for one emulator: the P x P block of the Hessian of the negative log-posterior,
// P = NC + 1 (+ 1 with a fitted nugget), theta order [corr (NC) | cov | nugget], from the device sums of kernels_hess.hip:
//   o (D + 3)              the gradient's sums as launch_grad leaves them: 0.5 sum W o Q_p (p < D), 0.5 sum W o sigma^2 C, tr Q^-1, ., alpha^T alpha
//   T ((D + 1) x (D + 2))  T[p][q] = sum_ab P_p[a,b] P_q[b,a] over the planes M_0 .. M_{D-1}, Q^-1, I (upper entries; T[D][D] = tr Q^-2)
//   A (D x D)              sum W o sigma^2 k'' s_p s_q (upper entries)
//   V, U (D rows of stride NPh)   v_p = M_p^T t = Q_p alpha,  u_p = M_p alpha;     z = Q^-1 alpha,  alpha = Q^-1 t,  t the residual targets (n each)
//   dpr (P)                the prior's second derivatives (Priors::d2logpdtheta2)
// First the matrix Fd over the per-dimension parameters [corr_0 .. corr_{D-1} | cov | nugget] (scratch of (D + 2)^2 doubles), then -- one
// shared length scale (uniform) -- theta_0 moves every length at once: its row is the sum of the D correlation rows, its diagonal entry the
// sum of the D x D block.  Hm (P x P, row-major) receives the UPPER triangle, the rest of it zeros.  Returns false when an entry is not
// finite.  Every dot product runs in ascending index with one accumulator: the same inputs give the same bits.
inline bool hessian_assemble(int n, int D, int NC, bool uniform, bool nug_fit, double eta, const double* o, const double* T, const double* A,
                             const double* V, const double* U, int NPh, const double* z, const double* alpha, const double* t, const double* dpr,
                             double* Fd, double* Hm) {
  const int TQ = D + 2, P = NC + 1 + (nug_fit ? 1 : 0);
  const double eta2 = eta * eta;
  auto dot = [&](const double* a, const double* b) {
    double acc = 0.;
    for (int e = 0; e < n; ++e) acc += a[e] * b[e];
    return acc;
  };
  const double ta = dot(t, alpha), aa = dot(alpha, alpha), az = dot(alpha, z);
  const double trK = o[D + 1], trK2 = T[D * TQ + D];
  // per-dimension matrix over [corr_0 .. corr_{D-1} | cov | nugget], upper triangle
  std::fill(Fd, Fd + (size_t)TQ * TQ, 0.);
  for (int p = 0; p < D; ++p) {
    const double* vp = V + (size_t)p * NPh;
    for (int q = p; q < D; ++q)
      Fd[p * TQ + q] = dot(vp, U + (size_t)q * NPh) - 0.5 * T[p * TQ + q] + 0.5 * A[p * D + q] + (p == q ? o[p] : 0.);
    const double va = dot(vp, alpha), vz = dot(vp, z);
    Fd[p * TQ + D] = (va - eta * vz) - 0.5 * (T[p * TQ + D + 1] - eta * T[p * TQ + D]) + o[p];
    Fd[p * TQ + D + 1] = eta * vz - 0.5 * eta * T[p * TQ + D];
  }
  Fd[D * TQ + D] = (ta - 2. * eta * aa + eta2 * az) - 0.5 * ((double)n - 2. * eta * trK + eta2 * trK2) + o[D];
  Fd[D * TQ + D + 1] = (eta * aa - eta2 * az) - 0.5 * (eta * trK - eta2 * trK2);
  Fd[(D + 1) * TQ + D + 1] = eta2 * az - 0.5 * eta2 * trK2 + 0.5 * eta * (trK - o[D + 2]);
  // theta order [corr (NC) | cov | nugget (fit only)]; one shared length scale: the sums of the per-dimension block and rows
  std::fill(Hm, Hm + (size_t)P * P, 0.);
  auto fd = [&](int p, int q) { return p <= q ? Fd[p * TQ + q] : Fd[q * TQ + p]; };
  auto src = [&](int r) { return r < NC ? r : D + (r - NC); };      // per-dimension index of a non-correlation parameter
  for (int r = 0; r < P; ++r)
    for (int c = r; c < P; ++c) {
      double val;
      if (!uniform || r >= NC) val = fd(src(r), src(c));
      else if (c >= NC) {
        val = 0.;
        for (int p = 0; p < D; ++p) val += fd(p, src(c));
      } else {
        val = 0.;
        for (int p = 0; p < D; ++p)
          for (int q = 0; q < D; ++q) val += fd(p, q);
      }
      Hm[(size_t)r * P + c] = val;
    }
  bool finite = true;
  for (int r = 0; r < P; ++r) {
    Hm[(size_t)r * P + r] -= dpr[r];
    for (int c = r; c < P; ++c) finite = finite && std::isfinite(Hm[(size_t)r * P + c]);
  }
  return finite;
}

}  // namespace mogp
