// IterSolver: the state of the iterative exact solver of a LocalGP handle (engine.h) -- preconditioned conjugate gradients on
// A = sigma2 k(X, X) + nugget I of the whole design (engine_iter.hip), the exact likelihood (engine_iter_lik.hip) and the variance bound.
// The handle owns the design and hands the solver const pointers to it; the solver never rescales it.
//
// The device buffers come in four groups.  A group counts its own bytes (BufGroup: a buffer cannot be declared without being counted),
// and a group that holds something built for a key -- the preconditioner, the variance cache -- changes through named transitions alone,
// as GPState (gp_state.h) does for the dense engine:
//   reserve    the one function that may free the group's buffers; when it does, what they held is gone and it drops the key itself
//   drop       nothing usable is held (the start of a build: an exception in between leaves "nothing held")
//   built      the buffers hold what was built for this key; the key is set last
// The variance cache stands for itself: a preconditioner rebuilt for other hyperparameters leaves it alone, growing its own buffers drops it.
#pragma once
#include <vector>

#include "devmem.h"

namespace mogp {

// what a preconditioner, a variance cache or a kept alpha belongs to (rtol and max_iter: of a kept alpha alone, else 0)
struct IterKey {
  int kt = -1, rank = -1, max_iter = 0;
  double sigma2 = 0., nugget = 0., rtol = 0.;
  std::vector<double> scale;
  bool operator==(const IterKey& o) const {
    return kt == o.kt && rank == o.rank && max_iter == o.max_iter && sigma2 == o.sigma2 && nugget == o.nugget && rtol == o.rtol && scale == o.scale;
  }
};
inline IterKey make_key(int kt, const double* scale, int D, double sigma2, double nugget, int rank) {
  IterKey k;
  k.kt = kt, k.rank = rank, k.sigma2 = sigma2, k.nugget = nugget;
  k.scale.assign(scale, scale + D);
  return k;
}

// A set of device buffers that knows its bytes: a member buffer is declared as Buf<T> name{this}, which is the only way to declare one.
class BufGroup {
 public:
  BufGroup() = default;
  BufGroup(const BufGroup&) = delete;
  BufGroup& operator=(const BufGroup&) = delete;
  double bytes() const {             // the device bytes of the group as its buffers are now
    double b = 0.;
    for (const DevBuf<double>* d : dbl) b += 8.0 * (double)d->size();
    for (const DevBuf<int>* i : ints) b += 4.0 * (double)i->size();
    return b;
  }

 protected:
  template <class T>
  struct Buf : DevBuf<T> {
    explicit Buf(BufGroup* g) { g->track(this); }
  };
  // b holds at least `count` elements afterwards; true when that freed what it held
  template <class T>
  static bool grow(DevBuf<T>& b, size_t count) {
    const bool frees = b.size() < count;
    b.reserve(count);
    return frees;
  }

 private:
  void track(const DevBuf<double>* b) { dbl.push_back(b); }
  void track(const DevBuf<int>* b) { ints.push_back(b); }
  std::vector<const DevBuf<double>*> dbl;
  std::vector<const DevBuf<int>*> ints;
};

// the scaled design and the residual rows of the handle, as the solver sees them
struct IterDesign {
  const double* Xs = nullptr;        // (N, D) scaled coordinates: LocalGP::ensure_scaled forms them before the solver is called
  const double* Y = nullptr;         // (E, N)
  long N = 0;
  int D = 0, E = 0;
};

class IterSolver {
 public:
  // P = L L^T + nugget I: the partial pivoted Cholesky factor, Ginv = (nugget I + L^T L)^-1 and the scratch of building and applying them
  struct Precond : BufGroup {
    Buf<double> L{this}, G{this}, diag{this}, dmax{this}, pval{this}, wpart{this}, w{this}, w2{this};
    Buf<int> piv{this}, state{this}, pidx{this};
    void reserve(long N, int rank);
    void drop() { key_ = IterKey(); }
    void built(const IterKey& k, int reached, double logdet) { rank_ = reached, logdetG_ = logdet, key_ = k; }
    bool holds(const IterKey& k) const { return k == key_; }
    bool any() const { return key_.kt >= 0; }
    const IterKey& key() const { return key_; }
    int rank() const { return rank_; }                   // the rank reached
    double logdetG() const { return logdetG_; }          // log|nugget I + L^T L| (0 at rank 0)

   private:
    IterKey key_;
    int rank_ = 0;
    double logdetG_ = 0.;
  };
  // the panels of the iteration (N x 32 each), the partial sums of the dots, the step scalars and the frozen flags
  struct CgPanels : BufGroup {
    Buf<double> b{this}, x{this}, xl{this}, r{this}, p{this}, q{this}, z{this}, v{this}, part{this}, sc{this};
    Buf<int> fl{this};
    void reserve(long N);
  };
  // R (N, the rank in whole panels of 32 columns) with R^T A R = I, and the triangular factor that is being applied while it is built
  struct VarCache : BufGroup {
    Buf<double> R{this}, T{this};
    void reserve(long N, int rank);
    void drop() { key_ = IterKey(), rank_ = 0; }
    void built(const IterKey& k, int r, int precond_reached) { rank_ = r, reached_ = precond_reached, key_ = k; }
    bool holds(const IterKey& k) const { return k == key_; }
    int rank() const { return rank_; }                   // the columns of R
    int reached() const { return reached_; }             // the rank the preconditioner it was built from had reached

   private:
    IterKey key_;
    int rank_ = 0, reached_ = 0;
  };
  // the exact likelihood's own buffers: the first preconditioned residuals, the coefficient log, the normals g1 and the sweep's sums
  struct LikScratch : BufGroup {
    Buf<double> W{this}, log{this}, g1{this}, part{this}, out{this};
    void reserve(long N, int D, int rank, int max_iter);
  };
  struct KeptAlpha {                 // alpha = A^-1 (residual row) of one emulator, kept while its key stays
    IterKey key;
    std::vector<double> alpha;
    int iterations = 0, converged = 0;
    double residual = 0.;
  };

  IterDesign design;
  Precond pre;
  CgPanels cg;
  VarCache var;
  LikScratch lik;

  double held() const { return pre.bytes() + cg.bytes(); }      // what predict_plan.h's iter_held_bytes counts, as it is now
  // the preconditioner's buffers and the panels for this rank, refused by name (predict_plan.h) when they do not fit
  void reserve(const char* who, int rank);
  void build(const IterKey& k, hipStream_t st);                 // the preconditioner of k, unless it is the one held
  // the variance cache of k from the preconditioner held (build(k) first), unless it is the one held
  void var_build(const IterKey& k, hipStream_t st);
  // CG on the panel cg.b (N x 32; columns >= cols are zero) into cg.x at the key of the preconditioner held; it / cv / rs: 32 entries each.
  // first_z (a panel) receives the first z = P^-1 r of every column, coef_log (2 * 32 * max_iter) the step coefficients; both may be null
  // and change no bit of anything else.
  void solve(int cols, double rtol, int max_iter, int* it, int* cv, double* rs, hipStream_t st, double* first_z = nullptr, double* coef_log = nullptr);
  // out (32, host) = the column-wise dots of two panels, the blocks added in ascending order; the copy is queued on st, not waited for
  void dots(const double* a, const double* b, double* out, hipStream_t st);
  // The kept alpha of emulator e: its key says whether it is the one asked for.  keep_alpha stores column 0 of cg.x with the statistics
  // of its solve and waits for st; the key is set last.
  KeptAlpha& alpha_of(int e);
  void keep_alpha(int e, const IterKey& k, int iterations, int converged, double residual, hipStream_t st);

 private:
  std::vector<KeptAlpha> alpha;      // per emulator
};

}  // namespace mogp
