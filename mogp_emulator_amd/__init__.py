"""
mogp_emulator_amd -- MI355X (gfx950) native fit + predict backend for mogp_emulator's GPU seam.

  csrc/            hand-written HIP kernels + C ABI (libmogp_hip.so, header: include/mogp_hip.h)
  _capi.py         ctypes prototypes of the C ABI
  libgpgpu.py      drop-in for the reference's pybind11 module `libgpgpu`
  LibGPGPU.py, GaussianProcessGPU.py, MultiOutputGP_GPU.py, fitting.py, Priors.py, Kernel.py
                   host-side mirrors of the reference's GPU-facing Python interface
  HistoryMatching.py, SequentialDesign.py, validation.py
                   consumers of the batched prediction (implausibility, MICE / ALC scoring and the sequential-design drivers, validation errors)
                   and leave-one-out / k-fold cross-validation at the fitted hyperparameters on the device (validation.cross_validate)
  SensitivityAnalysis.py
                   first-order and total-effect Sobol indices of the predictive mean, fused behind the batched prediction
  ExperimentalDesign.py
                   one-shot designs (Monte Carlo, Latin hypercube on the host; maximin LHC scored on the device)
  DimensionReduction.py
                   gKDR dimension reduction; R of a whole (X_scale, Y_scale) grid in one device call
  Laplace.py       Hessian of the log-posterior on the device and the Laplace approximation N(theta_hat, H^-1) around a MAP fit
  Marginal.py      predictions averaged over hyperparameter samples (Laplace draws, importance weighted, or the caller's own), reduced on the device
  Sampling.py      joint posterior sample paths f(X*) ~ N(mu*, Sigma*): covariance, Cholesky factor, normals and mu + L z on the device
  ActiveLearning.py
                   posterior covariance between two point sets and the ALC (integrated-variance) design criterion, reduced on the device
  LocalGP.py       local approximate GP prediction for designs beyond the dense path: k nearest neighbours and one small GP per query, on the device
  Vecchia.py       hyperparameters from the whole of a large design: the Vecchia likelihood and its analytic gradient on the device, L-BFGS fit
  IterativeGP.py   exact prediction for designs beyond the dense path: matrix-free preconditioned conjugate gradients on the whole design, on the device;
                   the exact log-likelihood and its gradient by stochastic Lanczos quadrature from one such solve; variance_bound: a
                   conservative predictive variance from a cached low-rank factor, one product per batch of queries and no solve;
                   sample_paths: posterior draws as functions (pathwise conditioning on a random-Fourier-feature prior);
                   predict(deriv=True), matvec_inputderiv and PosteriorPaths.gradient: input derivatives of the mean and of the paths
  dist.py          one-process-per-GPU sharding of emulators + single gather (torch.distributed/RCCL)
"""
from .LibGPGPU import HAVE_LIBGPGPU, gpu_usable            # noqa: F401
from .DimensionReduction import gKDR                        # noqa: F401
from .ExperimentalDesign import ExperimentalDesign, MonteCarloDesign, LatinHypercubeDesign, MaxiMinLHC, OptimisedLHC   # noqa: F401
from .Laplace import LaplaceResult, logpost_hessian, laplace_approximation   # noqa: F401
from .Marginal import predict_marginal, MarginalPredictResult, mixture_weights   # noqa: F401
from .Sampling import sample_posterior, PosteriorSamples, philox_normals   # noqa: F401
from .ActiveLearning import predict_cov, alc_criterion, ALCResult, alc_batch, ALCBatchResult   # noqa: F401
from .LocalGP import LocalGP, LocalPrediction, predict_local   # noqa: F401
from .Vecchia import VecchiaGP, VecchiaLogLik, VecchiaFit, ExactFit   # noqa: F401
from .IterativeGP import IterativeGP, IterativeSolve, IterativePrediction, ExactLogLik, PosteriorPaths, path_features   # noqa: F401

if HAVE_LIBGPGPU:
    from .GaussianProcessGPU import GaussianProcessGPU, PredictResult   # noqa: F401
    from .MultiOutputGP_GPU import MultiOutputGP_GPU                      # noqa: F401
    from .fitting import fit_GP_MAP                                         # noqa: F401
    from .Kernel import SquaredExponential, Matern52, ProductMat52, UniformSqExp, UniformMat52   # noqa: F401
    from .Priors import GPPriors, MeanPriors, InvGammaPrior, GammaPrior, LogNormalPrior, WeakPrior   # noqa: F401
    from .HistoryMatching import HistoryMatching                           # noqa: F401
    from .SequentialDesign import MICEFastGP, mice_criterion, SequentialDesign, MICEDesign, ALCDesign   # noqa: F401
    from .SensitivityAnalysis import sobol_indices, SobolResult          # noqa: F401
    from . import validation                                                # noqa: F401
    from .validation import cross_validate, CrossValidationResult, kfold_labels   # noqa: F401

__version__ = "0.1.0"
