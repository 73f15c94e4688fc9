"""NumPy restatement of the input derivatives at large designs (mogp_emulator_amd.IterativeGP.matvec_inputderiv, predict(deriv=True),
PosteriorPaths.gradient), written from the definitions, in float64 and in np.longdouble.  Scaled coordinates are x~ = x * s (one rounded
multiply, iterative_restate.scaled; the truth takes the float64 scaled points as exact), r2_ij = sum_d (q~_id - x~_jd)^2, and every
derivative is with respect to the RAW coordinate x_d of a query:

    G[i, d, c] = d/dx_d [sigma^2 k(q_i, X) V]_c = 2 s_d sum_j sigma^2 k'(r2_ij) (q~_id - x~_jd) V_jc          k' = dk / dr2; no nugget term
    dg_s/dx_d  = -amp s_d sum_f W_sf omega_fd sin(b_f + omega_f . x~),   amp = sqrt(2 sigma^2 / F)
    df_s/dx_d  = dm/dx_d + dg_s/dx_d + G[., d, s] at V = update;     d mean/dx_d = dm/dx_d + G at V = alpha

k' = -exp(-r2 / 2) / 2 for the squared-exponential kernels and -(5 / 6) (1 + t) exp(-t), t = sqrt(5 r2), for the Matern-5/2 kernels: finite at
r2 = 0.  The entry of the sum is k' times the DIFFERENCE of the scaled coordinates; kgrad_expanded is the form q~_d sum g V - sum g x~_jd V
that cancels on designs away from the origin, kept here to show that the bar tells the two apart."""
import numpy as np

import iterative_restate as ir
import pathwise_restate as pw


def kernel_dr2(r2, kind):
    """dk / dr2"""
    dtype = r2.dtype.type
    if kind in ir.MATERN:
        t = np.sqrt(dtype(5) * r2)
        return -(dtype(5) / dtype(6)) * (dtype(1) + t) * np.exp(-t)
    return -np.exp(-r2 / dtype(2)) / dtype(2)


def _r2(Q, X):
    r2 = np.zeros((Q.shape[0], X.shape[0]), dtype=Q.dtype)
    for d in range(Q.shape[1]):
        t = Q[:, d][:, None] - X[:, d][None, :]
        r2 = r2 + t * t
    return r2


def generated(Qt, Xt, kind, sigma2, dtype=np.float64):
    """g (M, N) = sigma^2 k'(r2) between the SCALED points Qt and Xt (float64 values, whatever the dtype of what follows)"""
    Q, X = np.asarray(Qt, dtype=np.float64).astype(dtype), np.asarray(Xt, dtype=np.float64).astype(dtype)
    return dtype(sigma2) * kernel_dr2(_r2(Q, X), kind)


def kgrad_in(Qt, Xt, s, kind, sigma2, V, dtype=np.float64):
    """G (M, D, c) in the difference form: per dimension the matrix g_ij (q~_id - x~_jd) times V, then 2 s_d once"""
    Q, X = np.asarray(Qt, dtype=np.float64).astype(dtype), np.asarray(Xt, dtype=np.float64).astype(dtype)
    V = np.asarray(V, dtype=np.float64).astype(dtype)
    g = generated(Qt, Xt, kind, sigma2, dtype)
    out = np.zeros((Q.shape[0], Q.shape[1], V.shape[1]), dtype=dtype)
    for d in range(Q.shape[1]):
        a = g * (Q[:, d][:, None] - X[:, d][None, :])
        out[:, d, :] = (dtype(2) * dtype(s[d])) * (a @ V)
    return out


def kgrad_expanded(Qt, Xt, s, kind, sigma2, V, dtype=np.float64):
    """the same in the expanded form q~_d (g V) - g (x~_d * V): equal in exact arithmetic"""
    Q, X = np.asarray(Qt, dtype=np.float64).astype(dtype), np.asarray(Xt, dtype=np.float64).astype(dtype)
    V = np.asarray(V, dtype=np.float64).astype(dtype)
    g = generated(Qt, Xt, kind, sigma2, dtype)
    gv = g @ V
    out = np.zeros((Q.shape[0], Q.shape[1], V.shape[1]), dtype=dtype)
    for d in range(Q.shape[1]):
        out[:, d, :] = (dtype(2) * dtype(s[d])) * (Q[:, d][:, None] * gv - g @ (X[:, d][:, None] * V))
    return out


def kgrad_bar(Qt, Xt, s, kind, sigma2, V):
    """per entry (i, d, c): 2^-52 2 s_d [(N + 6) sum_j |g_ij| |D_ijd| |V_jc| + (4 D + 32) sigma^2 sum_j |D_ijd| |V_jc|], D_ijd = q~_id - x~_jd
    -- a fixed-order sum of N products of three rounded factors (the generated g, the rounded difference, V; then 2 s_d and the store), and
    test_iterative_host.matvec_bar's absolute error of one generated entry ((D + 2) roundings of the difference-form r2 reach k' through
    |k''| r2 <= 0.23; the rest is the table exponential's), carried by |D_ijd|"""
    Qt, Xt, V = np.asarray(Qt, dtype=np.float64), np.asarray(Xt, dtype=np.float64), np.abs(np.asarray(V, dtype=np.float64))
    N, D = Xt.shape
    g = np.abs(generated(Qt, Xt, kind, sigma2))
    out = np.zeros((Qt.shape[0], D, V.shape[1]))
    for d in range(D):
        delta = np.abs(Qt[:, d][:, None] - Xt[:, d][None, :])
        out[:, d, :] = 2. ** -52 * 2. * s[d] * ((N + 6) * ((g * delta) @ V) + (4 * D + 32) * sigma2 * (delta @ V))
    return out


def rff_grad(Pt, s, omega, phase, W, sigma2, dtype=np.float64):
    """(M, D, S) d/dx_d [amp Phi W^T]: the sine of pathwise_restate.arguments (the argument the feature product builds) times the rounded
    products omega_fd W_sf, summed over f, then -(amp s_d) once"""
    Sn = np.sin(pw.arguments(Pt, omega, phase, dtype))
    Om, W = np.asarray(omega, dtype=np.float64).astype(dtype), np.asarray(W, dtype=np.float64).astype(dtype)
    F, D = Om.shape
    amp = np.sqrt(dtype(2) * dtype(sigma2) / dtype(F))
    out = np.zeros((Sn.shape[0], D, W.shape[0]), dtype=dtype)
    for d in range(D):
        out[:, d, :] = -(amp * dtype(s[d])) * (Sn @ (Om[:, d][None, :] * W).T)
    return out


def rffgrad_bar(Pt, s, omega, phase, W, sigma2):
    """per entry (i, d, s): pathwise_restate.rff_bar's expression with |cos| -> |sin| and |W_sf| -> |omega_fd| |W_sf|, times s_d:
    2^-52 amp s_d [(F + 4) sum_f |sin t_if| |omega_fd W_sf| + sum_f ((D + 2) T_if + 4) |omega_fd W_sf|] -- the rounding of the argument
    reaches the sine with slope <= 1 as it reaches the cosine"""
    Pt, omega, W = np.asarray(Pt, dtype=np.float64), np.asarray(omega, dtype=np.float64), np.abs(np.asarray(W, dtype=np.float64))
    F, D = omega.shape
    T = np.abs(phase)[None, :] + np.abs(Pt) @ np.abs(omega).T
    Sn = np.abs(np.sin(pw.arguments(Pt, omega, phase)))
    out = np.zeros((Pt.shape[0], D, W.shape[0]))
    for d in range(D):
        B = (np.abs(omega[:, d])[None, :] * W).T              # (F, S)
        out[:, d, :] = 2. ** -52 * np.sqrt(2. * sigma2 / F) * s[d] * ((F + 4) * (Sn @ B) + ((D + 2) * T + 4.) @ B)
    return out


def mean_gradient(X, Q, s, kind, sigma2, alpha, dmean=None, dtype=np.float64):
    """(m, D) d mean / dx at the raw queries Q: dm/dx (m, D) or None for the zero mean, plus G at V = alpha (N,)"""
    G = kgrad_in(ir.scaled(Q, s), ir.scaled(X, s), s, kind, sigma2, np.asarray(alpha, dtype=np.float64)[:, None], dtype)[:, :, 0]
    return G if dmean is None else np.asarray(dmean, dtype=np.float64).astype(dtype) + G


def path_gradient(X, Q, s, kind, sigma2, omega, phase, W, update, dmean=None, dtype=np.float64):
    """(S, m, D) df_s / dx at the raw queries Q from the fields of a PosteriorPaths: W (S, F), update (N, S), dm/dx (m, D) or None"""
    Qt = ir.scaled(Q, s)
    prior = np.transpose(rff_grad(Qt, s, omega, phase, W, sigma2, dtype), (2, 0, 1))
    if dmean is not None:
        prior = prior + np.asarray(dmean, dtype=np.float64).astype(dtype)[None, :, :]
    return prior + np.transpose(kgrad_in(Qt, ir.scaled(X, s), s, kind, sigma2, update, dtype), (2, 0, 1))
