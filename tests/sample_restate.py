"""NumPy restatement of what sample_posterior computes, written from the specification and independent of the package's own code: the
counter-based normal generator (Philox4x32-10 + Box-Muller on 53-bit uniforms) and mu + chol(Sigma~) z with the jitter ladder."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
U32 = 0xFFFFFFFF

# Random123's known answers for philox4x32-10: (counter, key, output)
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((U32, U32, U32, U32), (U32, U32), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]

LADDER_RUNGS = 5


def philox_scalar(ctr, key):
    """one block in plain Python integers"""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & U32, (p0 >> 32) ^ c3 ^ k1, p0 & U32
        k0, k1 = (k0 + W0) & U32, (k1 + W1) & U32
    return c0, c1, c2, c3


def philox_block(c0, c1, c2, c3, k0, k1):
    """vectorised over uint64 arrays that hold 32-bit values"""
    m = np.uint64(U32)
    s32 = np.uint64(32)
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & m, (p0 >> s32) ^ c3 ^ k1, p0 & m
        k0, k1 = (k0 + np.uint64(W0)) & m, (k1 + np.uint64(W1)) & m
    return c0, c1, c2, c3


def normals(seed, stream, S, m):
    """z (S, m): row s, column j from counter (j >> 1, s, stream, 0), key (seed & 0xffffffff, seed >> 32)"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    pairs = (m + 1) // 2
    p = np.broadcast_to(np.arange(pairs, dtype=np.uint64)[None, :], (S, pairs))
    s = np.broadcast_to(np.arange(S, dtype=np.uint64)[:, None], (S, pairs))
    e = np.full((S, pairs), int(stream) & U32, dtype=np.uint64)
    x0, x1, x2, x3 = philox_block(p, s, e, np.zeros((S, pairs), dtype=np.uint64), seed & U32, seed >> 32)
    u1 = ((x0 >> np.uint64(5)).astype(np.float64) * 67108864. + (x1 >> np.uint64(6)).astype(np.float64) + 1.) * 2. ** -53
    u2 = ((x2 >> np.uint64(5)).astype(np.float64) * 67108864. + (x3 >> np.uint64(6)).astype(np.float64)) * 2. ** -53
    r = np.sqrt(-2. * np.log(u1))
    a = 2. * np.pi * u2
    z = np.empty((S, 2 * pairs))
    z[:, 0::2] = r * np.cos(a)
    z[:, 1::2] = r * np.sin(a)
    return np.ascontiguousarray(z[:, :m])


def ladder_delta(t, mean_diag):
    d = mean_diag * 1e-6
    for _ in range(t):
        d *= 10.
    return d


def sample(mu, cov, z, nugget=0., jitter=0.):
    """(samples (S, m), jitter_used, ok, Sigma~) for one emulator: mu (m), cov (m, m) = Sigma* without nugget, z (S, m)"""
    m = mu.shape[0]
    dbar = float(np.mean(np.diag(cov)))
    tries = [0.] + [ladder_delta(t, dbar) for t in range(LADDER_RUNGS)]
    for delta in tries:
        St = cov + (nugget + (jitter + delta)) * np.eye(m)
        try:
            L = np.linalg.cholesky(St)
        except np.linalg.LinAlgError:
            continue
        return mu[None, :] + z @ L.T, jitter + delta, True, St
    return np.full((z.shape[0], m), np.nan), jitter + tries[-1], False, None
