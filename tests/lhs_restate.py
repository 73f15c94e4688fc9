"""NumPy restatement of the Latin-hypercube annealer (DESIGN.md section 3 "Design"; the device: csrc/kernels_lhs.hip), written from the
specification and independent of the package's code: the Philox4x32-10 block, the explicit left-to-right power, the sums in the device's
order, and exact integer criteria.  All chains of a call advance together here (arrays (C, ...)); they never read one another."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
U32 = 0xFFFFFFFF
THREADS = 256                   # threads of the chain's workgroup: 4 waves of 64
LDS_BYTES, LDS_RESERVED = 160 * 1024, 13 * 1024
POWER_BITS = 1000


def philox_block(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 over uint64 arrays that hold 32-bit values"""
    m, s32 = np.uint64(U32), np.uint64(32)
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & m, (p0 >> s32) ^ c3 ^ k1, p0 & m
        k0, k1 = (k0 + np.uint64(W0)) & m, (k1 + np.uint64(W1)) & m
    return c0, c1, c2, c3


def proposal(t, streams, seed, n, D):
    """(d, a, b, u) of proposal t for the Philox streams `streams` (C,)"""
    C = len(streams)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w0, w1, w2, w3 = philox_block(np.full(C, t & U32, dtype=np.uint64), np.full(C, t >> 32, dtype=np.uint64),
                                  np.asarray(streams, dtype=np.uint64) & np.uint64(U32), np.zeros(C, dtype=np.uint64), seed & U32, seed >> 32)
    s32 = np.uint64(32)
    d = ((w0 * np.uint64(D)) >> s32).astype(np.int64)
    a = ((w1 * np.uint64(n)) >> s32).astype(np.int64)
    b = ((w2 * np.uint64(n - 1)) >> s32).astype(np.int64)
    b = b + (b >= a)
    return d, a, b, w3.astype(np.float64) * 2.0 ** -32


def g(R, q):
    """1 / R^q: q - 1 rounded multiplications from the left, one division"""
    r = np.asarray(R).astype(np.float64)
    x = r.copy()
    for _ in range(q - 1):
        x = x * r
    return 1.0 / x


def strided_tree_sum(v):
    """The device's sum of v (..., m): thread k of 256 adds v[k], v[k + 256], ... in that order to 0.0; each wave of 64 halves its lanes
    (lane i += lane i + 32, 16, 8, 4, 2, 1); the result is (w0 + w1) + (w2 + w3) of the four wave sums."""
    v = np.asarray(v, dtype=np.float64)
    lead, m = v.shape[:-1], v.shape[-1]
    rows = -(-m // THREADS)
    pad = np.zeros(lead + (rows * THREADS,))
    pad[..., :m] = v
    pad = pad.reshape(lead + (rows, THREADS))
    s = np.zeros(lead + (THREADS,))
    for k in range(rows):
        s = s + pad[..., k, :]             # a padded 0.0 changes nothing: no partial sum is -0.0
    s = s.reshape(lead + (THREADS // 64, 64)).copy()
    off = 32
    while off:
        s[..., :off] = s[..., :off] + s[..., off:2 * off]
        off >>= 1
    w = s[..., 0]
    return (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])


def _sorted_rows(P):
    return P[np.argsort(P[:, 0], kind="stable")]


def row_sums_general(P, q):
    """r_l of the rows sorted by their first level: the sum over m = l + 1 .. n - 1, ascending, from 0.0, of g(R_lm)"""
    Pc = _sorted_rows(np.asarray(P, dtype=np.int64))
    n = len(Pc)
    r = np.zeros(n)
    for m in range(1, n):
        R = ((Pc[:m] - Pc[m]) ** 2).sum(axis=1)
        r[:m] = r[:m] + g(R, q)
    return r


def row_sums_one_column(n, q):
    """The same for D = 1, where the sorted rows are 0 .. n - 1 whatever P is: R_lm = (m - l)^2, so r_l is the running sum of
    g(1), g(4), ... up to g((n - 1 - l)^2) -- np.cumsum adds in sequence.  test_lhs_host.py holds it to row_sums_general."""
    k = np.arange(1, n, dtype=np.int64)
    run = np.cumsum(g(k * k, q))
    r = np.zeros(n)
    r[:n - 1] = run[::-1]
    return r


def phi(P, q):
    """Phi of one level matrix from scratch, in the device's order"""
    P = np.asarray(P)
    n, D = P.shape
    return float(strided_tree_sum(row_sums_one_column(n, q) if D == 1 else row_sums_general(P, q)))


def criteria(P):
    """(min R, pairs at it) over i < j, exact integers"""
    P = np.asarray(P, dtype=np.int64)
    n, D = P.shape
    if D == 1:                   # a permutation: neighbouring levels are 1 apart, n - 1 such pairs
        return 1, n - 1
    best, cnt = None, 0
    for i0 in range(0, n, 512):
        blk = P[i0:i0 + 512]
        R = ((blk[:, None, :] - P[None, :, :]) ** 2).sum(axis=2)
        R = R[np.arange(i0, i0 + len(blk))[:, None] < np.arange(n)[None, :]]
        if R.size == 0:
            continue
        m = int(R.min())
        k = int((R == m).sum())
        if best is None or m < best:
            best, cnt = m, k
        elif m == best:
            cnt += k
    return best, cnt


def winner(min_r, pairs):
    return min(range(len(min_r)), key=lambda c: (-int(min_r[c]), int(pairs[c]), c))


def lds_bytes(n, D):
    """(wide, bytes) of the chain's level matrix in LDS: 16-bit levels up to n = 65536, above that 16 bits and a one-bit plane over
    n D rounded up to 32"""
    if n <= 65536:
        return False, 2 * n * D
    cells = -(-n * D // 32) * 32
    return True, 2 * cells + cells // 8


def fits(n, D):
    return lds_bytes(n, D)[1] <= LDS_BYTES - LDS_RESERVED


def power_overflows(n, D, q):
    return (D * (n - 1) ** 2) ** q >= 2 ** POWER_BITS


def anneal(start, n_steps, q=5, theta0=0.1, rho=0.9, stage=None, seed=0, stream=0):
    """dict(levels, phi, min_r, pairs, accepted, phi_run) of the chains started at `start` (C, n, D)"""
    P = np.array(start, dtype=np.int64)
    if P.ndim == 2:
        P = P[None]
    C, n, D = P.shape
    stage = max(1, n_steps // 100) if stage is None else stage
    ar = np.arange(C)
    streams = (int(stream) + ar) & U32
    cur = np.array([phi(P[c], q) for c in range(C)])
    best, best_phi = P.copy(), cur.copy()
    accepted = np.zeros(C, dtype=np.int64)
    theta, left = float(theta0), stage
    for t in range(n_steps):
        d, a, b, u = proposal(t, streams, seed, n, D)
        Pa, Pb = P[ar, a], P[ar, b]                                           # (C, D)
        Ra = ((P - Pa[:, None, :]) ** 2).sum(axis=2)                          # (C, n)
        Rb = ((P - Pb[:, None, :]) ** 2).sum(axis=2)
        pj, pad, pbd = P[ar, :, d], Pa[ar, d][:, None], Pb[ar, d][:, None]
        qa, qb = (pad - pj) ** 2, (pbd - pj) ** 2
        Ra2, Rb2 = Ra - qa + qb, Rb - qb + qa
        skip = np.zeros((C, n), dtype=bool)
        skip[ar, a] = True
        skip[ar, b] = True
        for R in (Ra, Rb, Ra2, Rb2):
            R[skip] = 1
        term = (g(Ra2, q) - g(Ra, q)) + (g(Rb2, q) - g(Rb, q))
        term[skip] = 0.0
        delta = strided_tree_sum(term)
        acc = delta <= (theta * u) * cur
        ca = ar[acc]
        P[ca, a[acc], d[acc]], P[ca, b[acc], d[acc]] = pbd[acc, 0], pad[acc, 0]
        cur = np.where(acc, cur + delta, cur)
        accepted += acc
        better = acc & (cur < best_phi)
        best[better] = P[better]
        best_phi = np.where(better, cur, best_phi)
        left -= 1
        if left == 0:
            theta, left = theta * rho, stage
    crit = [criteria(best[c]) for c in range(C)]
    return dict(levels=best, phi=np.array([phi(best[c], q) for c in range(C)]), min_r=np.array([m for m, _ in crit], dtype=np.int64),
                pairs=np.array([k for _, k in crit], dtype=np.int64), accepted=accepted, phi_run=best_phi)
