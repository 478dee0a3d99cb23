"""Host references of the wavefront LU tests (test_wave_lu.py, test_wave_lu_host.py): the Newton matrix as the
device forms it, denseGETRF's pivot order in long double, the device layout of the factor workspace
(include/brhip.h, br_debug_wave_lu), the factors rebuilt from it in long double and the componentwise backward
bound. No GPU, no library."""
from fractions import Fraction

import numpy as np

LD = np.longdouble
U53 = 2.0 ** -53                                     # unit roundoff of the device arithmetic


def nmax_of(n):
    """width of the k_integrate instance of an n-component system (brhip_ctl.hpp)"""
    return 16 if n <= 16 else 32 if n <= 32 else 56 if n <= 56 else 64 if n <= 64 else 72


def max_wpb(nmax):
    """br_maxrpb: the most waves per workgroup the integrator launches for the width"""
    return 12 if nmax > 64 else 16 if nmax in (56, 64) else 4


def layout(n):
    """(rows per column, columns, entries of D^-1) of the factor workspace"""
    nmax = nmax_of(n)
    return (80, 72, 80) if nmax > 64 else (nmax, nmax, 64)


def ws_doubles(n):
    R, C, ND = layout(n)
    return R * C + ND


def newton_matrix(J, g):
    """I - gamma J [N, n, n] in float64 as lu_factor / lu_factor2 form it: every entry is c - gamma * J_ij
    contracted into one fused multiply-add (c = 1 on the diagonal, else 0), so one rounding of the exact value.
    Off the diagonal that is -fl(gamma J_ij); the diagonal is rounded from the exact rational here."""
    J = np.asarray(J, dtype=np.float64)
    g = np.asarray(g, dtype=np.float64)
    A = -(g[:, None, None] * J)
    N, n, _ = J.shape
    for i in range(N):
        gi = Fraction(float(g[i]))
        for k in range(n):
            A[i, k, k] = float(1 - gi * Fraction(float(J[i, k, k])))
    return A


def getrf_order(A, dtype=np.float64):
    """pivot order of SUNDIALS denseGETRF in `dtype` arithmetic: at step k the first row of largest |a_ik| among
    the (already interchanged) rows k..n-1; orig[s] = the original row at position s. (test_group_kernels'
    _getrf_order is this routine in float64.)"""
    A = np.array(A, dtype=dtype)
    n = A.shape[0]
    orig = np.arange(n)
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))     # (argmax: the first of equal maxima)
        if p != k:
            A[[k, p]] = A[[p, k]]
            orig[[k, p]] = orig[[p, k]]
        if A[k, k] == 0:
            break
        A[k + 1:, k] /= A[k, k]
        A[k + 1:, k + 1:] -= np.outer(A[k + 1:, k], A[k, k + 1:])
    return orig


def getrf_f64(A):
    """(L, U, orig) of the same elimination in float64 (unit lower L, upper U, L U = A[orig] up to rounding)"""
    A = np.array(A, dtype=np.float64)
    n = A.shape[0]
    orig = np.arange(n)
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        if p != k:
            A[[k, p]] = A[[p, k]]
            orig[[k, p]] = orig[[p, k]]
        A[k + 1:, k] /= A[k, k]
        A[k + 1:, k + 1:] -= np.outer(A[k + 1:, k], A[k, k + 1:])
    return np.tril(A, -1) + np.eye(n), np.triu(A), orig


def unpack(F, n):
    """(M, Dinv) views of one workspace copy F [W]: M[s, k] = row s of factor column k (all rows and columns of
    the layout), Dinv the stored D^-1 entries"""
    R, C, ND = layout(n)
    assert F.shape == (R * C + ND,)
    return F[:R * C].reshape(C, R).T, F[R * C:]


def pack(L, Uprime, Dinv, n, pad=0.0):
    """the workspace of factors in step order: column k holds L[s][k] on rows s > k, U'[s][k] on rows s < k and 0
    on s = k, then D^-1; everything outside rows and columns < n is `pad`, D^-1 beyond n is 0"""
    R, C, ND = layout(n)
    M = np.full((R, C), pad)
    M[:n, :n] = np.tril(L, -1) + np.triu(Uprime, 1)
    D = np.zeros(ND)
    D[:n] = Dinv
    return np.concatenate([M.T.reshape(-1), D])


def factors_ld(F, n):
    """(L, U) in long double from a workspace copy: L[s][k] below the diagonal (unit diagonal), U = D U' above it
    and D on it, D = 1 / D^-1"""
    assert np.finfo(LD).eps <= 2.0 ** -63, "long double is not wider than double here"
    M, Dinv = unpack(F, n)
    Ms = M[:n, :n].astype(LD)
    D = LD(1) / Dinv[:n].astype(LD)
    L = np.tril(Ms, -1) + np.eye(n, dtype=LD)
    U = np.triu(Ms, 1) * D[:, None] + np.diag(D)
    return L, U


def gamma_k(k):
    return k * U53 / (1 - k * U53)


def recon_ratio(F, n, A, perm):
    """max over the entries of |L U - P A| / (gamma_(n+4) (|L| |U|)), in long double, P A = A[perm]: the standard
    componentwise LU backward bound (n roundings) with four more for 1 / piv, a * dinv and D = 1 / D^-1, D U'."""
    L, U = factors_ld(F, n)
    err = np.abs(L @ U - A[perm].astype(LD))
    bound = LD(gamma_k(n + 4)) * (np.abs(L) @ np.abs(U))
    if not (np.all(np.isfinite(err)) and np.all(np.isfinite(bound))):
        return np.inf
    if np.any((bound == 0) & (err > 0)):
        return np.inf
    nz = bound > 0
    return float(np.max(err[nz] / bound[nz])) if np.any(nz) else 0.0


def backward_ratio(A, b, x):
    """max|A x - b| / (|A|_inf |x|_inf + |b|_inf): the project's solve check bounds it by 1e-12"""
    res = A @ x - b
    return float(np.max(np.abs(res)) / (np.abs(A).sum(1).max() * np.abs(x).max() + np.abs(b).max()))


def structure_errors(F, n):
    """what lu_solve / lu_solve2 rely on in a workspace copy (rows in step order); returns the violations"""
    R, C, ND = layout(n)
    M, Dinv = unpack(F, n)
    bad = []
    if np.any(M[np.arange(n), np.arange(n)] != 0.0):
        bad.append("diagonal")
    if np.any(M[n:, :n] != 0.0):
        bad.append("rows >= n")
    if R != 80 and np.any(M[:, n:] != 0.0):          # CPL = 1: the solve reads the padding columns' lines
        bad.append("columns >= n")
    if not np.all(np.isfinite(Dinv)):
        bad.append("D^-1 not finite")
    if np.any(Dinv[n:] != 0.0):
        bad.append("D^-1 beyond n")
    if not np.all(np.abs(np.tril(M[:n, :n], -1)) <= 1.0 + 2.0 ** -52):   # (a NaN fails this too)
        bad.append("|L| > 1")
    return bad
