"""The wavefront LU check (br_debug_wave_lu), the part that needs no GPU: the entry point in the library, the header
and the Python binding, its answers to bad arguments, and the host references the GPU tests compare against
(wave_lu_ref.py)."""
import os
import re

import numpy as np
import pytest

import wave_lu_ref as R
from conftest import ROOT

BR_ERR_INPUT = -10


def test_export_version_and_binding(pkg):
    L = pkg._lib
    lib = L.lib()
    assert lib.br_version() >= 232
    hdr = open(os.path.join(ROOT, "include", "brhip.h")).read()
    assert "br_debug_wave_lu" in L.EXPORTS and hasattr(lib, "br_debug_wave_lu")
    assert re.search(r"\bint\s+br_debug_wave_lu\(", hdr)
    assert callable(pkg.Engine.wave_lu)


def test_bad_arguments_are_input_errors(pkg):
    """every rejection is made on the host before anything is allocated: nothing reaches a GPU"""
    L = pkg._lib
    N, n = 2, 5
    J, v, g = np.zeros((N, n, n)), np.zeros((N, n)), np.ones(N)
    x, f, p = np.zeros((2, N, n)), np.zeros((2, N), np.int32), np.zeros((2, N, n), np.int32)
    F = np.zeros((2, N, R.ws_doubles(n)))

    def call(n_, wpb, perm_in=None, J0=J):
        return L.lib().br_debug_wave_lu(N, n_, wpb, 1, L.dptr(J0), None, L.dptr(g), None, L.dptr(v), L.iptr(perm_in),
                                        L.dptr(x), L.iptr(f), L.iptr(p), L.dptr(F))

    for n_, wpb in ((0, 1), (-1, 1), (73, 1), (5, 0), (5, 5), (20, 5), (53, 17), (66, 13)):
        assert call(n_, wpb) == BR_ERR_INPUT, (n_, wpb)
        assert L.lib().br_last_error().decode()
    for bad in ([0, 1, 2, 3, 3], [0, 1, 2, 3, 5], [-1, 1, 2, 3, 4]):
        pin = np.array([[0, 1, 2, 3, 4], bad], np.int32)
        assert call(n, 1, pin) == BR_ERR_INPUT, bad
    assert call(n, 1, None, None) == BR_ERR_INPUT
    assert not x.any() and not F.any()


def test_instance_widths_and_layout():
    assert [R.nmax_of(n) for n in (1, 16, 17, 32, 33, 56, 57, 64, 65, 72)] == [16, 16, 32, 32, 56, 56, 64, 64, 72, 72]
    assert [R.max_wpb(m) for m in (16, 32, 56, 64, 72)] == [4, 4, 16, 16, 12]
    assert R.ws_doubles(9) == 16 * 16 + 64 and R.ws_doubles(53) == 56 * 56 + 64 and R.ws_doubles(66) == 73 * 80
    src = open(os.path.join(ROOT, "batchreactor.jl_amd", "csrc", "brhip_ctl.hpp")).read()
    assert "n <= 16 ? 16 : (n <= 32 ? 32 : (n <= 56 ? 56 : (n <= 64 ? 64 : 72)))" in src
    assert "nmax > 64 ? (size_t)(nmax + 1) * CR2 : (size_t)nmax * nmax + WAVE" in src


def test_newton_matrix_is_one_rounding_per_entry():
    """the diagonal is the correctly rounded 1 - gamma J_kk (an FMA), not fl(1 - fl(gamma J_kk))"""
    g = np.array([2.0 ** -3 * (1 + 2.0 ** -30)])
    J = np.array([[[8.0 * (1 - 2.0 ** -29), 3.0], [-5.0, 1.0 / 3.0]]])
    A = R.newton_matrix(J, g)
    exact = [[1 - R.Fraction(float(g[0])) * R.Fraction(float(J[0, i, j])) if i == j
              else -R.Fraction(float(g[0])) * R.Fraction(float(J[0, i, j])) for j in range(2)] for i in range(2)]
    for i in range(2):
        for j in range(2):
            assert A[0, i, j] == float(exact[i][j])
    assert A[0, 0, 0] != 1.0 - g[0] * J[0, 0, 0]     # (the two-rounding form differs here)


def test_getrf_order_first_max_and_precisions():
    A = np.array([[1.0, 2.0, 0.0], [-4.0, 1.0, 1.0], [4.0, 0.0, 3.0]])
    assert R.getrf_order(A)[0] == 1 and R.getrf_order(A, R.LD)[0] == 1   # the first of the equal maxima
    rng = np.random.default_rng(5)
    for n in (1, 7, 40):
        B = rng.standard_normal((n, n))
        L, U, orig = R.getrf_f64(B)
        assert np.array_equal(orig, R.getrf_order(B)) and np.array_equal(orig, R.getrf_order(B, R.LD))
        assert np.allclose(L @ U, B[orig], rtol=0, atol=1e-12 * n)


@pytest.mark.parametrize("n", [1, 9, 20, 53, 64, 66, 72])
def test_reconstruction_from_the_device_layout_is_exact(n):
    """A float64 LU written into the device layout (pivots rounded to powers of two, so that D = 1 / D^-1 and
    U = D U' are exact) comes back as exactly those factors, from exactly the positions the header names, and the
    backward ratio against the matrix they multiply to is one rounding's; padding and the unit-lower bound are
    judged as the GPU tests need them."""
    rng = np.random.default_rng(100 + n)
    B = rng.standard_normal((n, n)) * np.exp(rng.uniform(-8, 8, (n, 1)))
    L, U, orig = R.getrf_f64(B)
    D = 2.0 ** np.round(np.log2(np.abs(np.diag(U)))) * np.sign(np.diag(U))
    Up = np.triu(U, 1) / D[:, None]
    F = R.pack(L, Up, 1.0 / D, n, pad=0.0)
    Rr, Cc, ND = R.layout(n)
    assert F.shape == (R.ws_doubles(n),)
    for s, k in ((0, 0), (n - 1, 0), (0, n - 1), (n // 2, n // 3)):
        want = L[s, k] if s > k else (Up[s, k] if s < k else 0.0)
        assert F[k * Rr + s] == want
    assert np.array_equal(F[Rr * Cc:Rr * Cc + n], 1.0 / D) and not F[Rr * Cc + n:].any()
    Lr, Ur = R.factors_ld(F, n)
    assert Lr.dtype == R.LD and np.array_equal(Lr, L.astype(R.LD))
    assert np.array_equal(Ur, (np.triu(U, 1) + np.diag(D)).astype(R.LD))
    A = np.empty((n, n))
    A[orig] = (Lr @ Ur).astype(np.float64)           # the matrix these factors multiply to, rounded once
    assert R.structure_errors(F, n) == []
    assert R.recon_ratio(F, n, A, orig) <= 2.0 ** -52 / R.gamma_k(n + 4)   # that rounding and nothing else
    # the judgements: a NaN or a non-zero in the padding, a NaN in D^-1, a multiplier above 1
    for idx, what in ((0, "diagonal"), (Rr * Cc + ND - 1, "D^-1 beyond n")):
        if what == "diagonal" or n < ND:
            G = F.copy()
            G[idx] = 1.0
            assert what in R.structure_errors(G, n)
    G = F.copy()
    G[Rr * Cc] = np.nan
    assert "D^-1 not finite" in R.structure_errors(G, n)
    if n < Rr:
        G = F.copy()
        G[n] = np.nan                                # row n of column 0
        assert "rows >= n" in R.structure_errors(G, n)
    if n < Cc:
        G = F.copy()
        G[n * Rr] = np.nan                           # row 0 of column n
        assert ("columns >= n" in R.structure_errors(G, n)) == (Rr != 80)
    if n > 1:
        G = F.copy()
        G[1] = 1.0 + 2.0 ** -51                      # L[1][0]
        assert "|L| > 1" in R.structure_errors(G, n)
        H = F.copy()
        H[1] = 2.0 * H[1] + 1.0                      # a wrong multiplier: the bound notices
        assert R.recon_ratio(H, n, A, orig) > 1.0
