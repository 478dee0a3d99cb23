"""The lane engine's own device code (k_lane<9 | 12>, brhip_lane.hpp) against references, kernel by kernel:
lane_tconst / lane_rhs / lane_jac through br_debug_lane_eval against the oracle's rhs and jac, l_getrf /
l_getrs through br_debug_lane_lu_solve against numpy, and whole integrations of lane-eligible mechanisms
WITH falloff reactions (Troe with 3 and 4 parameters, Lindemann, irreversible and three-product reactions).

The falloff mechanisms are subsets of GRI-Mech 3.0 written at test time (test_group_kernels.subset_mechanism).
"""

import os

import numpy as np
import pytest

from conftest import LIB
from test_gpu_parity import TH, _h2o2_with_inerts, close_states
from test_group_kernels import _backward_ok, _getrf_order, _lu_inputs, _wide_states, subset_mechanism

pytestmark = pytest.mark.gpu

LANE_SUBSETS = {"l9": "H2 H O O2 OH H2O HO2 H2O2 N2".split(),
                "l12e": "H2 H O O2 OH H2O CO CO2 HCO CH2O CH3 N2".split()}
CARBON = ("CO", "CO2", "HCO", "CH2O", "CH3")
FACTORS = np.array([0.0, 0.5, 1.0, 2.0, 7.3])


def lane_pair(pkg, orc, tmp_path, mech, conv=None):
    """(product mechanism, oracle mechanism, lane kernel name) of h2o2, h2o2_n12 (three inert species added),
    l9, l9-troe3 or l12e"""
    conv = orc.CONV_REFERENCE if conv is None else conv
    if mech == "h2o2":
        pm = pkg.Mechanism.from_files(LIB, gas_mech="h2o2.dat", conv=conv)
        return pm, orc.Mech(os.path.join(LIB, "h2o2.dat"), TH, None, conv=conv), "k_lane<9>"
    if mech == "h2o2_n12":
        d = _h2o2_with_inerts(tmp_path, 12)
    else:
        key = mech.split("-")[0]
        d = subset_mechanism(tmp_path, LANE_SUBSETS[key], troe3=mech.endswith("-troe3"), name=mech)
    pm = pkg.Mechanism.from_files(d, gas_mech="mech.dat", conv=conv)
    om = orc.Mech(os.path.join(d, "mech.dat"), os.path.join(d, "therm.dat"), None, conv=conv)
    return pm, om, ("k_lane<9>" if pm.n <= 9 else "k_lane<12>")


# ---------------------------------------------------------------------------------------------
# a. lane_tconst + lane_rhs + lane_jac against the oracle (helpers shared with test_wave_kernels.py)
# ---------------------------------------------------------------------------------------------
def multiplier_rows(pm, N, seed):
    """[N, nrg + nrs]: every second reactor's reactions at factors drawn from FACTORS, the others at 1; every
    falloff reaction meets at least three of the factors"""
    nr = pm.nrg + pm.nrs
    mult = np.ones((N, nr))
    mult[1::2] = FACTORS[np.random.default_rng(seed).integers(0, len(FACTORS), (len(mult[1::2]), nr))]
    for r in (np.flatnonzero(pm.tables["g_tb"] == 2) if pm.nrg else ()):
        assert len(set(mult[1::2, r])) >= 3, r
    assert mult.min() == 0.0 and mult.max() == 7.3
    return mult


def reference_states(pm, om, N, seed, mult=None):
    """_wide_states(pm, N, seed) with state 5 holding the reactants of the first falloff reaction at exactly 0
    and state 6 every carbon species at exactly 0 (where the mechanism has them), and the oracle's (du, J)
    at each, reactor i with its row of multipliers. A state the oracle cannot evaluate is replaced (another
    seed), not masked."""
    t = pm.tables
    fo = np.flatnonzero(t["g_tb"] == 2) if pm.nrg else np.zeros(0, int)
    carbon = [pm.gas_species.index(s) for s in CARBON if s in pm.gas_species]
    T, Asv, U = _wide_states(pm, N, seed)
    ref = [None] * N
    try:
        for i in range(N):
            if mult is not None:
                for r in range(pm.nrg + pm.nrs):   # gas reactions in mechanism order, then surface reactions
                    om.set_rxn_mult(r, mult[i, r], mult[i, r])
            for k in range(20):
                if k:
                    Tk, Ak, Uk = _wide_states(pm, N, seed + 97 * k)
                    T[i], Asv[i], U[i] = Tk[i], Ak[i], Uk[i]
                if i == 5 and len(fo):
                    U[i, t["g_f"][fo[0], :t["g_nf"][fo[0]]]] = 0.0
                if i == 6 and carbon:
                    U[i, carbon] = 0.0
                do, _, _ = om.rhs(T[i], Asv[i], U[i])
                Jo = om.jac(T[i], Asv[i], U[i])
                if np.all(np.isfinite(do)) and np.all(np.isfinite(Jo)):
                    ref[i] = (do, Jo)
                    break
            assert ref[i] is not None, i
    finally:
        for r in range((pm.nrg + pm.nrs) if mult is not None else 0):
            om.set_rxn_mult(r, 1.0, 1.0)
    assert T.min() < 1000.0 < T.max()
    return T, Asv, U, ref


def assert_parity(tag, U, du, J, ref):
    """the bars of test_group_rhs_jacobian_parity: |du - do| <= 1e-11 (max_j |Jo_kj| max|u| + |do|), row-wise
    |J - Jo| / max_j |Jo_kj| < 1e-11; prints the worst of each in units of the bar first"""
    e_du, e_j = [], []
    for i, (do, Jo) in enumerate(ref):
        scale = np.abs(Jo).max(1) * np.abs(U[i]).max() + np.abs(do) + 1e-300
        e_du.append(float(np.max(np.abs(du[i] - do) / scale)))
        js = np.abs(Jo).max(1, keepdims=True) + 1e-300
        e_j.append(float(np.max(np.abs(J[i] - Jo) / js)))
    print(f"{tag}: worst du {max(e_du) / 1e-11:.3g} (state {int(np.argmax(e_du))}), worst J {max(e_j) / 1e-11:.3g} "
          f"(state {int(np.argmax(e_j))}), in units of the 1e-11 bar")
    assert np.all(np.isfinite(du)) and np.all(np.isfinite(J)), tag
    for i in range(len(ref)):
        assert e_du[i] <= 1e-11, (tag, i, e_du[i])
        assert e_j[i] < 1e-11, (tag, i, e_j[i])


def lane_eval_blocks(N):
    """workgroups of br_debug_lane_eval's grid (include/brhip.h: one up to 128 reactors, two above); lane l of
    workgroup b evaluates reactors l + 64 (b + k blocks), k = 0, 1, ..."""
    return min(2, (N + 127) // 128)


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def assert_rows_reused(eng, T, U, du, J, ref, tag, rate_mult=None):
    """The N states again, each twice: N + N reversed, 2 N > 128 reactors on two workgroups of which every lane of
    the first takes a second reactor. A state in rows another reactor at another T has used (reversed half) must
    give the bits of the same state in fresh rows, in whichever lane it sits, and both the parity of the oracle."""
    N = len(T)
    idx = np.concatenate([np.arange(N), np.arange(N)[::-1]])
    blocks = lane_eval_blocks(2 * N)
    assert blocks == 2 and 2 * N >= 64 * blocks + 64           # lanes 0..63 of workgroup 0: reactors l and l + 128
    assert np.all(T[idx[128:192]] != T[idx[0:64]])             # ... at another T
    du2, J2 = eng.lane_eval(T[idx], U[idx], rate_mult=None if rate_mult is None else rate_mult[idx])
    assert_parity(tag + ", every state twice on two workgroups", U[idx], du2, J2, [ref[i] for i in idx])
    assert _bits_equal(du2, du[idx]), np.flatnonzero(np.any(du2 != du[idx], axis=1))
    assert _bits_equal(J2, J[idx]), np.flatnonzero(np.any(J2 != J[idx], axis=(1, 2)))


_EVAL_MECHS = ("h2o2", "h2o2_n12", "l9", "l9-troe3", "l12e")


def _lane_engine(pkg, monkeypatch, pm, kernel):
    monkeypatch.setenv("BRHIP_ENGINE", "lane")
    eng = pkg.Engine(pm)
    assert eng.engine == "lane" and eng.kernel_name == kernel, (eng.engine, eng.kernel_name)
    return eng


@pytest.mark.parametrize("conv", [0, 19])
@pytest.mark.parametrize("mech", _EVAL_MECHS)
def test_lane_rhs_jacobian_parity(pkg, orc, gpu, monkeypatch, tmp_path, mech, conv):
    """The lane engine's own T-only constants, RHS and analytic Jacobian (lane_tconst, lane_rhs, lane_jac,
    evaluated by br_debug_lane_eval in k_lane's LDS rows and global rows) against the oracle's rhs / jac at
    the bars of test_group_rhs_jacobian_parity, conv 0 (textbook) and 19 (reference: [M] factor of the
    falloff reactions, Troe c = -4). 100 states on one workgroup: lanes 0..35 evaluate a second reactor at
    another T in the rows of their first while lanes 36..63 wait masked. Then every state twice, 200
    reactors on two workgroups, every lane of the first reusing its rows (assert_rows_reused). T 700-2000 K,
    p 1e3-1e7 Pa (both sides of Pr = 1); state 5 has the reactants of the first falloff reaction at exactly
    0, state 6 every carbon species."""
    assert orc.CONV_REFERENCE == 19
    pm, om, kernel = lane_pair(pkg, orc, tmp_path, mech, conv)
    eng = _lane_engine(pkg, monkeypatch, pm, kernel)
    N = 100
    T, _, U, ref = reference_states(pm, om, N, 31)
    assert lane_eval_blocks(N) == 1 and N > 64                          # reactors 64..99 follow 0..35 in their rows
    assert np.all(T[64:] != T[:N - 64])
    du, J = eng.lane_eval(T, U)
    assert_parity(f"lane_eval {mech} conv {conv}", U, du, J, ref)
    assert_rows_reused(eng, T, U, du, J, ref, f"lane_eval {mech} conv {conv}")


@pytest.mark.parametrize("mech", ["l9", "l12e"])
def test_lane_multipliers_parity(pkg, orc, gpu, monkeypatch, tmp_path, mech):
    """Per-reactor rate multipliers in lane_tconst (k_inf scaled, the stored k0 / k_inf ratio not): every
    second reactor's reactions at factors from {0, 0.5, 1, 2, 7.3}, the falloff reactions among them, against
    the oracle with set_rxn_mult at the same bars; a table of ones gives the bits of the call without one."""
    pm, om, kernel = lane_pair(pkg, orc, tmp_path, mech)
    eng = _lane_engine(pkg, monkeypatch, pm, kernel)
    N = 100
    mult = multiplier_rows(pm, N, 7)
    T, _, U, ref = reference_states(pm, om, N, 31, mult)
    du, J = eng.lane_eval(T, U, rate_mult=mult)
    assert_parity(f"lane_eval {mech} with multipliers", U, du, J, ref)
    # (a lane's second reactor has another row of multipliers: rows of ones and of factors alternate, 64 is even,
    # so in the doubled, reversed run a lane goes from one kind to the other)
    assert_rows_reused(eng, T, U, du, J, ref, f"lane_eval {mech} with multipliers", rate_mult=mult)
    du0, J0 = eng.lane_eval(T, U)
    du1, J1 = eng.lane_eval(T, U, rate_mult=np.ones((1, eng.nr)), rate_mult_row=np.zeros(N, np.int32))
    assert np.array_equal(du1, du0) and np.array_equal(J1, J0)
    assert not np.array_equal(du, du0)
    assert np.array_equal(du[0::2], du0[0::2]) and np.array_equal(J[0::2], J0[0::2])   # (the rows of ones)


def test_lane_eval_needs_a_lane_instance(pkg, gpu):
    """br_debug_lane_eval on a mechanism without a lane instance (GRI, n = 53): BR_ERR_UNSUPPORTED"""
    pm = pkg.Mechanism.from_files(LIB, gas_mech="grimech.dat")
    eng = pkg.Engine(pm)
    with pytest.raises(RuntimeError, match="-30"):
        eng.lane_eval(np.full(1, 1000.0), np.zeros((1, pm.n)))


# ---------------------------------------------------------------------------------------------
# b. l_getrf + l_getrs against numpy
# ---------------------------------------------------------------------------------------------
def _getrf_pivots(A):
    """p[k] of SUNDIALS denseGETRF, from _getrf_order: the position, among the rows as interchanged so far,
    of the original row that ends at position k"""
    orig = _getrf_order(A)
    cur = list(range(len(orig)))
    p = []
    for k, o in enumerate(orig):
        j = cur.index(o)
        p.append(j)
        cur[k], cur[j] = cur[j], cur[k]
    return p


_LU_CASES = [(9, 1), (9, 5), (9, 9), (12, 10), (12, 12)]
_FILL = -7.0


def _skip_pattern(N):
    return (np.arange(N) % 3 == 2).astype(np.int32)


@pytest.mark.parametrize("nm,n", _LU_CASES)
def test_lane_lu_solve(pkg, gpu, nm, n):
    """The lane engine's register LU and solve (l_getrf, l_getrs, factors and reciprocal pivots through the
    g_lu / g_rpv rows) on the matrices of test_batched_lu_solve: 1e-12 backward error, and the pivot rows
    must be denseGETRF's (the first row of largest |a_ik|). Planted in column 0 as in test_group_lu_solve:
    +v / -v ties, values that differ in the low word only, a column of one magnitude next to a lane that
    interchanges. 100 matrices: a ragged second workgroup. Then with every third lane skipped: the others'
    results keep their bits, the skipped outputs their fill values."""
    N = 100
    J, g, b = _lu_inputs(n, N, 100 * nm + n)
    planted = {}
    if n >= 5:
        r1, r2, r3 = 1, n // 2 + 1, n - 1
        assert r1 < r2 < r3
        J[12, 0, 0], J[12, 2, 0] = 0.0, 3.0 / g[12]   # |a_20| = 3 > a_00 = 1: the neighbour of 13 interchanges
        for i, kind in ((9, "pm"), (10, "mp"), (15, "low"), (13, "flat"), (66, "low"), (67, "pm")):
            g[i] = 2.0 ** np.round(np.log2(g[i]))
            big = np.ldexp(1.25, int(np.ceil(np.log2(4 * np.abs(J[i, :, 0]).max() + 4 / g[i]))))   # > every |a_i0|
            if kind == "pm":
                J[i, r1, 0], J[i, r2, 0] = -big, big        # a = +v, -v
            elif kind == "mp":
                J[i, r1, 0], J[i, r2, 0] = big, -big        # a = -v, +v
            elif kind == "low":
                J[i, r1, 0], J[i, r2, 0], J[i, r3, 0] = big, -big * (1 + 2.0 ** -40), big * (1 + 2.0 ** -40)
            else:
                J[i, :, 0] = np.where(np.arange(n) % 2, 1.0, -1.0) / g[i]   # a_i0 = -1, +1, ...
                J[i, 0, 0] = 0.0                                            # a_00 = 1
            planted[i] = {"pm": r1, "mp": r1, "low": r2, "flat": 0}[kind]
            a0 = np.abs((np.arange(n) == 0) - g[i] * J[i, :, 0])      # |column 0| of I - gamma J, exact
            assert int(np.argmax(a0)) == planted[i]
            assert np.sum(a0 == a0.max()) == (n if kind == "flat" else 2)
            if kind == "low":
                assert a0[r1] < a0[r2] and a0[r1].view(np.uint64) >> 32 == a0[r2].view(np.uint64) >> 32
    x, f, piv = pkg.Engine.lane_lu(nm, J, g, b, fill=_FILL)
    assert np.all(f == 0)
    for i in range(N):
        assert _backward_ok(J, g, b, x, i), i
        assert list(piv[i]) == _getrf_pivots(np.eye(n) - g[i] * J[i]), (i, planted.get(i), piv[i])
        assert all(piv[i][k] >= k for k in range(n))
        if i in planted:
            assert piv[i][0] == planted[i], (i, piv[i])
    if n >= 5:
        assert piv[13][0] == 0 and piv[12][0] == 2
    skip = _skip_pattern(N)
    assert not any(skip[i] for i in planted)
    xs, fs, ps = pkg.Engine.lane_lu(nm, J, g, b, skip=skip, fill=_FILL)
    on = skip == 0
    assert np.array_equal(xs[on], x[on]) and np.array_equal(fs[on], f[on]) and np.array_equal(ps[on], piv[on])
    assert np.all(xs[~on] == _FILL) and np.all(fs[~on] == -1) and np.all(ps[~on] == -1)


@pytest.mark.parametrize("nm,n", _LU_CASES)
def test_lane_lu_zero_pivot_flag(pkg, gpu, nm, n):
    """l_getrf's zero-pivot flag: column k of I - gamma J exactly zero (gamma = 0.5, J[:, k] = 2 e_k) for
    k = 0, n // 2, n - 1 gives fail = k + 1 in lanes i = 1, 4, 7, ...; lanes 2, 5, 8, ... are skipped (fill
    values stay); the non-singular neighbours 0, 3, 6, ... are unaffected (fail = 0, 1e-12 backward error,
    denseGETRF's pivot rows)."""
    N = 100
    J, g, b = _lu_inputs(n, N, 200 * nm + n)
    ks = sorted({0, n // 2, n - 1})
    sing = {}
    for c, i in enumerate(range(1, N, 3)):
        k = ks[c % len(ks)]
        g[i] = 0.5
        J[i, :, k] = 0.0
        J[i, k, k] = 2.0
        assert not np.any((np.eye(n) - g[i] * J[i])[:, k])
        sing[i] = k
    assert set(sing.values()) == set(ks)
    skip = _skip_pattern(N)
    x, f, piv = pkg.Engine.lane_lu(nm, J, g, b, skip=skip, fill=_FILL)
    for i in range(N):
        if skip[i]:
            assert f[i] == -1 and np.all(x[i] == _FILL) and np.all(piv[i] == -1), i
        elif i in sing:
            assert f[i] == sing[i] + 1, (i, f[i], sing[i])
        else:
            assert f[i] == 0 and _backward_ok(J, g, b, x, i), (i, f[i])
            assert list(piv[i]) == _getrf_pivots(np.eye(n) - g[i] * J[i]), i


def test_lane_lu_solve_rejects_other_widths(pkg, gpu):
    """nm other than 9 and 12, n < 1 or n > nm: BR_ERR_INPUT"""
    L = pkg._lib
    for nm, n in ((8, 4), (16, 4), (10, 4), (9, 10), (12, 13), (9, 0), (12, -1)):
        m = max(n, 1)
        z, v = np.zeros((1, m, m)), np.zeros((1, m))
        f, p = np.zeros(1, np.int32), np.zeros((1, m), np.int32)
        rc = L.lib().br_debug_lane_lu_solve(nm, 1, n, L.dptr(z), L.dptr(np.ones(1)), L.dptr(v), None, L.dptr(v.copy()),
                                            L.iptr(f), L.iptr(p))
        assert rc == -10, (nm, n, rc)


# ---------------------------------------------------------------------------------------------
# c. integrations of the falloff mechanisms on the lane engine
# ---------------------------------------------------------------------------------------------
def _falloff_ignition_inputs(pm, N, seed):
    """the H2/O2/N2 mixtures of test_gpu_parity._ignition_inputs(pm, "h2o2", N, seed) (T 1000-1400 K, p 0.5-10
    bar, phi 0.5-2); with carbon species N2 is 0.45, CO 0.03 and CH2O 0.02: the carbon falloff reactions are live"""
    rng = np.random.default_rng(seed)
    T = rng.uniform(1000.0, 1400.0, N)
    p = np.exp(rng.uniform(np.log(0.5e5), np.log(1e6), N))
    phi = np.exp(rng.uniform(np.log(0.5), np.log(2), N))
    X = np.zeros((N, pm.ng))
    X[:, pm.gas_species.index("H2")] = 0.5 * 2 * phi / (2 * phi + 1)
    X[:, pm.gas_species.index("O2")] = 0.5 / (2 * phi + 1)
    X[:, pm.gas_species.index("N2")] = 0.5
    if "CO" in pm.gas_species:
        X[:, pm.gas_species.index("N2")] = 0.45
        X[:, pm.gas_species.index("CO")] = 0.03
        X[:, pm.gas_species.index("CH2O")] = 0.02
    assert np.allclose(X.sum(1), 1.0, rtol=0, atol=1e-15)
    U = np.stack([pm.initial_state(T[i], p[i], X[i]) for i in range(N)])
    return T, np.ones(N), U


@pytest.mark.parametrize("mech", ["l9", "l12e"])
def test_lane_engine_falloff_integration(pkg, orc, gpu, monkeypatch, tmp_path, mech):
    """k_lane<9> and k_lane<12> on mechanisms with falloff reactions, eight igniting reactors: end states at
    rtol 1e-10 / atol 1e-16 against the oracle to 1e-6 relative (floor 1e-14) with the analytic and the DQ
    Jacobian on both sides, n RHS per DQ Jacobian, and the wavefront engine's end states to the same bar."""
    pm, om, kernel = lane_pair(pkg, orc, tmp_path, mech)
    eng = _lane_engine(pkg, monkeypatch, pm, kernel)
    N, tf = 8, 1e-2
    T, Asv, U0 = _falloff_ignition_inputs(pm, N, 5)
    Ul = None
    for dq in (False, True):
        U, st = eng.integrate(T, Asv, U0, tf, rtol=1e-10, atol=1e-16, dq_jacobian=dq)
        assert np.all(st["status"] == 0), (dq, np.unique(st["status"]))
        if dq:
            assert np.all(st["nje"] > 0) and np.all(st["nfe_dq"] == st["nje"] * pm.n)
        else:
            Ul = U
        Uo, so, bad = om.integrate_batch(T, Asv, U0, tf, rtol=1e-10, atol=1e-16, analytic_jac=not dq)
        assert bad == 0 and all(s["status"] == 0 for s in so)
        assert all(s["t_ign"] < tf for s in so), [s["t_ign"] for s in so]
        for i in range(N):
            e = close_states(U[i], Uo[i], rtol=1e-6, floor=1e-14)
            assert e <= 1.0, (dq, i, e)
    monkeypatch.setenv("BRHIP_ENGINE", "wave")
    assert eng.engine == "wave"
    Uw, sw = eng.integrate(T, Asv, U0, tf, rtol=1e-10, atol=1e-16)
    assert np.all(sw["status"] == 0)
    assert max(close_states(Ul[i], Uw[i], rtol=1e-6, floor=1e-14) for i in range(N)) <= 1.0
