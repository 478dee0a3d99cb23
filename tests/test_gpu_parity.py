"""Parity of the HIP path (libbrhip.so, called through the C-ABI) against the CPU oracle.

Tolerances (north_star: production rates within 1e-12 relative; trajectories within 1e-4):
  * rates / RHS: |gpu - oracle| <= 1e-12 * scale_k, scale_k = sum_r |nu_kr q_r| (the magnitude
    of the terms summed into species k, so near-equilibrium cancellation is judged against
    the size of the contributions, not against their tiny difference) + 1e-300;
  * Jacobian: row-wise 1e-11 * max_j |J_kj|;
  * integrated states: |u_gpu - u_oracle| <= 1e-4 |u_oracle| + 100 atol for every component
    (1e-4 relative with an absolute floor of 100x the solver's abstol = 1e-8 kg/m3: both runs
    meet the same local error test but take rounding-dependent step sequences, so components
    near abstol can only agree to within a multiple of abstol).
"""

import os

import numpy as np
import pytest

from conftest import LIB, ROOT

pytestmark = pytest.mark.gpu
TH = os.path.join(LIB, "therm.dat")
SURF_GAS = ["CH4", "H2O", "H2", "CO", "CO2", "O2", "N2"]

ATOL = 1e-10


def close_states(u, uo, rtol=1e-4, floor=100 * ATOL):
    err = np.abs(u - uo) / (rtol * np.abs(uo) + floor)
    return float(err.max())

CASES = {
    "h2o2": dict(gas="h2o2.dat", surf=None),
    "gri": dict(gas="grimech.dat", surf=None),
    "surf": dict(gas=None, surf="ch4ni.xml"),
    "gas_surf": dict(gas="grimech.dat", surf="ch4ni.xml"),   # n = 66: two components per lane
}


def _mechs(pkg, orc, case, conv=None):
    """product and oracle mechanisms for a case; conv None = the reference conventions (default)"""
    conv = orc.CONV_REFERENCE if conv is None else conv
    c = CASES[case]
    gm = c["gas"]
    pm = pkg.Mechanism.from_files(LIB, gas_mech=gm, surface_mech=c["surf"], gasphase=None if gm else SURF_GAS, conv=conv)
    om = orc.Mech(os.path.join(LIB, gm) if gm else None, TH, os.path.join(LIB, c["surf"]) if c["surf"] else None,
                  gas_species=None if gm else SURF_GAS, conv=conv)
    return pm, om


def _states(pm, N, seed):
    rng = np.random.default_rng(seed)
    T = rng.uniform(900.0, 1400.0, N)
    p = np.exp(rng.uniform(np.log(0.5e5), np.log(1e6), N))
    x = rng.random((N, pm.ng)) ** 4 + 1e-12
    x /= x.sum(1, keepdims=True)
    th = rng.random((N, pm.ns)) ** 3 + 1e-14
    if pm.ns:
        th /= th.sum(1, keepdims=True)
    return T, p, x, th


def _scale(pm, qg, qs):
    """sum_r |nu_kr q_r| per species."""
    t = pm.tables
    sc = np.zeros(pm.n)
    for r in range(pm.nrg):
        for e in range(t["g_nf"][r]):
            sc[t["g_f"][r, e]] += abs(qg[r])
        for e in range(t["g_nr"][r]):
            sc[t["g_r"][r, e]] += abs(qg[r])
    for r in range(pm.nrs):
        for e in range(t["s_nf"][r]):
            sc[t["s_f"][r, e]] += abs(qs[r])
        for e in range(t["s_np"][r]):
            sc[t["s_p"][r, e]] += abs(qs[r])
    return sc


@pytest.mark.parametrize("conv", [0, 19], ids=["textbook", "reference"])
@pytest.mark.parametrize("case", ["h2o2", "gri", "surf", "gas_surf"])
def test_rates_parity(pkg, orc, gpu, case, conv):
    pm, om = _mechs(pkg, orc, case, conv)
    eng = pkg.Engine(pm)
    N = 64
    T, p, x, th = _states(pm, N, 11)
    w, s = eng.rates(T, p, x, th if pm.ns else None)
    for i in range(N):
        wo, so = om.rates(T[i], p[i], x[i], th[i] if pm.ns else None)
        qg, qs = om.rop(T[i], p[i], x[i], th[i] if pm.ns else None)
        sc = _scale(pm, qg, qs)
        assert np.all(np.abs(w[i] - wo) <= 1e-12 * sc[:pm.ng] + 1e-300), (case, i)
        if pm.ns:
            assert np.all(np.abs(s[i] - so) <= 1e-12 * sc + 1e-300), (case, i)


@pytest.mark.parametrize("conv", [0, 19], ids=["textbook", "reference"])
@pytest.mark.parametrize("case", ["h2o2", "gri", "surf", "gas_surf"])
def test_rhs_and_jacobian_parity(pkg, orc, gpu, case, conv):
    pm, om = _mechs(pkg, orc, case, conv)
    eng = pkg.Engine(pm)
    N = 16
    T, p, x, th = _states(pm, N, 12)
    Asv = np.exp(np.random.default_rng(3).uniform(0, np.log(100), N))
    U = np.stack([pm.initial_state(T[i], p[i], x[i], th[i] if pm.ns else None) for i in range(N)])
    # half the states get small negative entries (post-ignition solver states have them)
    neg = np.random.default_rng(4).random(U.shape) < 0.15
    U[N // 2:] = np.where(neg[N // 2:], -1e-3 * np.abs(U[N // 2:]), U[N // 2:])
    du = eng.rhs(T, Asv, U)
    J = eng.jacobian(T, Asv, U)
    for i in range(N):
        do, pp, xx = om.rhs(T[i], Asv[i], U[i])
        Jo = om.jac(T[i], Asv[i], U[i])
        scale = np.abs(Jo).max(1) * np.abs(U[i]).max() + np.abs(do) + 1e-300
        assert np.all(np.abs(du[i] - do) <= 1e-11 * scale), (case, i)
        js = np.abs(Jo).max(1, keepdims=True) + 1e-300
        assert np.max(np.abs(J[i] - Jo) / js) < 1e-11, (case, i)


@pytest.mark.parametrize("switch", ["BRHIP_JFAST", "BRHIP_SPREAD"])
def test_jacobian_parity_host_layout_switches(pkg, orc, gpu, monkeypatch, switch):
    """the A/B layouts behind the host switches (general column-list Jacobian; LDS scatter lists
    in first-appearance order) stay parity-green on GRI, same bar as the default layout"""
    monkeypatch.setenv(switch, "0")
    pm, om = _mechs(pkg, orc, "gri")
    eng = pkg.Engine(pm)
    N = 8
    T, p, x, th = _states(pm, N, 21)
    Asv = np.ones(N)
    U = np.stack([pm.initial_state(T[i], p[i], x[i]) for i in range(N)])
    du = eng.rhs(T, Asv, U)
    J = eng.jacobian(T, Asv, U)
    for i in range(N):
        do, _, _ = om.rhs(T[i], Asv[i], U[i])
        Jo = om.jac(T[i], Asv[i], U[i])
        scale = np.abs(Jo).max(1) * np.abs(U[i]).max() + np.abs(do) + 1e-300
        assert np.all(np.abs(du[i] - do) <= 1e-11 * scale), (switch, i)
        js = np.abs(Jo).max(1, keepdims=True) + 1e-300
        assert np.max(np.abs(J[i] - Jo) / js) < 1e-11, (switch, i)


def _ignition_inputs(pm, case, N, seed):
    rng = np.random.default_rng(seed)
    if case == "surf":
        T = rng.uniform(973.0, 1173.0, N)
        p = np.full(N, 1e5)
        sc = rng.uniform(1, 3, N)
        X = np.zeros((N, pm.ng))
        X[:, pm.gas_species.index("CH4")] = 0.5 / (1 + sc)
        X[:, pm.gas_species.index("H2O")] = 0.5 * sc / (1 + sc)
        X[:, pm.gas_species.index("N2")] = 0.5
        Asv = np.exp(rng.uniform(0, np.log(100), N))
    elif case == "h2o2":
        T = rng.uniform(1000.0, 1400.0, N)
        p = np.exp(rng.uniform(np.log(0.5e5), np.log(1e6), N))
        phi = np.exp(rng.uniform(np.log(0.5), np.log(2), N))
        X = np.zeros((N, pm.ng))
        X[:, pm.gas_species.index("H2")] = 0.5 * 2 * phi / (2 * phi + 1)
        X[:, pm.gas_species.index("O2")] = 0.5 / (2 * phi + 1)
        X[:, pm.gas_species.index("N2")] = 0.5
        Asv = np.ones(N)
    else:
        T = rng.uniform(1100.0, 1300.0, N)
        p = np.exp(rng.uniform(np.log(1e5), np.log(1e6), N))
        phi = rng.uniform(0.5, 1.5, N)
        X = np.zeros((N, pm.ng))
        X[:, pm.gas_species.index("CH4")] = 0.75 * phi / (phi + 2)
        X[:, pm.gas_species.index("O2")] = 1.5 / (phi + 2)
        X[:, pm.gas_species.index("N2")] = 0.25
        Asv = np.ones(N)
    U = np.stack([pm.initial_state(T[i], p[i], X[i]) for i in range(N)])
    return T, Asv, U


def _global_err(X, Ut):
    """max over species (above 1e-6 of the reactor's largest component) of |X - Ut| / |Ut|"""
    e = np.abs(X - Ut) / (np.abs(Ut) + 1e-6 * np.abs(Ut).max(axis=1, keepdims=True))
    return e.max(axis=1)


# Per-reactor parity at default tolerances (rtol 1e-6, atol 1e-10, src/BatchReactor.jl:141,:210),
# 0 -> 10 s through ignition, on a slice of the synthetic ensemble (bench inputs),
# at fixed output times (CVODE CV_NORMAL output through br_opts.tout), against per-case bounds set
# from the oracle's own rounding spread (tests/parity_bands.py, profiles/r04_parity_spread.json).
from parity_bands import OUT_T, BOUNDS, band_errors as _band_errors  # noqa: E402
_BANDS = ((0.0, 0.5, 1.0), (0.5, 2.0, 300.0), (2.0, np.inf, 30.0))   # coarse bounds of the dense-output edge test


@pytest.mark.parametrize("case,N,dq", [("h2o2", 256, False), ("gri", 64, False), ("surf", 64, False),
                                      ("gas_surf", 32, False), ("h2o2", 256, True), ("gri", 32, True),
                                      ("gas_surf", 16, True), ("surf", 64, True)],
                         ids=["h2o2", "gri", "surf", "gas_surf", "h2o2-dq", "gri-dq", "gas_surf-dq", "surf-dq"])
def test_integrate_parity(pkg, orc, gpu, case, N, dq):
    """Every reactor: same status (Success), the same ignition time to within the width of the
    ignition step (the marker's resolution), states at the 28 output times within the case's bounds
    (tests/parity_bands.py: 2x the oracle's own rounding spread across and after the front), the same
    step count to 35 % per reactor and 3 % over the slice (rounding changes step sequences).
    Both engines use the analytic Jacobian by default; the "-dq" cases run CVODE's DQ Jacobian
    (br_opts.dq_jacobian, the reference's setting: the quad engine for H2/O2, the wavefront engine
    for GRI, gas+surface and the 32-wide-vector surface-only case) against the oracle's DQ run."""
    from batchreactor_amd import ensemble
    pm, om = _mechs(pkg, orc, case)
    eng = pkg.Engine(pm)
    analytic = not dq
    T, Asv, U0 = ensemble.make_inputs(pm, case, 0, N)
    U, st = eng.integrate(T, Asv, U0, 10.0, tout=OUT_T, dq_jacobian=dq)
    assert np.all(st["status"] == 0), np.unique(st["status"])
    worst = np.zeros(3)
    nst_o = 0
    bounds = BOUNDS[(case, dq)]
    for i in range(N):
        uo, so, Yo = om.integrate_out(T[i], Asv[i], U0[i], 10.0, OUT_T, analytic_jac=analytic)
        assert so["status"] == 0
        ti = so["t_ign"]
        if pm.ng > 7:   # gas-phase mechanisms carry the OH marker; it resolves ignition to one step
            assert abs(st["t_ign"][i] - ti) <= bounds[3] * max(st["ign_dt"][i], so["ign_dt"]) + 1e-4 * ti, \
                (case, i, st["t_ign"][i], ti, st["ign_dt"][i], so["ign_dt"])
        eb = _band_errors(st["yout"][i], Yo, ti)
        worst = np.maximum(worst, eb)
        for w, (bound, e) in enumerate(zip(bounds[:3], eb)):
            assert e <= bound, (case, dq, i, ("pre", "front", "post")[w], e, bound)
        assert abs(st["nsteps"][i] - so["nsteps"]) <= 0.35 * so["nsteps"], (i, st["nsteps"][i], so["nsteps"])
        nst_o += so["nsteps"]
    assert abs(st["nsteps"].sum() / nst_o - 1) <= 0.03, (st["nsteps"].sum(), nst_o)
    if dq:
        assert np.all(st["nfe_dq"] == st["nje"] * pm.n), "DQ Jacobian: n RHS per Jacobian"
    print(f"\n  {case}{' (DQ)' if dq else ''}: worst error per band (units of 1e-4|u|+1e-8): {worst}, bounds {bounds[:3]}")


@pytest.mark.parametrize("dq", [False, True], ids=["analytic", "dq"])
def test_ignition_time_and_golden_rows_on_gpu(pkg, gpu, dq):
    """The HIP engine on the reference's own gas+surf case (test/batch_gas_and_surf: GRI + ch4ni,
    T = 1173 K, Asv = 1, rtol 1e-6 / atol 1e-10): ignition (max dX_OH/dt, br_stats.t_ign) at the
    golden's 3.8109e-3 s to 1e-3, the golden's accepted-step count (1,918) to 10 %, and every
    committed golden row (state at the same time through br_opts.tout) within the per-window bounds
    the oracle is held to (tests/test_oracle.py). "dq": the wavefront engine with CVODE's DQ
    Jacobian, the reference's own setting (src/BatchReactor.jl:204-210)."""
    import csv
    import json
    from conftest import GOLDEN
    from test_oracle import _WINDOWS, _WINDOWS_ADMISSIBLE

    def golden(name):
        rows = list(csv.reader(open(os.path.join(GOLDEN, name))))
        return np.array([[float(v) for v in r[1:]] for r in rows[1:]])

    g = golden("gas_and_surf_golden.csv")
    s = golden("gas_and_surf_covg_golden.csv")
    meta = json.load(open(os.path.join(GOLDEN, "golden_meta.json")))
    pm = pkg.Mechanism.from_files(LIB, gas_mech="grimech.dat", surface_mech="ch4ni.xml")
    x = pm.mole_fractions({"CH4": 0.25, "O2": 0.5, "N2": 0.25})
    u0 = pm.initial_state(1173.0, 1e5, x)
    tg = g[:, 0]
    U, st = pkg.Engine(pm).integrate([1173.0], [1.0], u0[None, :], 10.0, tout=tg, dq_jacobian=dq)
    assert st["status"][0] == 0
    print(f"\n  golden gas+surf ({'DQ' if dq else 'analytic'} J): {int(st['nsteps'][0])} steps "
          f"(golden {meta['accepted_steps']}), t_ign {st['t_ign'][0]:.6e}")
    assert abs(st["t_ign"][0] / meta["t_ign_max_dXOH_dt"] - 1) < 1e-3, st["t_ign"][0]
    assert abs(st["nsteps"][0] / meta["accepted_steps"] - 1) < 0.1
    Y = st["yout"][0]
    X = pm.state_to_molefrac(Y)
    G = g[:, 4:]
    ex = np.where(np.abs(G) >= 1e-4, np.abs(X - G) / np.maximum(np.abs(G), 1e-300), 0.0).max(axis=1)
    S = s[:, 2:]
    es = np.where(np.abs(S) >= 1e-4, np.abs(Y[:, pm.ng:] - S) / np.maximum(np.abs(S), 1e-300), 0.0).max(axis=1)
    for lo, hi, tol, tolc in (_WINDOWS_ADMISSIBLE if dq else _WINDOWS):
        sel = (tg >= lo) & (tg < hi)
        assert ex[sel].max() < tol and es[sel].max() < tolc, (lo, hi, ex[sel].max(), es[sel].max())


@pytest.mark.parametrize("case,N,dq", [("h2o2", 64, False), ("gri", 32, False), ("surf", 32, False),
                                      ("gas_surf", 16, False), ("gri", 64, True), ("gas_surf", 32, True),
                                      ("surf", 64, True), ("h2o2", 64, True)],
                         ids=["h2o2", "gri", "surf", "gas_surf", "gri-dq", "gas_surf-dq", "surf-dq", "h2o2-dq"])
def test_integrate_parity_tight(pkg, orc, gpu, case, N, dq):
    """Tight tolerances (rtol 1e-10, atol 1e-16) on both sides: the two integrations converge to the
    same trajectory, so the end states (tf = 1e-2 s, through ignition for the gas cases) must agree
    to 1e-6 relative (absolute floor 1e-14 kg/m3). "-dq": both with CVODE's DQ Jacobian (the
    wavefront engine's dq_jacobian path against the oracle's cvLsDenseDQJac)."""
    pm, om = _mechs(pkg, orc, case)
    eng = pkg.Engine(pm)
    T, Asv, U0 = _ignition_inputs(pm, case, N, 6)
    tf = 1e-2
    U, st = eng.integrate(T, Asv, U0, tf, rtol=1e-10, atol=1e-16, dq_jacobian=dq)
    assert np.all(st["status"] == 0)
    if dq:
        assert np.all(st["nfe_dq"] == st["nje"] * pm.n)
    Uo, so, bad = om.integrate_batch(T, Asv, U0, tf, rtol=1e-10, atol=1e-16, analytic_jac=not dq, nthreads=8)
    assert bad == 0 and all(s["status"] == 0 for s in so)
    for i in range(N):
        e = close_states(U[i], Uo[i], rtol=1e-6, floor=1e-14)
        assert e <= 1.0, (case, i, e)


def test_integrate_edge_cases(pkg, orc, gpu):
    pm, om = _mechs(pkg, orc, "h2o2")
    eng = pkg.Engine(pm)
    T, Asv, U0 = _ignition_inputs(pm, "h2o2", 4, 9)
    U, st = eng.integrate(T[:0], Asv[:0], U0[:0], 1.0)                  # empty ensemble
    assert U.shape == (0, pm.n)
    tf = np.array([1e-6, 1e-3, 1.0, 10.0])                              # ragged end times
    U, st = eng.integrate(T, Asv, U0, tf)
    for i in range(4):
        uo, so, _ = om.integrate(T[i], Asv[i], U0[i], tf[i], analytic_jac=True)
        assert close_states(U[i], uo) <= 1.0
    U1, st1 = eng.integrate(T[:1], Asv[:1], U0[:1], 10.0, max_steps=5)  # step limit -> CV_TOO_MUCH_WORK
    assert st1["status"][0] == -1


def test_mass_conservation_full_size(pkg, gpu):
    """Size-independent property at a large ensemble: total gas mass is invariant for gas-only
    chemistry (sum_k du_k = 0), so sum(u) at tf equals sum(u0) to the integration tolerance."""
    pm = pkg.Mechanism.from_files(LIB, gas_mech="h2o2.dat")
    eng = pkg.Engine(pm)
    T, Asv, U0 = _ignition_inputs(pm, "h2o2", 4096, 21)
    U, st = eng.integrate(T, Asv, U0, 1.0)
    assert np.all(st["status"] == 0)
    np.testing.assert_allclose(U.sum(1), U0.sum(1), rtol=1e-6)


def test_programmatic_api(pkg, gpu):
    """batch_reactor(inlet_comp, T, p, time; chem, thermo_obj, md) (test/runtests.jl:51-67)."""
    m = pkg.Mechanism.from_files(LIB, gas_mech="h2o2.dat")
    t, xd = pkg.batch_reactor_programmatic({"O2": 0.25, "N2": 0.5, "H2": 0.25}, 1073.15, 1e5, 10.0,
                                           chem=pkg.Chemistry(gaschem=True), mech=m)
    assert t[-1] == 10.0 and abs(sum(xd.values()) - 1) < 1e-12


@pytest.mark.parametrize("n", [9, 20, 53, 60, 66, 72])   # k_lu_check<16 | 32 | 56 | 64>, k_lu_check2<72> (twice)
def test_batched_lu_solve(pkg, gpu, n):
    """The integrator's row-per-lane LU (partial pivoting, no row swaps) + solve against numpy on
    random, ill-scaled Newton matrices I - gamma J (fp64; 1e-12 backward-error bound); then with
    singular matrices in between: the zero-pivot flag k + 1 (as denseGETRF)."""
    import ctypes as C
    rng = np.random.default_rng(n)
    N = 64
    J = rng.standard_normal((N, n, n)) * np.exp(rng.uniform(-8, 8, (N, n, 1)))
    g = np.exp(rng.uniform(-12, -2, N))
    b = rng.standard_normal((N, n))
    x = np.zeros((N, n))
    f = np.zeros(N, np.int32)
    L = pkg._lib.lib()
    rc = L.br_debug_lu_solve(N, n, pkg._lib.dptr(J), pkg._lib.dptr(g), pkg._lib.dptr(b), pkg._lib.dptr(x),
                             f.ctypes.data_as(C.POINTER(C.c_int)))
    assert rc == 0 and np.all(f == 0)
    for i in range(N):
        A = np.eye(n) - g[i] * J[i]
        res = A @ x[i] - b[i]
        assert np.max(np.abs(res)) <= 1e-12 * (np.abs(A).sum(1).max() * np.abs(x[i]).max() + np.abs(b[i]).max())
    # the zero-pivot flag: column k of I - gamma J exactly zero (gamma = 0.5, J[:, k] = 2 e_k) gives
    # fail = k + 1; the matrices in between are as above
    ks = (0, n // 2, n - 1)
    sing = {}
    for c, i in enumerate(range(1, N, 3)):
        k = ks[c % 3]
        g[i] = 0.5
        J[i, :, k] = 0.0
        J[i, k, k] = 2.0
        sing[i] = k
    rc = L.br_debug_lu_solve(N, n, pkg._lib.dptr(J), pkg._lib.dptr(g), pkg._lib.dptr(b), pkg._lib.dptr(x),
                             f.ctypes.data_as(C.POINTER(C.c_int)))
    assert rc == 0
    for i in range(N):
        if i in sing:
            assert f[i] == sing[i] + 1, (i, f[i], sing[i])
            continue
        assert f[i] == 0, (i, f[i])
        A = np.eye(n) - g[i] * J[i]
        res = A @ x[i] - b[i]
        assert np.max(np.abs(res)) <= 1e-12 * (np.abs(A).sum(1).max() * np.abs(x[i]).max() + np.abs(b[i]).max())


@pytest.mark.parametrize("n", [33, 53, 64])
def test_batched_lu_solve_mfma(pkg, gpu, n):
    """The MFMA-blocked LU (lu_factor_mf: 8-column panels, trailing updates X += E' X[piv] on
    v_mfma_f64_16x16x4f64; measured slower in the integrator, profiles/r04_lu_mfma_ab.json, so it
    lives in the variant library libbrhip_lumf.so, not in libbrhip.so) + the product's solve, the
    same matrices and backward-error bound as test_batched_lu_solve; factored twice (natural row
    order, then the first factorization's pivot order)."""
    import ctypes as C
    rng = np.random.default_rng(n)
    N = 64
    J = rng.standard_normal((N, n, n)) * np.exp(rng.uniform(-8, 8, (N, n, 1)))
    g = np.exp(rng.uniform(-12, -2, N))
    b = rng.standard_normal((N, n))
    x = np.zeros((N, n))
    f = np.zeros(N, np.int32)
    path = os.path.join(os.path.dirname(pkg._lib.__file__), "libbrhip_lumf.so")
    assert os.path.exists(path), "variant library not built (make -C batchreactor.jl_amd/csrc)"
    fn = C.CDLL(path).br_debug_lu_solve_mf
    fn.restype = C.c_int
    rc = fn(N, n, pkg._lib.dptr(J), pkg._lib.dptr(g), pkg._lib.dptr(b), pkg._lib.dptr(x),
            f.ctypes.data_as(C.POINTER(C.c_int)))
    assert rc == 0 and np.all(f == 0)
    for i in range(N):
        A = np.eye(n) - g[i] * J[i]
        res = A @ x[i] - b[i]
        assert np.max(np.abs(res)) <= 1e-12 * (np.abs(A).sum(1).max() * np.abs(x[i]).max() + np.abs(b[i]).max())


def test_coop_lu_solve_bit_identical(pkg, gpu):
    """The cooperative-engine experiment (scripts/micro/coop_lusolve.hip, not
    part of libbrhip.so; profiles/r06_coop_ab.json): the LU factors held in the registers of a 4-wave
    workgroup, with a barrier per step or per 16-column panel, give bit-for-bit the integrator's
    lu_factor<56> / lu_solve<56> results (pivoting included: scaled random matrices, the first LU in
    natural row order, later ones in the previous pivot order), within the backward-error bound."""
    import ctypes as C
    path = os.path.join(ROOT, "scripts", "micro", "libcoop.so")
    assert os.path.exists(path), "experiment library not built (make -C scripts/micro libcoop.so)"
    lib = C.CDLL(path)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    lib.coop_run.argtypes = [C.c_int, C.c_int, C.c_int, dp, C.c_int, dp, dp, C.c_int, C.c_int, dp, dp, ip, dp, ip]
    rng = np.random.default_rng(11)
    n, N, nj, reps, nsolve = 53, 256, 64, 2, 3
    J = np.ascontiguousarray(rng.standard_normal((nj, n, n)) * np.exp(rng.uniform(-8, 8, (nj, n, 1))))
    g = np.ascontiguousarray(np.exp(rng.uniform(-12, -2, N)))
    b = np.ascontiguousarray(rng.standard_normal((N, n)))
    P = lambda a: a.ctypes.data_as(dp)  # noqa: E731
    outs = {}
    for mode in (0, 1, 3):
        x, chk, f = np.zeros((N, n)), np.zeros((N, n)), np.zeros(N, np.int32)
        ms, vg = C.c_double(0.0), C.c_int(0)
        assert lib.coop_run(mode, N, n, P(J), nj, P(g), P(b), reps, nsolve, P(x), P(chk), f.ctypes.data_as(ip),
                            C.byref(ms), C.byref(vg)) == 0
        assert np.all(f == 0)
        outs[mode] = (x, chk)
    for mode in (1, 3):
        assert np.array_equal(outs[mode][0].view(np.int64), outs[0][0].view(np.int64)), mode
        assert np.array_equal(outs[mode][1].view(np.int64), outs[0][1].view(np.int64)), mode
    x = outs[0][0]
    for i in range(0, N, 17):
        A = np.eye(n) - g[i] * J[i % nj]
        res = A @ x[i] - b[i] * nsolve
        assert np.max(np.abs(res)) <= 1e-12 * (np.abs(A).sum(1).max() * np.abs(x[i]).max() + nsolve * np.abs(b[i]).max())


def test_cvset_lane_parallel_matches_plain(gpu):
    """The lane-parallel BDF coefficient update (cv_set_lp: independent divisions spread over the
    lanes of a DPP row, row broadcasts, zero coefficients for unused orders) and the shared root of
    the three step-size ratios return the plain forms' bits (cv_set, one root_int per ratio) on random
    controller states of every order / qwait / nst case (scripts/micro/cvset_check.hip, the whole
    integrator translation unit)."""
    import ctypes as C
    path = os.path.join(ROOT, "scripts", "micro", "libcvset_check.so")
    assert os.path.exists(path), "check library not built (make -C scripts/micro libcvset_check.so)"
    N = 4096
    rng = np.random.default_rng(3)
    iin = np.zeros((N, 4), np.int32)
    iin[:, 0] = rng.integers(1, 6, N)
    iin[:, 1] = rng.integers(0, 3, N)
    iin[:, 2] = rng.choice([0, 7], N)
    din = np.zeros((N, 10))
    h = 10.0 ** rng.uniform(-9, -2, N)
    din[:, 0] = h
    din[:, 1] = h * rng.uniform(0.06, 1.5, N)
    for i in range(1, 7):
        din[:, 2 + i] = h * rng.uniform(0.3, 3.0, N)
    din[:, 9] = 10.0 ** rng.uniform(-3, 1, N)
    out = np.zeros((N, 16, 2, 16))
    lib = C.CDLL(path)
    assert lib.cvset_check(N, din.ctypes.data_as(C.c_void_p), iin.ctypes.data_as(C.c_void_p),
                           out.ctypes.data_as(C.c_void_p)) == 0
    a, b = out[:, :, 0, :], out[:, :, 1, :]
    assert np.array_equal(a.view(np.int64), b.view(np.int64))


def test_gas_surf_golden_early_steps(pkg, gpu):
    """The reference's own gas+surface output (test/batch_gas_and_surf, GRI + ch4ni, T = 1173 K,
    Asv = 1, rtol 1e-6 / atol 1e-10; tests/golden/gas_and_surf_*golden.csv) against the engine's
    per-step trace of the same run (n = 66, two components per lane): the first 11 accepted step
    times to 1e-4, coverages above 1e-12 and the surface-driven gas species to 1e-4 relative, and
    the pressure of the last RHS evaluation (save_data semantics, src/BatchReactor.jl:383-402)."""
    import csv
    from conftest import GOLDEN

    def golden(name):
        rows = list(csv.reader(open(os.path.join(GOLDEN, name))))
        return np.array([[float(v) for v in r[1:]] for r in rows[1:]]), [int(r[0]) for r in rows[1:]]

    g, idx = golden("gas_and_surf_golden.csv")
    s, _ = golden("gas_and_surf_covg_golden.csv")
    assert idx[:12] == list(range(12))
    pm = pkg.Mechanism.from_files(LIB, gas_mech="grimech.dat", surface_mech="ch4ni.xml")
    assert pm.n == 66
    x = pm.mole_fractions({"CH4": 0.25, "O2": 0.5, "N2": 0.25})
    u0 = pm.initial_state(1173.0, 1e5, x)
    eng = pkg.Engine(pm)
    U, st, tr = eng.integrate(np.array([1173.0]), np.array([1.0]), u0[None, :], 10.0, trace_cap=12, max_steps=12)
    rows = tr[0]
    M = np.asarray(pm.molwt)
    n = pm.n
    for i in range(1, 12):
        t, p, u = rows[i, 0], rows[i, 3], rows[i, 4 + n:4 + 2 * n]    # last-RHS state (save_data)
        assert abs(t / g[i, 0] - 1) < 1e-4, (i, t, g[i, 0])
        th = u[pm.ng:]
        gth = s[i, 2:]
        big = gth > 1e-12
        assert np.max(np.abs(th[big] / gth[big] - 1)) < 1e-4, (i, t)
        xm = (u[:pm.ng] / M) / np.sum(u[:pm.ng] / M)
        for name in ("H2O", "CH4", "O2", "N2"):
            k = pm.gas_species.index(name)
            assert abs(xm[k] / g[i, 4 + k] - 1) < 1e-4, (i, name)
        assert abs(p / g[i, 2] - 1) < 1e-9, (i, p, g[i, 2])
        assert abs(rows[i, 4:4 + pm.ng].sum() / g[i, 3] - 1) < 1e-6, i       # rho from the accepted u


def test_file_driven_gas_surf_profiles(pkg, gpu, tmp_path):
    """batch_reactor(input_file, lib_dir; surfchem, gaschem) on test/batch_gas_and_surf (the
    reference's testset "Batch gas and surface chemistry", test/runtests.jl:31-35): returns
    "Success" and writes gas_profile / surface_covg .dat + .csv with one row per accepted step
    (save_data, src/BatchReactor.jl:383-402). Against the reference's own CSVs: same headers, every
    CSV token in Julia's string(Float64) format, the first 11 rows (step times, p, rho,
    surface-driven species, coverages), the ignition time from the written OH column (max dX/dt
    between rows, as the golden's) to 1e-3, the final row at t = 10 s (species >= 1e-4 to 1e-3) and
    the step count within 10 % of the reference's 1918."""
    import csv
    import json
    import shutil
    from conftest import GOLDEN
    d = tmp_path / "batch_gas_and_surf"
    d.mkdir()
    shutil.copy(os.path.join(GOLDEN, "batch_gas_and_surf", "batch.xml"), d / "batch.xml")
    ret = pkg.batch_reactor(str(d / "batch.xml"), LIB, surfchem=True, gaschem=True)
    assert ret == "Success"
    gas = list(csv.reader(open(d / "gas_profile.csv")))
    cov = list(csv.reader(open(d / "surface_covg.csv")))
    ref = list(csv.reader(open(os.path.join(GOLDEN, "gas_and_surf_golden.csv"))))
    refc = list(csv.reader(open(os.path.join(GOLDEN, "gas_and_surf_covg_golden.csv"))))
    meta = json.load(open(os.path.join(GOLDEN, "golden_meta.json")))
    assert gas[0] == ref[0][1:] and cov[0] == refc[0][1:]          # fixture rows carry a row index
    assert abs(len(gas) - 1 - meta["accepted_steps"]) <= 0.1 * meta["accepted_steps"] and len(cov) == len(gas)
    assert gas[-1][0] == "10.0"
    for r in gas[1:] + cov[1:]:
        for tok in r:
            assert pkg.julia_string(float(tok)) == tok, tok
    hdr = gas[0]

    def rel(a, b, tol):
        return abs(a - b) <= tol * abs(b)

    for i in range(1, 13):                                           # CSV rows 1..12 = steps 0..11
        g = np.array([float(v) for v in gas[i]])
        r = np.array([float(v) for v in ref[i][1:]])
        assert rel(g[0], r[0], 1e-4) and rel(g[2], r[2], 1e-9) and rel(g[3], r[3], 1e-6), (i, g[:4], r[:4])
        for name in ("H2O", "CH4", "O2", "N2"):
            k = hdr.index(name)
            assert rel(g[k], r[k], 1e-4), (i, name)
        c = np.array([float(v) for v in cov[i]])[2:]
        rc = np.array([float(v) for v in refc[i][1:]])[2:]
        big = rc > 1e-12
        assert np.max(np.abs(c[big] / rc[big] - 1)) < 1e-4, i
    G = np.array([[float(v) for v in r] for r in gas[1:]])
    k = hdr.index("OH")
    dx = np.diff(G[:, k]) / np.diff(G[:, 0])
    j = int(np.argmax(dx))
    assert abs(0.5 * (G[j, 0] + G[j + 1, 0]) / meta["t_ign_max_dXOH_dt"] - 1) < 1e-3
    last, rlast = G[-1], np.array([float(v) for v in ref[-1][1:]])
    big = np.abs(rlast[4:]) >= 1e-4
    assert np.max(np.abs(last[4:][big] / rlast[4:][big] - 1)) < 1e-3
    dat = open(d / "gas_profile.dat").read().splitlines()
    assert len(dat) == len(gas) and dat[0].split() == hdr


@pytest.mark.parametrize("scenario,chem", [("batch_surf", dict(surfchem=True)), ("batch_h2o2", dict(gaschem=True)),
                                           ("batch_ch4", dict(gaschem=True))])
def test_reference_file_scenarios(pkg, orc, gpu, tmp_path, scenario, chem):
    """The reference's file-driven testsets (test/runtests.jl:13-29: surface, H2/O2 = config C1,
    GRI CH4) through batch_reactor on the GPU: "Success", the four output files, the last row at
    t = tf, and the final state against the oracle's run of the same input (the file path traces its
    rows, so it runs on the wavefront engine with the analytic Jacobian, and the oracle uses the
    analytic Jacobian too): species >= 1e-6 to 1e-3 relative."""
    import csv
    import shutil
    from conftest import GOLDEN
    d = tmp_path / scenario
    d.mkdir()
    shutil.copy(os.path.join(GOLDEN, scenario, "batch.xml"), d / "batch.xml")
    assert pkg.batch_reactor(str(d / "batch.xml"), LIB, **chem) == "Success"
    for f in ("gas_profile.dat", "gas_profile.csv", "surface_covg.dat", "surface_covg.csv"):
        assert (d / f).exists()
    gas = list(csv.reader(open(d / "gas_profile.csv")))
    mech, x, T, p0, Asv, tf = pkg.compile_mechanism(str(d / "batch.xml"), LIB, pkg.Chemistry(**chem))
    assert float(gas[-1][0]) == tf
    eng = pkg.Engine(mech)
    om = orc.Mech(os.path.join(LIB, mech_file) if (mech_file := {"batch_surf": None, "batch_h2o2": "h2o2.dat",
                                                                 "batch_ch4": "grimech.dat"}[scenario]) else None,
                  os.path.join(LIB, "therm.dat"), os.path.join(LIB, "ch4ni.xml") if scenario == "batch_surf" else None,
                  gas_species=None if mech_file else mech.gas_species)
    u0 = mech.initial_state(T, p0, x)
    uo, so, _ = om.integrate(T, Asv, u0, tf, analytic_jac=True)   # traced runs use the wavefront engine
    assert so["status"] == 0
    xo = mech.state_to_molefrac(uo)
    xg = np.array([float(v) for v in gas[-1][4:]])
    big = xo >= 1e-6
    assert np.max(np.abs(xg[big] / xo[big] - 1)) < 1e-3, scenario
    if scenario == "batch_surf":
        cov = list(csv.reader(open(d / "surface_covg.csv")))
        assert cov[0] == ["t", "T"] + mech.surf_species and len(cov) == len(gas)
        th = np.array([float(v) for v in cov[-1][2:]])
        bt = uo[mech.ng:] >= 1e-6
        assert np.max(np.abs(th[bt] / uo[mech.ng:][bt] - 1)) < 1e-3


def test_doc_surface_rows_on_gpu(pkg, gpu):
    """docs/src/index.md:160-185 (batch_surf inputs, Asv = 10; the sample predates the Asv factor
    on dtheta/dt, CONV_DOC_COVG) on the HIP engine through dense output at the printed times: gas
    to 2e-3, coverages to 1e-2 (4-5 printed digits), as the oracle (tests/test_oracle.py)."""
    import csv
    from conftest import GOLDEN
    m = pkg.Mechanism.from_files(LIB, surface_mech="ch4ni.xml", gasphase=SURF_GAS,
                                 conv=pkg.CONV_REFERENCE | pkg.CONV_DOC_COVG)
    x = m.mole_fractions({"CH4": 0.25, "H2O": 0.25, "N2": 0.5})
    u0 = m.initial_state(1073.15, 1e5, x)
    rows = list(csv.reader(open(os.path.join(GOLDEN, "doc_surf_rows.csv"))))
    gas = {float(r[2]): np.array([float(v) for v in r[6:]]) for r in rows if r[1] == "gas"}
    surf = {float(r[2]): np.array([float(v) for v in r[4:]]) for r in rows if r[1] == "surf"}
    tout = np.array(sorted(t for t in set(gas) | set(surf) if t > 0))
    U, st = pkg.Engine(m).integrate([1073.15], [10.0], u0[None, :], 10.0, tout=tout)
    assert st["status"][0] == 0
    checked = 0
    for j, t in enumerate(tout):
        y = st["yout"][0, j]
        if t in gas and t > 1e-11:
            big = gas[t] > 1e-10
            assert np.max(np.abs(m.state_to_molefrac(y)[big] / gas[t][big] - 1)) < 2e-3, t
            checked += 1
        if t in surf and t > 1e-11:
            big = surf[t] > 1e-10
            assert np.max(np.abs(y[m.ng:][big] / surf[t][big] - 1)) < 1e-2, t
            checked += 1
    assert checked >= 6


def test_surface_programmatic_species_order(pkg, gpu):
    """Reference testset "surface chemistry with interface call" (test/runtests.jl:37-49): the
    species list is collect(keys(inlet_comp)) in Julia Dict order (src/BatchReactor.jl:103); the
    engine matches species by name, so any key order gives the same end state, and t[end] == t."""
    comp = {"CH4": 0.25, "H2O": 0.0, "H2": 0.0, "CO": 0.0, "CO2": 0.25, "O2": 0.0, "N2": 0.5}
    res = []
    for order in (list(comp), list(reversed(list(comp))), ["N2", "CO2", "H2", "CH4", "O2", "CO", "H2O"]):
        c = {k: comp[k] for k in order}
        m = pkg.Mechanism.from_files(LIB, surface_mech="ch4ni.xml", gasphase=list(c))
        t, xd = pkg.batch_reactor_programmatic(c, 1073.15, 1e5, 10, Asv=10.0, chem=pkg.Chemistry(surfchem=True), mech=m)
        assert t[-1] == 10
        assert list(xd) == order        # the returned Dict's keys are inlet_comp's (:103, :145)
        res.append(xd)
    for xd in res[1:]:
        for k in comp:
            assert abs(xd[k] - res[0][k]) <= 1e-4 * abs(res[0][k]) + 1e-12, k   # summation order: rounding


def test_ensemble_api(pkg, orc, gpu):
    """batch_reactor_ensemble: N reactors with their own T, p and composition in one call; x_end,
    theta_end and t_ign per reactor against the oracle run of each (same analytic Jacobian)."""
    m = pkg.Mechanism.from_files(LIB, gas_mech="grimech.dat", surface_mech="ch4ni.xml")
    om = orc.Mech(os.path.join(LIB, "grimech.dat"), TH, os.path.join(LIB, "ch4ni.xml"))
    N = 6
    T = np.linspace(1120.0, 1240.0, N)
    p = np.full(N, 1e5)
    X = np.zeros((N, m.ng))
    phi = np.linspace(0.6, 1.4, N)
    X[:, m.gas_species.index("CH4")] = 0.75 * phi / (phi + 2)
    X[:, m.gas_species.index("O2")] = 1.5 / (phi + 2)
    X[:, m.gas_species.index("N2")] = 0.25
    xe, the, st = pkg.batch_reactor_ensemble(m, T, p, X, 10.0, Asv=1.0)
    assert xe.shape == (N, m.ng) and the.shape == (N, m.ns) and np.all(st["status"] == 0)
    for i in range(N):
        uo, so, _ = om.integrate(T[i], 1.0, m.initial_state(T[i], p[i], X[i]), 10.0, analytic_jac=True)
        xo = m.state_to_molefrac(uo)
        big = xo >= 1e-4
        assert np.max(np.abs(xe[i][big] / xo[big] - 1)) < 1e-3
        assert abs(st["t_ign"][i] / so["t_ign"] - 1) < 1e-4


def test_dense_output_edge_cases(pkg, orc, gpu):
    """br_opts.tout: outputs at t <= 0 return u0; outputs past a reactor's tf stay untouched;
    repeated times give identical rows; a ragged tf per reactor; the end-time output equals u(tf);
    for both engines (lane: H2/O2; wavefront: surface)."""
    for case in ("h2o2", "surf"):
        pm, om = _mechs(pkg, orc, case)
        eng = pkg.Engine(pm)
        T, Asv, U0 = _ignition_inputs(pm, case, 4, 5)
        tf = np.array([1e-3, 1e-2, 1.0, 10.0])
        tout = np.array([0.0, 1e-4, 1e-3, 1e-3, 0.5, 1.0, 20.0])
        U, st = eng.integrate(T, Asv, U0, tf, tout=tout)
        Y = st["yout"]
        assert np.all(st["status"] == 0)
        for i in range(4):
            np.testing.assert_array_equal(Y[i, 0], U0[i])
            np.testing.assert_array_equal(Y[i, 2], Y[i, 3])
            for j, t in enumerate(tout):
                if t > tf[i]:
                    assert np.all(Y[i, j] == 0.0), (case, i, j)
                if t == tf[i]:
                    assert close_states(Y[i, j], U[i], rtol=1e-12, floor=1e-20) <= 1.0
            sel = tout <= tf[i]
            uo, so, Yo = om.integrate_out(T[i], Asv[i], U0[i], tf[i], tout[sel], analytic_jac=True)
            e = (np.abs(Y[i][sel] - Yo) / (1e-4 * np.abs(Yo) + 100 * ATOL)).max(axis=1)
            ti = so["t_ign"] if so["t_ign"] == so["t_ign"] else np.inf
            r = tout[sel] / ti
            for lo, hi, bound in _BANDS:
                assert e[(r >= lo) & (r < hi)].max(initial=0.0) <= bound, (case, i, lo, hi)


def test_lane_engine_h2o2(pkg, orc, gpu, monkeypatch):
    """One-reactor-per-lane engine (k_lane: small gas mechanisms, CVODE's DQ Jacobian as the
    reference's CVODE_BDF) against the oracle run with the same DQ Jacobian. N = 200 > 64 lanes
    per wave, so lanes take new reactors from the work counter mid-run. Tight tolerances: end
    states agree to 1e-6 relative; default tolerances: same status and, summed over the
    ensemble, the same step / RHS / Jacobian counts to 10 % (rounding changes step sequences)."""
    monkeypatch.setenv("BRHIP_ENGINE", "lane")
    pm, om = _mechs(pkg, orc, "h2o2")
    eng = pkg.Engine(pm)
    assert eng.engine == "lane"
    N = 200
    T, Asv, U0 = _ignition_inputs(pm, "h2o2", N, 6)
    tf = np.where(np.arange(N) % 3 == 0, 1e-3, 1e-2)            # ragged end times
    U, st = eng.integrate(T, Asv, U0, tf, rtol=1e-10, atol=1e-16, dq_jacobian=True)
    assert np.all(st["status"] == 0)
    for i in range(N):
        uo, so, _ = om.integrate(T[i], Asv[i], U0[i], tf[i], analytic_jac=False, rtol=1e-10, atol=1e-16)
        assert so["status"] == 0
        e = close_states(U[i], uo, rtol=1e-6, floor=1e-14)
        assert e <= 1.0, (i, e)
    U, st = eng.integrate(T, Asv, U0, 1e-2, dq_jacobian=True)
    Ud, std_, _ = om.integrate_batch(T, Asv, U0, 1e-2, analytic_jac=False, nthreads=8)
    sd = np.array([s["status"] for s in std_])
    assert np.array_equal(st["status"] == 0, sd == 0)
    ok = (st["status"] == 0) & (sd == 0)
    for key in ("nsteps", "nfe", "nje"):
        g = float(st[key][ok].sum())
        o = float(sum(std_[i][key] for i in np.nonzero(ok)[0]))
        assert abs(g - o) <= 0.1 * o, (key, g, o)
    assert np.max([close_states(U[i], Ud[i], rtol=1e-3) for i in np.nonzero(ok)[0]]) <= 1.0


def test_lane_and_wave_engines_agree(pkg, gpu, monkeypatch):
    """The two integrator engines (per-lane DQ Jacobian, per-wavefront analytic Jacobian) give the
    same H2/O2 end states at tight tolerances."""
    pm = pkg.Mechanism.from_files(LIB, gas_mech="h2o2.dat")
    T, Asv, U0 = _ignition_inputs(pm, "h2o2", 96, 8)
    monkeypatch.setenv("BRHIP_ENGINE", "lane")
    eng = pkg.Engine(pm)
    assert eng.engine == "lane"
    Ul, sl = eng.integrate(T, Asv, U0, 1e-2, rtol=1e-10, atol=1e-16)
    monkeypatch.setenv("BRHIP_ENGINE", "wave")
    assert eng.engine == "wave"
    Uw, sw = eng.integrate(T, Asv, U0, 1e-2, rtol=1e-10, atol=1e-16)
    assert np.all(sl["status"] == 0) and np.all(sw["status"] == 0)
    assert max(close_states(Ul[i], Uw[i], rtol=1e-6, floor=1e-14) for i in range(96)) <= 1.0


def test_quad_engine_h2o2(pkg, orc, gpu, monkeypatch):
    """Four-reactors-per-wave engine (k_group<16, NM>, "quad": one reactor per 16-lane DPP row, the wavefront
    engine's CVODE controller instantiated for 16-lane groups, analytic Jacobian, LU in registers).
    N = 200 with ragged end times: groups take new reactors from the work counter while the other
    groups of their wave are mid-run. Tight tolerances: end states agree with the oracle to 1e-6
    relative. Default tolerances with dense output: ignition time, the per-window bounds of
    test_integrate_parity and the step counts as there."""
    monkeypatch.setenv("BRHIP_ENGINE", "quad")
    pm, om = _mechs(pkg, orc, "h2o2")
    eng = pkg.Engine(pm)
    assert eng.engine == "quad" and eng.kernel_name == "k_group<16, 9>"
    N = 200
    T, Asv, U0 = _ignition_inputs(pm, "h2o2", N, 6)
    tf = np.where(np.arange(N) % 3 == 0, 1e-3, 1e-2)            # ragged end times
    U, st = eng.integrate(T, Asv, U0, tf, rtol=1e-10, atol=1e-16)
    assert np.all(st["status"] == 0), np.unique(st["status"])
    for i in range(N):
        uo, so, _ = om.integrate(T[i], Asv[i], U0[i], tf[i], analytic_jac=True, rtol=1e-10, atol=1e-16)
        assert so["status"] == 0
        assert close_states(U[i], uo, rtol=1e-6, floor=1e-14) <= 1.0, i
    from batchreactor_amd import ensemble
    N = 128
    T, Asv, U0 = ensemble.make_inputs(pm, "h2o2", 0, N)
    U, st = eng.integrate(T, Asv, U0, 10.0, tout=OUT_T)
    assert np.all(st["status"] == 0)
    bounds = BOUNDS[("h2o2", False)]
    nst_o = 0
    for i in range(N):
        uo, so, Yo = om.integrate_out(T[i], Asv[i], U0[i], 10.0, OUT_T, analytic_jac=True)
        ti = so["t_ign"]
        assert abs(st["t_ign"][i] - ti) <= bounds[3] * max(st["ign_dt"][i], so["ign_dt"]) + 1e-4 * ti, i
        eb = _band_errors(st["yout"][i], Yo, ti)
        for w, (bound, e) in enumerate(zip(bounds[:3], eb)):
            assert e <= bound, (i, ("pre", "front", "post")[w], e, bound)
        assert abs(st["nsteps"][i] - so["nsteps"]) <= 0.35 * so["nsteps"], (i, st["nsteps"][i], so["nsteps"])
        nst_o += so["nsteps"]
    assert abs(st["nsteps"].sum() / nst_o - 1) <= 0.03, (st["nsteps"].sum(), nst_o)


def test_launch_info_follows_the_engine(pkg, orc, gpu, monkeypatch):
    """br_mech_launch_info (the bench line's roofline.launch) describes the engine br_integrate
    launches: the quad engine's workgroups hold 4 reactors per wave, the wavefront engine's one, the lane
    engine's one wave of 64 reactors (within its 64 KB of LDS), the pair engine's 2 reactors per wave."""
    pm, _ = _mechs(pkg, orc, "h2o2")
    monkeypatch.setenv("BRHIP_ENGINE", "quad")
    q = pkg.Engine(pm).launch_info
    monkeypatch.setenv("BRHIP_ENGINE", "wave")
    w = pkg.Engine(pm).launch_info
    assert q["reactors_per_workgroup"] % 4 == 0 and q["reactors_per_workgroup"] >= 4, q
    assert 1 <= q["waves_per_cu"] <= 32 and 1 <= w["waves_per_cu"] <= 32, (q, w)
    assert 0 < q["lds_bytes_per_workgroup"] <= 160 * 1024 and 0 < w["lds_bytes_per_workgroup"] <= 160 * 1024
    assert q != w
    monkeypatch.setenv("BRHIP_ENGINE", "lane")
    le = pkg.Engine(pm)
    assert le.engine == "lane"
    ln = le.launch_info
    assert ln["reactors_per_workgroup"] == 64 and ln["waves_per_cu"] >= 1, ln
    assert 0 < ln["lds_bytes_per_workgroup"] <= 64 * 1024, ln
    sm, _ = _mechs(pkg, orc, "surf")
    monkeypatch.setenv("BRHIP_ENGINE", "pair")
    pe = pkg.Engine(sm)
    assert pe.engine == "pair"
    p = pe.launch_info
    assert p["reactors_per_workgroup"] % 2 == 0 and p["reactors_per_workgroup"] >= 2, p
    assert 1 <= p["waves_per_cu"] <= 32 and 0 < p["lds_bytes_per_workgroup"] <= 160 * 1024, p


def test_quad_engine_dq_jacobian(pkg, orc, gpu, monkeypatch):
    """The quad engine with CVODE's DQ Jacobian (br_opts.dq_jacobian, the reference's setting): n RHS per
    Jacobian counted in nfe_dq, states at the 28 output times within the H2/O2-DQ bounds of
    test_integrate_parity against the oracle's cvLsDenseDQJac run, the same ignition time and step
    counts; tight tolerances: end states to 1e-6 relative."""
    monkeypatch.setenv("BRHIP_ENGINE", "quad")
    from batchreactor_amd import ensemble
    pm, om = _mechs(pkg, orc, "h2o2")
    eng = pkg.Engine(pm)
    assert eng.engine == "quad"
    N = 128
    T, Asv, U0 = ensemble.make_inputs(pm, "h2o2", 0, N)
    U, st = eng.integrate(T, Asv, U0, 10.0, tout=OUT_T, dq_jacobian=True)
    assert np.all(st["status"] == 0)
    assert np.all(st["nfe_dq"] == st["nje"] * pm.n)
    bounds = BOUNDS[("h2o2", True)]
    nst_o = 0
    for i in range(N):
        uo, so, Yo = om.integrate_out(T[i], Asv[i], U0[i], 10.0, OUT_T, analytic_jac=False)
        ti = so["t_ign"]
        assert abs(st["t_ign"][i] - ti) <= bounds[3] * max(st["ign_dt"][i], so["ign_dt"]) + 1e-4 * ti, i
        eb = _band_errors(st["yout"][i], Yo, ti)
        for w, (bound, e) in enumerate(zip(bounds[:3], eb)):
            assert e <= bound, (i, ("pre", "front", "post")[w], e, bound)
        nst_o += so["nsteps"]
    assert abs(st["nsteps"].sum() / nst_o - 1) <= 0.03, (st["nsteps"].sum(), nst_o)
    T, Asv, U0 = _ignition_inputs(pm, "h2o2", 64, 6)
    U, st = eng.integrate(T, Asv, U0, 1e-2, rtol=1e-10, atol=1e-16, dq_jacobian=True)
    assert np.all(st["status"] == 0)
    for i in range(64):
        uo, so, _ = om.integrate(T[i], Asv[i], U0[i], 1e-2, analytic_jac=False, rtol=1e-10, atol=1e-16)
        assert close_states(U[i], uo, rtol=1e-6, floor=1e-14) <= 1.0, i


def test_quad_engine_step_budget_and_wave_agreement(pkg, orc, gpu, monkeypatch):
    """Quad engine: max_steps = 60 stops every reactor that needs more with BR_ERR_MAXSTEPS (-1) after
    exactly 60 steps, as the oracle's CVODE run; and the quad and wavefront engines (same
    controller, same analytic Jacobian) give the same end states at tight tolerances."""
    pm, om = _mechs(pkg, orc, "h2o2")
    eng = pkg.Engine(pm)
    T, Asv, U0 = _ignition_inputs(pm, "h2o2", 96, 12)
    monkeypatch.setenv("BRHIP_ENGINE", "quad")
    assert eng.engine == "quad"
    U, st = eng.integrate(T[:64], Asv[:64], U0[:64], 10.0, max_steps=60)
    for i in range(64):
        _, so, _ = om.integrate(T[i], Asv[i], U0[i], 10.0, analytic_jac=True, max_steps=60)
        assert so["status"] == -1 and so["nsteps"] == 60
        assert st["status"][i] == -1 and st["nsteps"][i] == 60, (i, st["status"][i], st["nsteps"][i])
    Uq, sq = eng.integrate(T, Asv, U0, 1e-2, rtol=1e-10, atol=1e-16)
    monkeypatch.setenv("BRHIP_ENGINE", "wave")
    Uw, sw = eng.integrate(T, Asv, U0, 1e-2, rtol=1e-10, atol=1e-16)
    assert np.all(sq["status"] == 0) and np.all(sw["status"] == 0)
    assert max(close_states(Uq[i], Uw[i], rtol=1e-6, floor=1e-14) for i in range(96)) <= 1.0


def test_pair_engine_surface(pkg, orc, gpu, monkeypatch):
    """Two-reactors-per-wave engine (k_group<32, 24>, "pair": one reactor per 32-lane half, surface
    chemistry with coverage-dependent activation and sticking, the Asv quirk) on the surface-only
    Ni/CH4 case (n = 20) against the oracle: the per-window bounds of test_integrate_parity at the 28
    output times on a slice of the bench ensemble, step counts to 35 % / 3 %; tight tolerances with
    per-reactor Asv in [1, 100]: end states to 1e-6 relative; the DQ Jacobian path: n RHS per Jacobian
    and the same end states; and the same end states as the wavefront engine."""
    monkeypatch.setenv("BRHIP_ENGINE", "pair")
    from batchreactor_amd import ensemble
    pm, om = _mechs(pkg, orc, "surf")
    eng = pkg.Engine(pm)
    assert eng.engine == "pair" and eng.kernel_name == "k_group<32, 24>", eng.kernel_name
    N = 64
    T, Asv, U0 = ensemble.make_inputs(pm, "surf", 0, N)
    U, st = eng.integrate(T, Asv, U0, 10.0, tout=OUT_T)
    assert np.all(st["status"] == 0), np.unique(st["status"])
    bounds = BOUNDS[("surf", False)]
    nst_o = 0
    for i in range(N):
        uo, so, Yo = om.integrate_out(T[i], Asv[i], U0[i], 10.0, OUT_T, analytic_jac=True)
        assert so["status"] == 0
        eb = _band_errors(st["yout"][i], Yo, so["t_ign"])
        for w, (bound, e) in enumerate(zip(bounds[:3], eb)):
            assert e <= bound, (i, w, e, bound)
        assert abs(st["nsteps"][i] - so["nsteps"]) <= 0.35 * so["nsteps"], (i, st["nsteps"][i], so["nsteps"])
        nst_o += so["nsteps"]
    assert abs(st["nsteps"].sum() / nst_o - 1) <= 0.03, (st["nsteps"].sum(), nst_o)
    N = 48
    T, Asv, U0 = _ignition_inputs(pm, "surf", N, 6)
    for dq in (False, True):
        U, st = eng.integrate(T, Asv, U0, 1e-2, rtol=1e-10, atol=1e-16, dq_jacobian=dq)
        assert np.all(st["status"] == 0)
        if dq:
            assert np.all(st["nfe_dq"] == st["nje"] * pm.n)
        for i in range(N):
            uo, so, _ = om.integrate(T[i], Asv[i], U0[i], 1e-2, analytic_jac=not dq, rtol=1e-10, atol=1e-16)
            assert so["status"] == 0
            assert close_states(U[i], uo, rtol=1e-6, floor=1e-14) <= 1.0, (dq, i)
    Up, sp_ = eng.integrate(T, Asv, U0, 1e-2, rtol=1e-10, atol=1e-16)
    monkeypatch.setenv("BRHIP_ENGINE", "wave")
    Uw, sw = eng.integrate(T, Asv, U0, 1e-2, rtol=1e-10, atol=1e-16)
    assert np.all(sw["status"] == 0)
    assert max(close_states(Up[i], Uw[i], rtol=1e-6, floor=1e-14) for i in range(N)) <= 1.0


def _h2o2_with_inerts(tmp_path, n):
    """H2/O2 with inert (reaction-free) species appended from the thermo library up to n components:
    gas mechanisms of 12, 20 and 30 species for the group engines' other register widths (the bench
    mechanisms have n = 9 and 53)"""
    import shutil
    th = [ln for ln in open(TH).read().split("\n")]
    names = [ln[:18].split()[0] for ln in th if len(ln) >= 80 and ln[79] == "1"]
    base = "H2 O2 H2O H O OH HO2 H2O2 N2".split()
    extra = [s for s in names if s not in base][: n - len(base)]
    assert len(base) + len(extra) == n
    src = open(os.path.join(LIB, "h2o2.dat")).read()
    src = src.replace("ELEMENTS\nH O N\nEND", "ELEMENTS\nH O N C AR\nEND")
    src = src.replace("H2 O2 H2O H O OH HO2 H2O2 N2", " ".join(base + extra))
    d = tmp_path / f"lib{n}"
    d.mkdir()
    (d / "mech.dat").write_text(src)
    shutil.copy(TH, d / "therm.dat")
    return str(d)


@pytest.mark.parametrize("n,engine,kernel", [(12, "quad", "k_group<16, 16>"), (20, "pair", "k_group<32, 24>"),
                                             (30, "pair", "k_group<32, 32>")])
def test_group_engine_register_widths(pkg, orc, gpu, monkeypatch, tmp_path, n, engine, kernel):
    """The group engines' other instances (quad with a 16-wide register tile, pair with 24 / 32) on
    gas-only mechanisms of 12 / 20 / 30 species (H2/O2 plus inert species that only dilute and enter
    the third-body sums): end states at tight tolerances against the oracle to 1e-6 relative, ignition
    times within two ignition steps at default tolerances, and the same end states as the wavefront
    engine."""
    d = _h2o2_with_inerts(tmp_path, n)
    pm = pkg.Mechanism.from_files(d, gas_mech="mech.dat")
    om = orc.Mech(os.path.join(d, "mech.dat"), os.path.join(d, "therm.dat"), None, conv=orc.CONV_REFERENCE)
    assert pm.n == n
    monkeypatch.setenv("BRHIP_ENGINE", engine)
    eng = pkg.Engine(pm)
    assert eng.engine == engine and eng.kernel_name == kernel, eng.kernel_name
    N = 48
    rng = np.random.default_rng(n)
    T = rng.uniform(1000.0, 1300.0, N)
    X = np.zeros((N, pm.ng))
    X[:, pm.gas_species.index("H2")] = 0.3
    X[:, pm.gas_species.index("O2")] = 0.15
    X[:, pm.gas_species.index("N2")] = 0.3
    X[:, len("H2 O2 H2O H O OH HO2 H2O2 N2".split()):] = 0.25 / (n - 9)
    U0 = np.stack([pm.initial_state(T[i], 1e5, X[i]) for i in range(N)])
    Asv = np.ones(N)
    Ug, st = eng.integrate(T, Asv, U0, 1e-2, rtol=1e-10, atol=1e-16)
    assert np.all(st["status"] == 0)
    for i in range(N):
        uo, so, _ = om.integrate(T[i], 1.0, U0[i], 1e-2, analytic_jac=True, rtol=1e-10, atol=1e-16)
        assert so["status"] == 0
        assert close_states(Ug[i], uo, rtol=1e-6, floor=1e-14) <= 1.0, (n, i)
    U, st = eng.integrate(T, Asv, U0, 1e-2)
    for i in range(0, N, 6):
        uo, so, _ = om.integrate(T[i], 1.0, U0[i], 1e-2, analytic_jac=True)
        assert abs(st["t_ign"][i] - so["t_ign"]) <= 2 * max(st["ign_dt"][i], so["ign_dt"]) + 1e-4 * so["t_ign"], i
    monkeypatch.setenv("BRHIP_ENGINE", "wave")
    Uw, sw = eng.integrate(T, Asv, U0, 1e-2, rtol=1e-10, atol=1e-16)
    assert np.all(sw["status"] == 0)
    assert max(close_states(Ug[i], Uw[i], rtol=1e-6, floor=1e-14) for i in range(N)) <= 1.0


@pytest.mark.parametrize("which,engine,kernel", [("h2o2+3", "lane", "k_lane<12>"), ("gri47+ni", "wave", "k_integrate<64>")])
def test_remaining_integrator_instances(pkg, orc, gpu, monkeypatch, tmp_path, which, engine, kernel):
    """The two integrator instances no bench or golden mechanism reaches: k_lane<12> (H2/O2 plus three
    inert species, n = 12) and k_integrate<64> (GRI-Mech without six species + the Ni surface mechanism,
    n = 47 + 13 = 60, one component per lane with surface chemistry). Eight reactors each, the bars of
    test_integrate_parity_tight: rtol 1e-10 / atol 1e-16 on both sides, end states at tf = 1e-2 s to
    1e-6 relative (floor 1e-14)."""
    if which == "h2o2+3":
        d, surf, case = _h2o2_with_inerts(tmp_path, 12), None, "h2o2"
    else:
        from test_group_kernels import subset_mechanism
        gri = pkg.Mechanism.from_files(LIB, gas_mech="grimech.dat").gas_species
        species = [s for s in gri if s not in ("AR", "C3H7", "C3H8", "CH2CHO", "CH3CHO", "HCNO")]
        d, surf, case = subset_mechanism(tmp_path, species, surface="ch4ni.xml"), "ch4ni.xml", "gas_surf"
    pm = pkg.Mechanism.from_files(d, gas_mech="mech.dat", surface_mech=surf)
    om = orc.Mech(os.path.join(d, "mech.dat"), os.path.join(d, "therm.dat"), os.path.join(d, surf) if surf else None,
                  conv=orc.CONV_REFERENCE)
    assert pm.n == (12 if which == "h2o2+3" else 60)
    monkeypatch.setenv("BRHIP_ENGINE", engine)
    eng = pkg.Engine(pm)
    assert eng.engine == engine and eng.kernel_name == kernel, (eng.engine, eng.kernel_name)
    N, tf = 8, 1e-2
    T, Asv, U0 = _ignition_inputs(pm, case, N, 6)
    U, st = eng.integrate(T, Asv, U0, tf, rtol=1e-10, atol=1e-16)
    assert np.all(st["status"] == 0)
    Uo, so, bad = om.integrate_batch(T, Asv, U0, tf, rtol=1e-10, atol=1e-16, analytic_jac=True, nthreads=8)
    assert bad == 0 and all(s["status"] == 0 for s in so)
    for i in range(N):
        e = close_states(U[i], Uo[i], rtol=1e-6, floor=1e-14)
        assert e <= 1.0, (which, i, e)


def test_lane_engine_deferral(pkg, orc, gpu, monkeypatch):
    """Reactors still running after BRHIP_DEFER_STEPS steps in the lane engine are handed to the
    wavefront engine, which continues them from their last accepted lane state (a CVODE restart at
    that time; the lane's counters and ignition marker carry over). With the threshold at 30 steps
    most of the 300 reactors take that path; every end state must still match the oracle at tight
    tolerances, the step counts must be the full ones (lane + wave), and dense output rows written
    by either engine must match the oracle."""
    monkeypatch.setenv("BRHIP_ENGINE", "lane")
    monkeypatch.setenv("BRHIP_DEFER_STEPS", "30")
    pm, om = _mechs(pkg, orc, "h2o2")
    eng = pkg.Engine(pm)
    assert eng.engine == "lane"
    N = 300
    T, Asv, U0 = _ignition_inputs(pm, "h2o2", N, 11)
    tf = np.where(np.arange(N) % 2 == 0, 1e-6, 1e-2)          # short runs stay on the lanes
    tout = np.array([1e-7, 1e-5, 5e-3])
    U, st = eng.integrate(T, Asv, U0, tf, rtol=1e-10, atol=1e-16, tout=tout)
    assert np.all(st["status"] == 0)
    assert np.sum(st["nsteps"] > 30) > N // 3
    for i in range(N):
        sel = tout <= tf[i]
        uo, so, Yo = om.integrate_out(T[i], Asv[i], U0[i], tf[i], tout[sel], analytic_jac=True, rtol=1e-10, atol=1e-16)
        assert close_states(U[i], uo, rtol=1e-6, floor=1e-14) <= 1.0, i
        for j in range(int(sel.sum())):
            assert close_states(st["yout"][i, j], Yo[j], rtol=1e-6, floor=1e-14) <= 1.0, (i, j)
        if st["nsteps"][i] > 30:   # lane + wave steps; the restart re-ramps the order (a few tens of steps)
            assert 0.8 * so["nsteps"] <= st["nsteps"][i] <= 1.2 * so["nsteps"] + 40, (i, st["nsteps"][i], so["nsteps"])


def test_lane_deferral_step_budget(pkg, orc, gpu, monkeypatch):
    """The step limit holds for the whole run across the lane -> wavefront hand-over (SciML's
    maxiters counts every step of one solve): with max_steps = 60 and deferral after 30 lane steps,
    every reactor that needs more than 60 steps stops with BR_ERR_MAXSTEPS (-1) after exactly 60
    steps in total -- the oracle's CVODE run reports the same status at the same step count."""
    monkeypatch.setenv("BRHIP_ENGINE", "lane")
    monkeypatch.setenv("BRHIP_DEFER_STEPS", "30")
    pm, om = _mechs(pkg, orc, "h2o2")
    eng = pkg.Engine(pm)
    assert eng.engine == "lane"
    N = 64
    T, Asv, U0 = _ignition_inputs(pm, "h2o2", N, 12)
    U, st = eng.integrate(T, Asv, U0, 10.0, max_steps=60)
    for i in range(N):
        _, so, _ = om.integrate(T[i], Asv[i], U0[i], 10.0, analytic_jac=True, max_steps=60)
        assert so["status"] == -1 and so["nsteps"] == 60
        assert st["status"][i] == -1 and st["nsteps"][i] == 60, (i, st["status"][i], st["nsteps"][i])


@pytest.mark.parametrize("case,N", [("gri", 3000), ("surf", 5000)])
def test_persistent_grid_matches_static(pkg, gpu, monkeypatch, case, N):
    """k_integrate's persistent grid (waves take reactors from a work counter, reusing their LDS
    block and workspace slot) gives bit-identical end states and counters to the one-reactor-per-
    wave grid (BRHIP_STATIC=1): each reactor's arithmetic does not depend on which wave or slot
    ran it. N exceeds the resident wave count, so slots are reused many times."""
    gas = {"gri": "grimech.dat", "surf": None}[case]
    pm = pkg.Mechanism.from_files(LIB, gas_mech=gas, surface_mech="ch4ni.xml" if case == "surf" else None,
                                  gasphase=None if gas else "CH4 H2O H2 CO CO2 O2 N2".split())
    from batchreactor_amd import ensemble
    T, Asv, U0 = ensemble.make_inputs(pm, case, 0, N)
    eng = pkg.Engine(pm)
    monkeypatch.delenv("BRHIP_STATIC", raising=False)
    Ud, sd = eng.integrate(T, Asv, U0, 10.0)
    monkeypatch.setenv("BRHIP_STATIC", "1")
    Us, ss = eng.integrate(T, Asv, U0, 10.0)
    assert np.array_equal(Ud, Us)
    for k in ("nsteps", "nfe", "nje", "nsetups", "netf", "status"):
        assert np.array_equal(sd[k], ss[k]), k


@pytest.mark.parametrize("dq", [False, True], ids=["analytic", "dq"])
def test_failure_fraction_matches_cvode(pkg, orc, gpu, dq):
    """C5 gas+surface: a few reactors in 1e3 end with CVODE's CV_ERR_FAILURE (-3, seven consecutive
    error-test failures, in the order-5 phase before ignition). The oracle does the same on the same
    inputs (20000-reactor run: oracle 73, engine 84, 7 in common: which reactors fail is
    rounding-dependent, the rate is the algorithm's). Pinned here: the engine's failure count on the
    first 3000 reactors is within Poisson noise of the oracle's on the same reactors, and every
    failure is -3 (no other status) -- with the analytic Jacobian and with CVODE's DQ Jacobian (the
    reference's setting) on both sides."""
    from batchreactor_amd import ensemble
    pm, om = _mechs(pkg, orc, "gas_surf")
    N = 3000
    T, Asv, U0 = ensemble.make_inputs(pm, "gas_surf", 0, N)
    U, st = pkg.Engine(pm).integrate(T, Asv, U0, 10.0, dq_jacobian=dq)
    _, sto, _ = om.integrate_batch(T, Asv, U0, 10.0, analytic_jac=not dq, nthreads=16)
    so = np.array([s["status"] for s in sto])
    fg, fo = int(np.sum(st["status"] != 0)), int(np.sum(so != 0))
    assert set(np.unique(st["status"])) <= {0, -3} and set(np.unique(so)) <= {0, -3}
    assert abs(fg - fo) <= 3 * np.sqrt(fo + fg) + 3, (fg, fo)
    print(f"\n  gas_surf failures on {N} ({'DQ' if dq else 'analytic'} J): engine {fg}, oracle {fo}")


@pytest.mark.parametrize("ndev", [1, 3])
def test_integrate_multi_shards(pkg, gpu, ndev):
    """br_integrate_multi: the ensemble split over `ndev` handles (on the one GPU of the test box;
    one handle per GPU in production), integrated concurrently; states, counters and dense output
    are bit-identical to one br_integrate over the whole ensemble (each reactor's arithmetic does not
    depend on its shard), for an ensemble size not divisible by ndev."""
    from batchreactor_amd import ensemble
    pm = pkg.Mechanism.from_files(LIB, gas_mech="grimech.dat")
    T, Asv, U0 = ensemble.make_inputs(pm, "gri", 0, 301)
    tout = np.array([1e-4, 1e-3, 1.0])
    U1, s1 = pkg.Engine(pm).integrate(T, Asv, U0, 10.0, tout=tout)
    engines = [pkg.Engine(pm, device=0) for _ in range(ndev)]
    Um, sm = pkg.integrate_multi(engines, T, Asv, U0, 10.0, tout=tout)
    assert np.array_equal(U1, Um) and np.array_equal(s1["yout"], sm["yout"])
    for k in ("nsteps", "nfe", "nje", "status", "t_ign"):
        assert np.array_equal(s1[k], sm[k]), k


@pytest.mark.parametrize("scenario,flags,chem", [
    ("batch_h2o2", ["--gas"], dict(gaschem=True)),
    ("batch_surf", ["--surf"], dict(surfchem=True)),
    ("batch_gas_and_surf", ["--gas", "--surf"], dict(gaschem=True, surfchem=True))])
def test_native_cli_matches_python_host(pkg, gpu, tmp_path, scenario, flags, chem):
    """The file-driven batch_reactor through the C-ABI only (brhip_batch: br_read_batch_xml,
    br_mech_parse, br_mech_create, br_integrate_traced -- the Julia module's path, no Python in it)
    writes the same four files as the Python host, byte for byte."""
    import shutil
    import subprocess
    from conftest import GOLDEN, ROOT
    a, b = tmp_path / "native", tmp_path / "python"
    for d in (a, b):
        d.mkdir()
        shutil.copy(os.path.join(GOLDEN, scenario, "batch.xml"), d / "batch.xml")
    cli = os.path.join(ROOT, "batchreactor.jl_amd", "brhip_batch")
    r = subprocess.run([cli, str(a / "batch.xml"), LIB] + flags, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "Success", r.stderr
    assert pkg.batch_reactor(str(b / "batch.xml"), LIB, **chem) == "Success"
    for f in ("gas_profile.dat", "gas_profile.csv", "surface_covg.dat", "surface_covg.csv"):
        assert (a / f).read_text() == (b / f).read_text(), f


_SMALL_SURF = """<?xml version="1.0" encoding="ISO-8859-1"?>
<surface_chemisrty unit="kJ/mol" name="h2coni">
	<species>(ni) H(ni) O(ni) H2O(ni) OH(ni) CO(ni) </species>
	<site name="(ni)">
		<coordination>co(ni)=1.0</coordination>
		<density unit="mol/cm2">2.66e-09</density>
		<initial>h2o(ni)=0.4,(ni)=0.6 </initial>
	</site>
	<stick>
		<rxn id="1" >h2 + (ni) + (ni) => h(ni) + h(ni) 	@ 1.0000e-2 </rxn>
		<rxn id="2" >o2 + (ni) + (ni) => o(ni) + o(ni) 	@ 1.0000e-2 </rxn>
		<rxn id="4" >h2o + (ni) => h2o(ni)              	@ 1.0000e-1 </rxn>
		<rxn id="6" >co + (ni) => co(ni)                	@ 5.0000e-1 </rxn>
	</stick>
	<arrhenius>
		<rxn id="7"  >h(ni) + h(ni) => (ni) + (ni) + h2 	@ 2.545e+19	0.0	81.21	</rxn>
		<rxn id="8"  >o(ni) + o(ni) => (ni) + (ni) + o2 	@ 4.283e+23	0.0	474.95	</rxn>
		<rxn id="10" >h2o(ni)  => (ni) + h2o		@ 3.732e+12	0.0 	60.79	</rxn>
		<rxn id="12" >co(ni)  => (ni) + co 		@ 3.563e+11	0.0	111.27	</rxn>
		<rxn id="13" >o(ni) + h(ni) => oh(ni) + (ni)	@ 5.000e+22	0.0	97.90	</rxn>
		<rxn id="14" >oh(ni) + (ni) => o(ni) + h(ni)	@ 1.781e+21	0.0	36.09	</rxn>
		<rxn id="15" >oh(ni) + h(ni) => h2o(ni) + (ni)	@ 3.000e+20	0.0	42.70	</rxn>
		<rxn id="16" >h2o(ni) + (ni) => oh(ni) + h(ni)	@ 2.271e+21	0.0	91.76	</rxn>
		<rxn id="17" >oh(ni) + oh(ni) => o(ni) + h2o(ni)	@ 3.000e+21	0.0	100.00	</rxn>
		<rxn id="18" >o(ni) + h2o(ni) => oh(ni) + oh(ni)	@ 6.373e+23	0.0	210.86	</rxn>
	</arrhenius>
	<coverage id="12">co(ni)=-50</coverage>
</surface_chemisrty>
"""
SMALL_SURF_GAS = ["H2", "O2", "H2O", "CO", "N2"]


def _small_surface_mech(pkg, orc, tmp_path):
    """A surface mechanism small enough for the quad engine (n = 5 gas + 6 surface = 11 <= 16): the
    H2/O2/H2O/CO subset of the reference's ch4ni.xml (tests/golden/lib; same rate constants,
    sticking reactions, the coverage-dependent CO desorption), written to a scratch library."""
    import shutil
    d = tmp_path / "smallsurf"
    d.mkdir()
    (d / "h2coni.xml").write_text(_SMALL_SURF)
    shutil.copy(TH, d / "therm.dat")
    pm = pkg.Mechanism.from_files(str(d), surface_mech="h2coni.xml", gasphase=SMALL_SURF_GAS)
    om = orc.Mech(None, str(d / "therm.dat"), str(d / "h2coni.xml"), gas_species=SMALL_SURF_GAS,
                  conv=orc.CONV_REFERENCE)
    return pm, om


def test_quad_engine_surface_chemistry(pkg, orc, gpu, monkeypatch, tmp_path):
    """The quad engine (k_group<16, NM>, the default for mechanisms with n <= 16) on SURFACE chemistry:
    sticking coefficients, coverage-dependent activation, the Asv assembly of src/BatchReactor.jl:345,
    on a reduced Ni mechanism with n = 11. Default engine selection picks it; against the oracle at
    tight tolerances (end states to 1e-6 relative, analytic and DQ Jacobians), at default tolerances
    (2x the oracle's own u0-perturbation spread at the 28 output times, tests/parity_bands.py; step
    counts to 35 % / 3 %), and the
    same end states as the wavefront engine."""
    pm, om = _small_surface_mech(pkg, orc, tmp_path)
    assert pm.n == 11 and pm.ns == 6
    monkeypatch.delenv("BRHIP_ENGINE", raising=False)
    eng = pkg.Engine(pm)
    assert eng.engine == "quad" and eng.kernel_name.startswith("k_group<16,"), (eng.engine, eng.kernel_name)
    N = 96
    rng = np.random.default_rng(17)
    T = rng.uniform(800.0, 1100.0, N)
    X = np.zeros((N, pm.ng))
    X[:, 0] = rng.uniform(0.05, 0.3, N)          # H2
    X[:, 1] = rng.uniform(0.05, 0.2, N)          # O2
    X[:, 2] = rng.uniform(0.0, 0.1, N)           # H2O
    X[:, 3] = rng.uniform(0.0, 0.05, N)          # CO
    X[:, 4] = 1.0 - X[:, :4].sum(1)              # N2
    U0 = np.stack([pm.initial_state(T[i], 1e5, X[i]) for i in range(N)])     # theta0 from <initial>
    Asv = np.exp(rng.uniform(0, np.log(100), N))
    for dq in (False, True):
        U, st = eng.integrate(T, Asv, U0, 1e-2, rtol=1e-10, atol=1e-16, dq_jacobian=dq)
        assert np.all(st["status"] == 0), (dq, np.unique(st["status"]))
        if dq:
            assert np.all(st["nfe_dq"] == st["nje"] * pm.n)
        for i in range(N):
            uo, so, _ = om.integrate(T[i], Asv[i], U0[i], 1e-2, analytic_jac=not dq, rtol=1e-10, atol=1e-16)
            assert so["status"] == 0
            assert close_states(U[i], uo, rtol=1e-6, floor=1e-14) <= 1.0, (dq, i)
    U, st = eng.integrate(T, Asv, U0, 10.0, tout=OUT_T)
    assert np.all(st["status"] == 0)
    bounds = BOUNDS[("small_surf", False)]
    nst_o = 0
    for i in range(N):
        uo, so, Yo = om.integrate_out(T[i], Asv[i], U0[i], 10.0, OUT_T, analytic_jac=True)
        assert so["status"] == 0
        eb = _band_errors(st["yout"][i], Yo, float("nan"))
        assert eb[0] <= bounds[0], (i, eb)
        assert abs(st["nsteps"][i] - so["nsteps"]) <= 0.35 * so["nsteps"], (i, st["nsteps"][i], so["nsteps"])
        nst_o += so["nsteps"]
    assert abs(st["nsteps"].sum() / nst_o - 1) <= 0.03, (st["nsteps"].sum(), nst_o)
    Uq, _ = eng.integrate(T, Asv, U0, 1e-2, rtol=1e-10, atol=1e-16)
    monkeypatch.setenv("BRHIP_ENGINE", "wave")
    assert eng.engine == "wave"
    Uw, sw = eng.integrate(T, Asv, U0, 1e-2, rtol=1e-10, atol=1e-16)
    assert np.all(sw["status"] == 0)
    assert max(close_states(Uq[i], Uw[i], rtol=1e-6, floor=1e-14) for i in range(N)) <= 1.0


# The bench-sample reactors whose GPU deviation exceeded the round-5 bounds (profiles/
# r06_parity_outliers.json, scripts/parity_outliers.py): (config, Jacobian kind, reactor index of the
# bench workload, bench.PARITY_SAMPLE).
BENCH_OUTLIERS = [("gri", True, 1407), ("gri", True, 1621), ("gri", True, 99), ("gas_surf", False, 678),
                  ("gas_surf", True, 678), ("h2o2", True, 1285), ("h2o2", True, 1589)]


@pytest.mark.parametrize("case,dq,idx", BENCH_OUTLIERS,
                         ids=[f"{c}-{'dq' if d else 'an'}-{i}" for c, d, i in BENCH_OUTLIERS])
def test_bench_outlier_reactors(pkg, orc, gpu, case, dq, idx):
    """Regression test for the round-5 bench outliers: on exactly those reactors
    of the bench workload, (a) the GPU's windows at the default tolerances lie inside the re-derived
    per-case bounds (tests/parity_bands.py: 2x the oracle's own rounding spread on the bench sample),
    and (b) converged runs (rtol 1e-10 / atol 1e-16, same Jacobian kind on both sides) end at states
    that agree to 1e-6 relative -- the deviation at 1e-6 is CVODE's rounding chaos, not a different
    trajectory (src/BatchReactor.jl:204-210)."""
    from batchreactor_amd import ensemble
    pm, om = _mechs(pkg, orc, case)
    eng = pkg.Engine(pm)
    T, Asv, U0 = ensemble.make_inputs(pm, case, idx, 1)
    tf = 10.0
    _, stg = eng.integrate(T, Asv, U0, tf, tout=OUT_T, dq_jacobian=dq)
    _, sto, bad, Yo = om.integrate_batch(T, Asv, U0, tf, analytic_jac=not dq, nthreads=1, tout=OUT_T)
    assert bad == 0 and stg["status"][0] == 0
    w = _band_errors(stg["yout"][0], Yo[0], sto[0]["t_ign"])
    assert np.all(np.array(w) <= np.array(BOUNDS[(case, dq)][:3])), (case, dq, idx, w)
    U, st = eng.integrate(T, Asv, U0, tf, rtol=1e-10, atol=1e-16, dq_jacobian=dq)
    Uo, so, bad = om.integrate_batch(T, Asv, U0, tf, rtol=1e-10, atol=1e-16, analytic_jac=not dq, nthreads=1)
    assert bad == 0 and st["status"][0] == 0
    assert close_states(U[0], Uo[0], rtol=1e-6, floor=1e-14) <= 1.0
