"""The wavefront engine keeps a lane's own {kf, kr} pairs and its molar mass in registers between linear-solver
setups (KReg, csrc/brhip_device.hpp). The registers are a third copy of values whose first two homes are
init_tconst's stores and the wave's global slot, so what can go wrong is their lifetime: a wave that takes its next
reactor, a setup (analytic Jacobian, DQ columns, LU) that clobbers them, rate multipliers that change them, and
the temperature refreshes of the programme and energy instances. Every test here runs GRI-Mech 3.0 on
k_integrate<56>.

Inputs of the reuse tests: CH4/O2/N2 = .1/.2/.7 at 1e5 Pa, T distinct in [1200, 1201) K, tf = 6.25e-3 s. Found with
the CPU oracle (integrate_batch, both Jacobians, 4611 reactors, tf on a grid of 0.25e-3 s): a second Jacobian
needs more than 50 steps (LS_MSBJ), which this mixture takes only shortly before it ignites near 7e-3 s. 5.75e-3 s
leaves reactors at nje = 1; 6e-3 s is the oracle's shortest tf with nje = 2 everywhere, but at 58 to 60 steps, and
the GPU's DQ run, whose rounding differs, left a reactor at nje = 1 there; at 6.25e-3 s every reactor has nje = 2
after 67 to 70 steps and at least 97 % of its CH4 left. A wider T range does not work: at [1200, 1205) K the hot
end is down to 91 % CH4 at the same tf."""
import numpy as np
import pytest

from conftest import LIB
from parity_bands import BOUNDS, band_errors

pytestmark = pytest.mark.gpu

COUNTERS = ("nsteps", "nfe", "nje", "nsetups", "nni", "ncfn", "netf", "status", "nfe_dq")
TIMES = ("t_end", "t_ign", "ign_dt", "ign_rate")
TF = 6.25e-3


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.fixture(scope="module")
def gri(pkg, gpu):
    pm = pkg.Mechanism.from_files(LIB, gas_mech="grimech.dat")
    eng = pkg.Engine(pm)
    assert eng.kernel_name == "k_integrate<56>", eng.kernel_name
    yield pm, eng
    eng.close()


@pytest.fixture(scope="module")
def ensemble(gri):
    """(slots, T, Asv, U0, tf): more reactors than the persistent grid has waves, and not a multiple of anything"""
    import torch
    pm, eng = gri
    slots = eng.launch_info["waves_per_cu"] * torch.cuda.get_device_properties(0).multi_processor_count
    N = slots + slots // 8 + 3
    T = 1200.0 + np.arange(N) / N
    x = pm.mole_fractions({"CH4": 0.1, "O2": 0.2, "N2": 0.7})
    U0 = np.array([pm.initial_state(t, 1e5, x) for t in T])
    return slots, T, np.ones(N), U0, np.full(N, TF)


def _mult(eng, N):
    """three rows of multipliers (none, every third reaction x 1.5, every fifth off and every seventh halved),
    dealt round robin: neighbouring reactors, and a wave's successive reactors, differ in their {kf, kr}"""
    m = np.ones((3, eng.nr))
    m[1, ::3] = 1.5
    m[2, ::5] = 0.0
    m[2, 1::7] = 0.5
    return m, (np.arange(N) % 3).astype(np.int32)


@pytest.mark.parametrize("dq", [False, True], ids=["analytic", "dq"])
@pytest.mark.parametrize("mult", [False, True], ids=["plain", "rate_mult"])
def test_slot_reuse_and_setup_paths(gri, ensemble, dq, mult):
    """One launch over more reactors than resident waves (some waves take a second reactor from the work counter)
    against the same reactors in launches of a quarter of the grid (every reactor is its wave's first): states and
    every counter bit-equal. nje >= 2 everywhere, so each reactor ran at least one setup after the first and the
    reload behind it; with dq the DQ column loop sits between that reload's predecessor and the next RHS; with
    rate_mult the pairs differ from reactor to reactor at (nearly) the same T."""
    pm, eng = gri
    slots, T, Asv, U0, tf = ensemble
    N = len(T)
    kw = dict(dq_jacobian=dq)
    rows = None
    if mult:
        kw["rate_mult"], rows = _mult(eng, N)
    U, st = eng.integrate(T, Asv, U0, tf, rate_mult_row=rows, **kw)
    # (rows 1 and 2 of the multipliers are other mixtures in effect: the oracle has row 1 at nje 4..5 with 68 % of its
    # CH4 left, row 2 at 36..41 steps; the conditions the inputs were chosen for hold on the unscaled reactors)
    plain = np.ones(N, bool) if rows is None else rows == 0
    assert np.all(st["status"] == 0) and st["nje"][plain].min() >= 2, (st["status"].max(), st["nje"][plain].min())
    assert st["nje"].min() >= 1 and st["nsteps"].min() > 20
    k = pm.gas_species.index("CH4")
    assert (U[plain, k] / U0[plain, k]).min() > 0.9              # nobody ignited
    if dq:
        assert np.all(st["nfe_dq"] == st["nje"] * pm.n)
    chunk = slots // 4
    for a in range(0, N, chunk):
        s = slice(a, min(a + chunk, N))
        Uc, sc = eng.integrate(T[s], Asv[s], U0[s], tf[s], rate_mult_row=None if rows is None else rows[s], **kw)
        assert _same(Uc, U[s]), (dq, mult, a, int(np.sum(np.any(Uc != U[s], axis=1))))
        for c in COUNTERS + TIMES:
            assert _same(sc[c], st[c][s]), (dq, mult, a, c)
    if mult:                                                     # (the multipliers do change the run)
        U1, _ = eng.integrate(T[:6], Asv[:6], U0[:6], tf[:6], dq_jacobian=dq)
        assert _same(U1[0::3], U[0:6:3]) and not _same(U1[1], U[1]) and not _same(U1[2], U[2])


def test_programme_instance_against_the_host_restatement(pkg, orc, gri):
    """k_integrate<56, true> refreshes the T-only constants inside the step loop; the registers are loaded again
    after every refresh. Eight reactors, each with its own ramp (T0 = 950 + 5 i K, up 100 K in 0.5 ms, held to
    1 ms), against the host CVODE restatement f(t, u) = oracle.rhs(T(t), 1, u) at tf, with the bound and the
    step-count band of test_tprog_gpu's trajectory test (the pre-ignition band of GRI's DQ runs, 35 %)."""
    import test_tprog_gpu as tp
    pm, eng = gri
    om = tp._oracle(orc, "gri")
    x = pm.mole_fractions({"CH4": 0.1, "O2": 0.2, "N2": 0.7})
    N, tf = 8, 1e-3
    T0 = 950.0 + 5.0 * np.arange(N)
    U0 = np.array([pm.initial_state(t, 1e5, x) for t in T0])
    kt = np.tile([0.0, 5e-4, 1e-3], (N, 1))
    kT = np.stack([T0, T0 + 100.0, T0 + 100.0], axis=1)
    U, st = eng.integrate(None, np.ones(N), U0, np.full(N, tf), dq_jacobian=True, tprog=(kt, kT))
    assert np.all(st["status"] == 0) and np.all(st["nfe_dq"] == st["nje"] * pm.n)
    bound = BOUNDS[("gri", True)][0]
    for i in range(N):
        prog = pkg.TemperatureProgram.from_knots(kt[i], kT[i])
        status, uh, sh = pkg._lib.integrate_host(lambda t, u: om.rhs(prog(t), 1.0, u)[0], U0[i], tf)
        assert status == 0
        e = band_errors(U[i:i + 1], uh[None, :], np.nan, np.array([tf]))[0]
        print(f"\n  reactor {i}: {e:.3g} bands at tf (bound {bound}), steps {int(st['nsteps'][i])} vs {int(sh[0])}")
        assert e <= bound, (i, e, bound)
        assert abs(st["nsteps"][i] - sh[0]) <= 0.35 * sh[0], (i, st["nsteps"][i], sh[0])


def test_energy_instance_against_the_cpu_statement(pkg, orc, gpu):
    """k_integrate<56, false, true> (adiabatic, T a state component) refreshes the constants before any RHS whose T
    moved, twice per DQ Jacobian for the T column alone; it loads every pair from the slot (KReg<0>). Eight copies
    of energy_cases' GRI regime in one launch: each against the CPU statement at tf with test_energy_gpu's bounds
    (2 x the CPU statement's own spread per ignition window, floor 1e-6; t_ign; 35 % on the steps), and all eight
    bit-equal to each other (eight waves, eight slots, one answer)."""
    import energy_cases as ec
    pm, om, y0, tf = ec.mechs(pkg, orc, "gri", 0)
    base = ec.host_run(pkg, orc, "gri", 0)
    spread, dt_spread = ec.host_spread(pkg, orc, "gri", 0)
    bound = np.maximum(2.0 * spread, 1e-6)
    N = 8
    eng = pkg.Engine(pm)
    assert eng.energy_kernel_name == "k_integrate<56, false, true>", eng.energy_kernel_name
    U, st = eng.integrate(np.full(N, y0[-1]), np.ones(N), np.tile(y0[:-1], (N, 1)), np.full(N, tf), energy="adiabatic")
    eng.close()
    assert np.all(st["status"] == 0) and np.all(st["nfe_dq"] == st["nje"] * (pm.ng + 1)) and st["nje"].min() > 0
    for i in range(1, N):
        assert _same(U[i], U[0]) and _same(st["T_end"][i], st["T_end"][0]), i
        for c in COUNTERS + TIMES:
            assert _same(st[c][i], st[c][0]), (i, c)
    e = ec.window_errors(np.append(U[0], st["T_end"][0]), base["y"], base["t_ign"], [tf])
    d_ign = abs(st["t_ign"][0] - base["t_ign"])
    b_ign = max(st["ign_dt"][0], base["ign_dt"], 2.0 * dt_spread)
    print(f"\n  bands at tf {e}, bound {bound}; t_ign {st['t_ign'][0]:.6g} vs {base['t_ign']:.6g} (bound {b_ign:.3g}); "
          f"steps {int(st['nsteps'][0])} vs {int(base['stats'][0])}")
    assert np.all(e <= bound), (e, bound)
    assert d_ign <= b_ign, (d_ign, b_ign)
    assert abs(st["nsteps"][0] - base["stats"][0]) <= 0.35 * base["stats"][0]
