"""Per-reactor rate multipliers (br_opts.rate_mult / rate_mult_row) in every engine, and br_sensitivity.

A multiplier scales the T-only constants of a reaction (gas: kf before kr = kf / Kc, a falloff's k0 / k_inf
untouched; surface: k), so most of what is checked here is checked bit for bit: a table of ones changes
nothing, a multiplier of 2 is a doubled A factor (a power of two scales exactly), all rates times 2 is time
over 2, and a shared-row table is its dense expansion. The oracle's set_rxn_mult(r, m, m) gives the
independent check for generic multipliers and for the sensitivities.

Sizes: 37 reactors on the quad engine (16 per workgroup, 4 per wave), 70 on the lane engine, 9 / 5 / 3 on
k_integrate<32 | 56 | 72>, 5 on the pair engine -- partial groups and more than one workgroup everywhere.
"""
import copy
import os

import numpy as np
import pytest

from conftest import LIB
from test_gpu_parity import close_states
from test_group_kernels import S24, ignition_mixtures, subset_mechanism

pytestmark = pytest.mark.gpu

COUNTERS = ("nsteps", "nfe", "nje", "nsetups", "nni", "ncfn", "netf", "status", "nfe_dq")
TIMES = ("t_end", "t_ign", "ign_dt")                  # scale with 1 / m when every rate is scaled by m
# which -> (BRHIP_ENGINE or None = the mechanism's default, case, N, kernel, tf)
ENGINES = {"quad": (None, "h2o2", 37, "k_group<16, 9>", 2e-3), "lane": ("lane", "h2o2", 70, "k_lane<9>", 2e-3),
           "wave32": ("wave", "surf", 9, "k_integrate<32>", 1.0), "wave56": ("wave", "gri", 5, "k_integrate<56>", 1e-2),
           "wave72": ("wave", "gas_surf", 3, "k_integrate<72>", 1e-2), "pair": ("pair", "s24", 5, "k_group<32, 24>", 1e-2)}
FILES = {"h2o2": dict(gas_mech="h2o2.dat"), "gri": dict(gas_mech="grimech.dat"),
         "surf": dict(surface_mech="ch4ni.xml", gasphase=["CH4", "H2O", "H2", "CO", "CO2", "O2", "N2"]),
         "gas_surf": dict(gas_mech="grimech.dat", surface_mech="ch4ni.xml")}


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _case(pkg, monkeypatch, tmp_path, which):
    """(mechanism, T, Asv, U0, tf, N) of an ENGINES entry, with BRHIP_ENGINE set for it"""
    from batchreactor_amd import ensemble
    env, case, N, _, tf = ENGINES[which]
    if env is None:
        monkeypatch.delenv("BRHIP_ENGINE", raising=False)
    else:
        monkeypatch.setenv("BRHIP_ENGINE", env)
    if case == "s24":                                   # a generated GRI subset with falloff reactions
        pm = pkg.Mechanism.from_files(subset_mechanism(tmp_path, S24), gas_mech="mech.dat")
        T, Asv, U0 = ignition_mixtures(pm, N, 5)
    else:
        pm = pkg.Mechanism.from_files(LIB, **FILES[case])
        T, Asv, U0 = ensemble.make_inputs(pm, case, 0, N)
    return pm, T, Asv, U0, np.full(N, tf), N


def _engine(pkg, pm, which):
    eng = pkg.Engine(pm)
    assert eng.kernel_name == ENGINES[which][3], eng.kernel_name
    return eng


def _assert_rows_equal(U, st, Ur, sr, rows, what, fields=COUNTERS + TIMES + ("ign_rate",)):
    assert _same(U[rows], Ur[rows]), (what, "u")
    for k in fields:
        assert _same(st[k][rows], sr[k][rows]), (what, k)


# --------------------------------------------------------------------------------- 1. ones == none
@pytest.mark.parametrize("which", list(ENGINES))
def test_all_ones_equals_no_multipliers(pkg, gpu, monkeypatch, tmp_path, which):
    """A table of 1.0 gives the states and every counter of a run without multipliers, bit for bit, with
    the analytic and the DQ Jacobian."""
    pm, T, Asv, U0, tf, N = _case(pkg, monkeypatch, tmp_path, which)
    eng = _engine(pkg, pm, which)
    ones = np.ones((N, eng.nr))
    for dq in (False, True):
        U, st = eng.integrate(T, Asv, U0, tf, dq_jacobian=dq)
        assert np.all(st["nsteps"] > 0)
        Um, sm = eng.integrate(T, Asv, U0, tf, dq_jacobian=dq, rate_mult=ones)
        _assert_rows_equal(Um, sm, U, st, np.arange(N), (which, dq))
        Um, sm = eng.integrate(T, Asv, U0, tf, dq_jacobian=dq, rate_mult=ones[:1], rate_mult_row=np.zeros(N, np.int32))
        _assert_rows_equal(Um, sm, U, st, np.arange(N), (which, dq, "shared row"))


# --------------------------------------------------------------------------------- 2. m = 2 is a doubled A
def _chosen_reactions(pm):
    """first and last member of every kind -- falloff, +M, elementary irreversible, elementary reversible;
    sticking, Arrhenius surface -- and the first and last index of the gas and of the surface block"""
    t, nrg, nrs = pm.tables, pm.nrg, pm.nrs
    kinds = []
    if nrg:
        tb, rev = np.asarray(t["g_tb"]), np.asarray(t["g_rev"])
        kinds += [np.flatnonzero(tb == 2), np.flatnonzero(tb == 1), np.flatnonzero((tb == 0) & (rev == 0)),
                  np.flatnonzero((tb == 0) & (rev != 0)), np.array([0, nrg - 1])]
    if nrs:
        stick = np.asarray(t["s_stick"])
        kinds += [nrg + np.flatnonzero(stick != 0), nrg + np.flatnonzero(stick == 0), np.array([nrg, nrg + nrs - 1])]
    out = []
    for k in kinds:
        for r in ([int(k[0]), int(k[-1])] if len(k) else []):
            if r not in out:
                out.append(r)
    return out


def _doubled_A(pm, r):
    """a copy of the mechanism whose reaction r has twice the A factor (and low-pressure A, for a falloff)"""
    p2 = copy.deepcopy(pm)
    if r < pm.nrg:
        p2.tables["g_arr"][r, 0] *= 2.0
        if p2.tables["g_tb"][r] == 2:
            p2.tables["g_low"][r, 0] *= 2.0
    else:
        p2.tables["s_arr"][r - pm.nrg, 0] *= 2.0
    return p2


@pytest.mark.parametrize("which", list(ENGINES))
def test_one_doubled_reaction_equals_doubled_A(pkg, gpu, monkeypatch, tmp_path, which):
    """m_r = 2 on the odd reactors, 1 on the even ones: the odd reactors must equal, bit for bit, a plain
    run of a copy of the mechanism whose A_r is doubled in the description, the even ones a plain run of
    the mechanism itself. g_par[0] / s_par[0] hold A itself and 2 scales exactly, so any difference is a
    defect -- a multiplier that reached another reaction (the packed order), one direction only, or the
    falloff ratio."""
    pm, T, Asv, U0, tf, N = _case(pkg, monkeypatch, tmp_path, which)
    eng = _engine(pkg, pm, which)
    chosen = _chosen_reactions(pm)
    tb = np.asarray(pm.tables["g_tb"]) if pm.nrg else np.zeros(0)
    if which in ("wave56", "wave72", "pair"):
        assert (tb == 2).any() and (tb == 1).any()
    if pm.nrs:
        assert np.asarray(pm.tables["s_stick"]).any() and not np.asarray(pm.tables["s_stick"]).all()
    U1, s1 = eng.integrate(T, Asv, U0, tf)
    odd, even = np.arange(1, N, 2), np.arange(0, N, 2)
    changed = 0
    for r in chosen:
        mult = np.ones((N, eng.nr))
        mult[odd, r] = 2.0
        Um, sm = eng.integrate(T, Asv, U0, tf, rate_mult=mult)
        e2 = _engine(pkg, _doubled_A(pm, r), which)
        U2, s2 = e2.integrate(T, Asv, U0, tf)
        e2.close()
        _assert_rows_equal(Um, sm, U2, s2, odd, (which, r, "doubled"))
        _assert_rows_equal(Um, sm, U1, s1, even, (which, r, "plain"))
        changed += int(not _same(U2[odd], U1[odd]))
    assert changed >= len(chosen) // 2, (which, changed, chosen)     # (the doubled runs do differ from the plain one)


# --------------------------------------------------------------------------------- 3. time-scaling identity
@pytest.mark.parametrize("which", list(ENGINES))
def test_time_scaling_identity(pkg, gpu, monkeypatch, tmp_path, which):
    """Every multiplier = 2 and tf / 2: the end states and step counters of the plain run, bit for bit,
    and t_ign (t_end, ign_dt) exactly half, ign_rate exactly twice -- every quantity of the controller
    scales by a power of two. With the surface mechanisms this is the surface multipliers' integration
    check (the oracle has no surface hook). Both Jacobians."""
    pm, T, Asv, U0, tf, N = _case(pkg, monkeypatch, tmp_path, which)
    eng = _engine(pkg, pm, which)
    two = np.full((1, eng.nr), 2.0)
    rows = np.zeros(N, np.int32)
    for dq in (False, True):
        U, st = eng.integrate(T, Asv, U0, tf, dq_jacobian=dq)
        Um, sm = eng.integrate(T, Asv, U0, tf / 2, dq_jacobian=dq, rate_mult=two, rate_mult_row=rows)
        for k in COUNTERS:
            assert _same(sm[k], st[k]), (which, dq, k)
        assert _same(Um, U), (which, dq)
        for k in TIMES:
            assert _same(sm[k], st[k] / 2), (which, dq, k)
        assert _same(sm["ign_rate"], st["ign_rate"] * 2), (which, dq)


# --------------------------------------------------------------------------------- 4. oracle parity
def _generic_table(N, nr, nzero=2):
    """every reaction of every reactor its own multiplier in [0.5, 2] (splitmix64), nzero of them 0"""
    from batchreactor_amd.ensemble import splitmix64_uniform
    m = 0.5 + 1.5 * splitmix64_uniform(np.arange(N * nr) + 1000).reshape(N, nr)
    for i in range(N):
        for z in range(nzero):
            m[i, (5 * i + 7 * z + 3) % nr] = 0.0
    return m


@pytest.mark.parametrize("case,N", [("h2o2", 8), ("gri", 4)])
def test_generic_multipliers_against_the_oracle(pkg, orc, gpu, monkeypatch, case, N):
    """Every gas reaction of every reactor with its own multiplier in [0.5, 2], two of them 0: the end
    states at rtol 1e-10 / atol 1e-16 agree with the oracle's (set_rxn_mult(r, m, m)) to 1e-6, the
    project's criterion for converged runs."""
    from batchreactor_amd import ensemble
    monkeypatch.delenv("BRHIP_ENGINE", raising=False)
    pm = pkg.Mechanism.from_files(LIB, **FILES[case])
    om = orc.Mech(os.path.join(LIB, FILES[case]["gas_mech"]), os.path.join(LIB, "therm.dat"))
    assert om.nrg == pm.nrg
    eng = pkg.Engine(pm)
    T, Asv, U0 = ensemble.make_inputs(pm, case, 0, N)
    tf = 1e-2
    mult = _generic_table(N, pm.nrg)
    assert mult.min() == 0.0 and mult[mult > 0].min() >= 0.5 and mult.max() <= 2.0
    U, st = eng.integrate(T, Asv, U0, tf, rtol=1e-10, atol=1e-16, rate_mult=mult)
    assert np.all(st["status"] == 0)
    Up, _ = eng.integrate(T, Asv, U0, tf, rtol=1e-10, atol=1e-16)
    for i in range(N):
        for r in range(pm.nrg):
            om.set_rxn_mult(r, mult[i, r], mult[i, r])
        uo, so, _ = om.integrate(T[i], Asv[i], U0[i], tf, rtol=1e-10, atol=1e-16, analytic_jac=True)
        assert so["status"] == 0
        err = close_states(U[i], uo, rtol=1e-6, floor=1e-14)
        print(f"{case} reactor {i}: err / bound = {err:.3g}, plain run differs by {close_states(Up[i], uo, 1e-6, 1e-14):.3g}")
        assert err <= 1.0, (case, i, err)
        assert close_states(Up[i], uo, rtol=1e-6, floor=1e-14) > 1.0, (case, i)   # (the multipliers matter)
    for r in range(pm.nrg):
        om.set_rxn_mult(r, 1.0, 1.0)


# --------------------------------------------------------------------------------- 5. rows and slices
def _shared_table(nr, K=3):
    from batchreactor_amd.ensemble import splitmix64_uniform
    return 0.5 + 1.5 * splitmix64_uniform(np.arange(K * nr) + 5000).reshape(K, nr)


@pytest.mark.parametrize("which", ["quad", "wave56"])
def test_row_indirection_equals_the_dense_table(pkg, gpu, monkeypatch, tmp_path, which):
    """A 3-row table with rate_mult_row = (i * 7) % 3 equals its dense expansion bit for bit: through
    br_integrate, through br_integrate_multi with two handles (the row indices, and the rows of the dense
    table, sliced with the ensemble) and through both passes of br_integrate_phase."""
    pm, T, Asv, U0, tf, N = _case(pkg, monkeypatch, tmp_path, which)
    eng = _engine(pkg, pm, which)
    tab = _shared_table(eng.nr)
    rows = ((np.arange(N) * 7) % 3).astype(np.int32)
    dense = tab[rows]
    Ud, sd = eng.integrate(T, Asv, U0, tf, rate_mult=dense)
    Ur, sr = eng.integrate(T, Asv, U0, tf, rate_mult=tab, rate_mult_row=rows)
    _assert_rows_equal(Ur, sr, Ud, sd, np.arange(N), (which, "rows"))
    U1, _ = eng.integrate(T, Asv, U0, tf)
    assert not _same(U1, Ud)
    e2 = pkg.Engine(pm)
    for kw in (dict(rate_mult=dense), dict(rate_mult=tab, rate_mult_row=rows)):
        Um, sm = pkg.integrate_multi([eng, e2], T, Asv, U0, tf, **kw)
        _assert_rows_equal(Um, sm, Ud, sd, np.arange(N), (which, "multi", sorted(kw)))
    e2.close()
    tau = np.array([0.5, 1.0, 1.5])
    Upd, spd = eng.integrate_phase(T, Asv, U0, tf, tau, rate_mult=dense)
    Upr, spr = eng.integrate_phase(T, Asv, U0, tf, tau, rate_mult=tab, rate_mult_row=rows)
    _assert_rows_equal(Upd, spd, Ud, sd, np.arange(N), (which, "phase = integrate"))
    _assert_rows_equal(Upr, spr, Upd, spd, np.arange(N), (which, "phase rows"))
    assert _same(spd["tout"], spr["tout"]) and _same(spd["yout"], spr["yout"])
    assert _same(spd["tout"], pkg.phase_grid(sd["t_ign"], tau, tf))       # pass 1 ran with the multipliers too
    assert np.isfinite(spd["tout"]).any()


def test_lane_hand_over_takes_the_row_by_reactor_id(pkg, gpu, monkeypatch, tmp_path):
    """The forced lane engine with BRHIP_DEFER_STEPS = 20: every reactor that runs longer is handed to the
    wavefront engine through rid_list, where its list position is not its index. Odd reactors with m_r = 2
    must still equal the doubled-A mechanism's run under the same hand-over, even ones the plain run, and
    the shared-row form its dense expansion -- all bit for bit."""
    pm, T, Asv, U0, tf, N = _case(pkg, monkeypatch, tmp_path, "lane")
    monkeypatch.setenv("BRHIP_DEFER_STEPS", "20")
    eng = _engine(pkg, pm, "lane")
    r = int(np.flatnonzero(np.asarray(pm.tables["g_tb"]) == 0)[0])
    odd, even = np.arange(1, N, 2), np.arange(0, N, 2)
    mult = np.ones((N, eng.nr))
    mult[odd, r] = 2.0
    U1, s1 = eng.integrate(T, Asv, U0, tf)
    assert (s1["nsteps"] > 20).sum() >= 8 and np.all(s1["status"] == 0)     # handed over, and finished there
    Um, sm = eng.integrate(T, Asv, U0, tf, rate_mult=mult)
    e2 = _engine(pkg, _doubled_A(pm, r), "lane")
    U2, s2 = e2.integrate(T, Asv, U0, tf)
    e2.close()
    assert not _same(U2, U1)
    _assert_rows_equal(Um, sm, U2, s2, odd, "doubled")
    _assert_rows_equal(Um, sm, U1, s1, even, "plain")
    rows = (np.arange(N) % 2).astype(np.int32)
    Ur, sr = eng.integrate(T, Asv, U0, tf, rate_mult=np.stack([mult[0], mult[1]]), rate_mult_row=rows)
    _assert_rows_equal(Ur, sr, Um, sm, np.arange(N), "rows")


# --------------------------------------------------------------------------------- 6. input checks
def test_bad_multipliers_are_refused_with_their_index(pkg, gpu, monkeypatch, tmp_path):
    pm, T, Asv, U0, tf, N = _case(pkg, monkeypatch, tmp_path, "quad")
    eng = _engine(pkg, pm, "quad")
    for bad, where in ((-0.5, (4, 3)), (np.nan, (0, 17)), (np.inf, (36, 0))):
        mult = np.ones((N, eng.nr))
        mult[where] = bad
        with pytest.raises(RuntimeError, match=rf"-10: rate_mult\[{where[0]}\]\[{where[1]}\]"):
            eng.integrate(T, Asv, U0, tf, rate_mult=mult)
    rows = np.zeros(N, np.int32)
    rows[5] = 2
    with pytest.raises(RuntimeError, match=r"-10: rate_mult_row\[5\] = 2"):
        eng.integrate(T, Asv, U0, tf, rate_mult=np.ones((2, eng.nr)), rate_mult_row=rows)
    rows[5] = -1
    with pytest.raises(RuntimeError, match=r"-10: rate_mult_row\[5\] = -1"):
        eng.integrate_phase(T, Asv, U0, tf, [1.0], rate_mult=np.ones((2, eng.nr)), rate_mult_row=rows)
    mult = np.ones((N, eng.nr))
    mult[30, 2] = -1.0                                   # the index in the ensemble, not in the shard
    e2 = pkg.Engine(pm)
    with pytest.raises(RuntimeError, match=r"-10: rate_mult\[30\]\[2\]"):
        pkg.integrate_multi([eng, e2], T, Asv, U0, tf, rate_mult=mult)
    e2.close()
    U, st = eng.integrate(T, Asv, U0, tf, rate_mult=np.zeros((1, eng.nr)), rate_mult_row=np.zeros(N, np.int32))
    assert _same(U, U0) and np.all(st["status"] == 0)    # 0 is allowed: every reaction off, nothing happens


# --------------------------------------------------------------------------------- 7. br_sensitivity, explicit
def _sens_table(nr, rxn, f):
    tab = np.ones((2 * len(rxn) + 1, nr))
    for j, r in enumerate(rxn):
        tab[1 + 2 * j, r] = f
        tab[2 + 2 * j, r] = 1.0 / f
    return tab


def _explicit(eng, T, Asv, U0, tf, rxn, f, **kw):
    """the 2 nsel + 1 runs of every base reactor through br_integrate with a hand-built table:
    (u [N, rows, n], stats of [N, rows])"""
    N, rows = len(T), 2 * len(rxn) + 1
    rep = lambda a: np.repeat(np.asarray(a), rows, axis=0)
    U, st = eng.integrate(rep(T), rep(Asv), rep(U0), rep(tf), rate_mult=_sens_table(eng.nr, rxn, f),
                          rate_mult_row=np.tile(np.arange(rows, dtype=np.int32), N), **kw)
    return U.reshape(N, rows, -1), {k: v.reshape(N, rows) for k, v in st.items()}


def test_sensitivity_equals_explicit_runs(pkg, gpu, monkeypatch):
    """H2/O2, 5 base reactors, all 18 reactions, f = 2, against 5 x 37 runs of br_integrate with the same
    table. S_u is one subtraction and one division of the same numbers: equal to 1e-14 relative. S_tign
    differs by the device's log: each ln t carries a relative error of a few 1e-16, so the bound is 1e-14
    relative to the logarithms that are subtracted, 1e-14 (|ln t+| + |ln t-|) / (2 ln f). max_steps is
    the largest step count of the unperturbed runs, so the perturbed runs that need more steps fail and NaN
    entries exist; they must coincide, and nbad must count them. BRHIP_SENS_CHUNK = 2 (three launches, the
    last one partial) gives the default chunk's bits."""
    from batchreactor_amd import ensemble
    monkeypatch.delenv("BRHIP_ENGINE", raising=False)
    monkeypatch.delenv("BRHIP_SENS_CHUNK", raising=False)
    pm = pkg.Mechanism.from_files(LIB, **FILES["h2o2"])
    eng = pkg.Engine(pm)
    N, f = 5, 2.0
    T, Asv, U0 = ensemble.make_inputs(pm, "h2o2", 0, N)
    tf = np.full(N, 2e-3)
    rxn = np.arange(eng.nr)
    _, s0 = eng.integrate(T, Asv, U0, tf)
    kw = dict(max_steps=int(s0["nsteps"].max()))         # some perturbed runs need more steps: they fail
    out = eng.sensitivity(T, Asv, U0, tf, factor=f, states=True, **kw)
    assert out["S_tign"].shape == (N, 18) and out["S_u"].shape == (N, 18, pm.n)
    Ue, se = _explicit(eng, T, Asv, U0, tf, rxn, f, **kw)
    assert _same(out["u"], Ue[:, 0]) and _same(out["stats"]["t_ign"], se["t_ign"][:, 0])
    assert _same(out["stats"]["nsteps"], se["nsteps"][:, 0])
    ok = (se["status"][:, 1::2] == 0) & (se["status"][:, 2::2] == 0)
    tp, tm = se["t_ign"][:, 1::2], se["t_ign"][:, 2::2]
    good = ok & np.isfinite(tp) & np.isfinite(tm)
    den = 2.0 * np.log(f)
    with np.errstate(invalid="ignore"):
        St = np.where(good, (np.log(tp) - np.log(tm)) / den, np.nan)
        Su = np.where(ok[:, :, None], (Ue[:, 1::2] - Ue[:, 2::2]) / den, np.nan)
        bound = 1e-14 * (np.abs(np.log(tp)) + np.abs(np.log(tm))) / den
    assert _same(np.isnan(out["S_tign"]), np.isnan(St)) and _same(np.isnan(out["S_u"]), np.isnan(Su))
    assert out["nbad"] == int(np.isnan(St).sum() + np.isnan(Su).sum())
    assert good.sum() >= 36 and (~ok).sum() >= 1, (good.sum(), (~ok).sum())
    d = np.abs(out["S_tign"] - St)[good]
    print("S_tign: max |device - explicit| / bound =", float((d / bound[good]).max()), " largest |S| =", float(np.nanmax(np.abs(St))))
    assert np.all(d <= bound[good])
    np.testing.assert_allclose(out["S_u"][ok], Su[ok], rtol=1e-14, atol=0.0)
    assert np.nanmax(np.abs(St)) > 0.3                    # (real sensitivities, not zeros)
    monkeypatch.setenv("BRHIP_SENS_CHUNK", "2")
    o2 = eng.sensitivity(T, Asv, U0, tf, factor=f, states=True, **kw)
    for k in ("S_tign", "S_u", "u"):
        assert _same(o2[k], out[k]), k
    assert o2["nbad"] == out["nbad"] and _same(o2["stats"]["nsteps"], out["stats"]["nsteps"])
    sub = eng.sensitivity(T, Asv, U0, tf, factor=f, reactions=[17, 0, 4], **kw)       # a selection, in its order
    assert _same(sub["S_tign"], out["S_tign"][:, [17, 0, 4]]) and "S_u" not in sub


# --------------------------------------------------------------------------------- 8. br_sensitivity, oracle
GRI_TOP12 = [154, 37, 52, 117, 158, 155, 10, 160, 9, 31, 283, 144]     # the largest |S_tign| in the oracle
SENS_CASES = {"h2o2-1000K": ("h2o2", {"H2": 0.3, "O2": 0.2, "N2": 0.5}, 1000.0, 1e5, 2e-3, None),
              "h2o2-1200K": ("h2o2", {"H2": 0.3, "O2": 0.2, "N2": 0.5}, 1200.0, 3e5, 5e-4, None),
              "gri": ("gri", {"CH4": 0.25, "O2": 0.5, "N2": 0.25}, 1200.0, 1e5, 2e-2, GRI_TOP12 + [0, 100, 200, 324])}


@pytest.mark.parametrize("name", list(SENS_CASES))
def test_ignition_sensitivity_against_the_oracle(pkg, orc, gpu, monkeypatch, name):
    """d ln t_ign / d ln k_r by br_sensitivity (f = 2, default tolerances, analytic Jacobian) against the
    same central difference of the oracle's ignition times with set_rxn_mult(r, f, f) and (r, 1/f, 1/f).
    The bound per entry is derived: t_ign is the midpoint of the steepest accepted step, known to within
    that step, so each of the four runs (GPU +, GPU -, oracle +, oracle -) contributes ign_dt / t_ign to
    the difference of the logarithms; the tolerance is their sum over 2 ln f. The test is only worth
    something where sensitivities stand out of that: at least three reactions must have |S_oracle| > 4 x
    their tolerance. H2/O2: sum_r S_tign = -1 over all reactions (every rate times c is time over c), to
    within the summed tolerances."""
    case, comp, T0, p0, tf0, sel = SENS_CASES[name]
    monkeypatch.delenv("BRHIP_ENGINE", raising=False)
    monkeypatch.delenv("BRHIP_SENS_CHUNK", raising=False)
    pm = pkg.Mechanism.from_files(LIB, **FILES[case])
    om = orc.Mech(os.path.join(LIB, FILES[case]["gas_mech"]), os.path.join(LIB, "therm.dat"))
    eng = pkg.Engine(pm)
    rxn = np.arange(pm.nrg) if sel is None else np.array(sel)
    assert len(rxn) == (18 if sel is None else 16) and rxn.max() < pm.nrg
    f = 2.0
    u0 = pm.initial_state(T0, p0, pm.mole_fractions(comp))
    T, Asv, U0, tf = np.array([T0]), np.ones(1), u0[None, :], np.array([tf0])
    out = eng.sensitivity(T, Asv, U0, tf, factor=f, reactions=rxn)
    S = out["S_tign"][0]
    assert out["nbad"] == 0 and np.all(np.isfinite(S))
    _, se = _explicit(eng, T, Asv, U0, tf, rxn, f)       # the perturbed runs' own ign_dt / t_ign
    rel_g = (se["ign_dt"] / se["t_ign"])[0]
    den = 2.0 * np.log(f)
    So, tol = np.zeros(len(rxn)), np.zeros(len(rxn))
    for j, r in enumerate(rxn):
        t, rel = [], []
        for m in (f, 1.0 / f):
            om.set_rxn_mult(int(r), m, m)
            _, so, _ = om.integrate(T0, 1.0, u0, tf0, analytic_jac=True)
            assert so["status"] == 0 and so["t_ign"] < tf0
            t.append(so["t_ign"])
            rel.append(so["ign_dt"] / so["t_ign"])
        om.set_rxn_mult(int(r), 1.0, 1.0)
        So[j] = (np.log(t[0]) - np.log(t[1])) / den
        tol[j] = (rel[0] + rel[1] + rel_g[1 + 2 * j] + rel_g[2 + 2 * j]) / den
    for j, r in enumerate(rxn):
        print(f"{name} r={int(r):3d}  S_gpu={S[j]:+.5f}  S_oracle={So[j]:+.5f}  |diff|={abs(S[j] - So[j]):.2e}  tol={tol[j]:.2e}")
    assert (np.abs(So) > 4 * tol).sum() >= 3, (So, tol)
    assert np.all(np.abs(S - So) <= tol), np.flatnonzero(np.abs(S - So) > tol)
    if sel is None:
        print(f"{name} sum S_gpu = {S.sum():+.5f}, sum S_oracle = {So.sum():+.5f}, summed tol = {tol.sum():.2e}")
        assert abs(S.sum() + 1.0) <= tol.sum(), (S.sum(), tol.sum())
