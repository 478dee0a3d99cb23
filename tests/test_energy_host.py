"""Adiabatic constant-volume reactors (br_opts.energy), the part that needs no GPU: the new br_opts fields in
every binding, the input errors that are answered before the handle is looked at, the numpy statement of the
model's thermodynamics (Mechanism.thermo_e_cv / internal_energy), and the CPU statement of a run
(br_integrate_host on f(t, [u, T]), tests/energy_cases.py) against SciPy's Radau on both regimes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import energy_cases as ec
from conftest import LIB, ROOT
from test_gpu_parity import close_states

BR_ERR_INPUT = -10


def test_opts_fields_version_and_bindings(pkg):
    """energy, T_end, T_out sit together in front of nout in the header, the Python and the Julia struct, the
    fields from ntprog to tout_per_reactor keep their order behind yout, br_version() tells the layout."""
    L = pkg._lib
    assert L.lib().br_version() >= 230
    names = [f[0] for f in L.Opts._fields_]
    k = names.index("energy")
    assert names[k - 1:k + 4] == ["ignition_species", "energy", "T_end", "T_out", "nout"]
    assert [f[1] for f in L.Opts._fields_[k:k + 3]] == [C.c_int, L.dp, L.dp]
    assert names[k + 4:] == ["tout", "yout", "ntprog", "tprog_t", "tprog_T", "ntprog_rows", "tprog_row", "dq_jacobian", "nmult",
                             "rate_mult", "rate_mult_row", "tout_per_reactor"]
    o = L.Opts()
    assert o.energy == 0 and not o.T_end and not o.T_out
    hdr = open(os.path.join(ROOT, "include", "brhip.h")).read()
    body = hdr.split("typedef struct br_opts {")[1].split("} br_opts;")[0]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    hnames = [d.strip().split()[-1].lstrip("*") for st in body.split(";") for d in st.split(",") if d.strip()]
    assert hnames == names
    assert "#define BR_ENERGY_ADIABATIC_V 1" in hdr and L.ENERGY_ADIABATIC_V == 1
    jl = re.sub(r"#[^\n]*", "", open(os.path.join(ROOT, "julia", "BatchReactorHIP.jl")).read())
    jbody = jl.split("\nstruct BrOpts")[1].split("\nend")[0]
    jnames = [f.split("::")[0].strip() for ln in jbody.split("\n") for f in ln.split(";") if "::" in f]
    assert jnames == names
    assert "with_energy(o::BrOpts" in jl and "with_energy" in jl.split("\nexport ")[1]
    assert "br_debug_energy_eval" in L.EXPORTS and hasattr(L.lib(), "br_debug_energy_eval")
    assert pkg.engine.energy_mode(None) == 0 and pkg.engine.energy_mode("adiabatic") == 1
    with pytest.raises(ValueError):
        pkg.engine.energy_mode("isobaric")


@pytest.mark.parametrize("entry", ["br_integrate", "br_integrate_traced", "br_integrate_multi", "br_integrate_phase",
                                   "br_integrate_dev", "br_sensitivity"])
def test_input_errors_before_the_handle(pkg, entry):
    """A bad energy value, and energy together with a temperature programme, are BR_ERR_INPUT with a message that
    names the cause, from every entry point that takes br_opts, with a NULL handle: nothing reaches a GPU."""
    L = pkg._lib
    N = 2
    u, tf, st = np.ones((N, 3)), np.ones(N), np.zeros((N, L.NSTAT))
    kt, kT = np.zeros((N, 1)), np.full((N, 1), 1000.0)

    def call(o):
        a = (L.dptr(tf), L.dptr(tf), L.dptr(u), L.dptr(tf), C.byref(o))
        lib = L.lib()
        if entry == "br_integrate":
            return lib.br_integrate(None, N, *a, L.dptr(st))
        if entry == "br_integrate_traced":
            return lib.br_integrate_traced(None, N, *a, L.dptr(st), L.dptr(st))
        if entry == "br_integrate_multi":
            return lib.br_integrate_multi(None, 1, N, *a, L.dptr(st))
        if entry == "br_integrate_phase":
            return lib.br_integrate_phase(None, N, *a, L.dptr(st), 1, L.dptr(tf), L.dptr(tf), L.dptr(u))
        if entry == "br_integrate_dev":
            return lib.br_integrate_dev(None, N, None, None, None, None, C.byref(o), None, None)
        return lib.br_sensitivity(None, N, *a[:4], a[4], 2.0, 1, None, None, None, None, None, None)

    for bad in (2, -1, 7):
        rc = call(L.Opts(rtol=1e-6, atol=1e-10, energy=bad))
        msg = L.lib().br_last_error().decode()
        assert rc == BR_ERR_INPUT and "br_opts.energy" in msg and str(bad) in msg, (entry, bad, rc, msg)
    o = L.Opts(rtol=1e-6, atol=1e-10, energy=1, ntprog=1, ntprog_rows=N, tprog_t=L.dptr(kt), tprog_T=L.dptr(kT))
    rc = call(o)
    msg = L.lib().br_last_error().decode()
    if entry == "br_sensitivity":      # (a programme alone is already refused there, before anything else)
        assert rc == -30 and "temperature programme" in msg, (rc, msg)
    else:
        assert rc == BR_ERR_INPUT and "energy" in msg and "programme" in msg, (entry, rc, msg)
    # a good energy request gets as far as the NULL handle
    rc = call(L.Opts(rtol=1e-6, atol=1e-10, energy=1))
    assert rc == BR_ERR_INPUT and "br_opts.energy" not in L.lib().br_last_error().decode(), entry


@pytest.mark.parametrize("mech", ["h2o2.dat", "grimech.dat"])
def test_thermo_e_cv_against_differences_of_internal_energy(pkg, mech):
    """cv_k = d e_k / dT: thermo_e_cv's cv against central differences of internal_energy of one mole per m3 of
    each species, to 1e-7 relative, at temperatures in both NASA ranges away from every Tmid; e and cv switch
    range exactly at Tmid (low range below, high range at and above); the clamp holds e and cv outside
    [200, 6000] K; internal_energy is sum_k c_k e_k."""
    pm = pkg.Mechanism.from_files(LIB, gas_mech=mech)
    tmid = pm.nasa[:, 0]
    Ts = np.array([300.0, 450.0, 700.0, 950.0, 1050.0, 1250.0, 2000.0, 2900.0, 4000.0, 5500.0])
    assert np.all(np.abs(Ts[:, None] - tmid[None, :]) > 20.0)
    I = np.diag(pm.molwt)                       # u = M_k e_k: c = e_k, so internal_energy(u, T) = e_k(T)
    worst = 0.0
    for T in Ts:
        e, cv = pm.thermo_e_cv(T)
        h = 1e-4 * T
        d = (pm.internal_energy(I, np.full(pm.ng, T + h)) - pm.internal_energy(I, np.full(pm.ng, T - h))) / (2 * h)
        assert np.allclose(pm.internal_energy(I, np.full(pm.ng, T)), e, rtol=1e-15, atol=0)
        worst = max(worst, float(np.max(np.abs(d - cv) / np.abs(cv))))
    print(f"\n  {mech}: max |dE/dT - cv| / cv = {worst:.3g}")
    assert worst <= 1e-7
    for k in (0, pm.ng - 1):                    # the branch rule at Tmid itself
        a_hi, a_lo, Tm = pm.nasa[k, 1:8], pm.nasa[k, 8:15], tmid[k]
        cp = lambda a, T: a[0] + a[1] * T + a[2] * T ** 2 + a[3] * T ** 3 + a[4] * T ** 4
        hi, lo = (cp(a_hi, Tm) - 1.0) * 8.31446261815324, (cp(a_lo, Tm) - 1.0) * 8.31446261815324
        assert abs(hi - lo) > 1e-9 * abs(hi)                            # (the two fits do differ at Tmid)
        assert abs(pm.thermo_e_cv(Tm)[1][k] - hi) <= 1e-14 * abs(hi)
        assert abs(pm.thermo_e_cv(np.nextafter(Tm, 0.0))[1][k] - lo) <= 1e-14 * abs(lo)
    for Tout, Tin in ((150.0, 200.0), (-5.0, 200.0), (7000.0, 6000.0)):
        assert all(np.array_equal(a, b) for a, b in zip(pm.thermo_e_cv(Tout), pm.thermo_e_cv(Tin)))
    assert np.all(np.isnan(pm.thermo_e_cv(np.nan)[0]))
    rng = np.random.default_rng(2)
    u = rng.random((4, pm.ng))
    T = np.array([400.0, 900.0, 1500.0, 3000.0])
    want = [np.sum(u[i] / pm.molwt * pm.thermo_e_cv(T[i])[0]) for i in range(4)]
    assert np.allclose(pm.internal_energy(u, T), want, rtol=1e-15, atol=0)


@pytest.mark.parametrize("name", list(ec.REGIMES))
def test_cpu_statement_against_radau(pkg, orc, name):
    """br_integrate_host on f(t, [u, T]) at rtol 1e-10 / atol 1e-16 against SciPy's Radau at the same tolerances,
    conv = 0: the end state, T included, to 1e-6 relative (floor 1e-14), and within 0.5 of that bar, so that the
    GPU run can be held to the bar itself. The regimes ignite (T_end is the burnt temperature), and the run's
    drift of E = sum_k c_k e_k(T), which the model conserves identically, is what test_energy_gpu.py measures
    the device run's against."""
    pm, om, y0, tf = ec.mechs(pkg, orc, name, 0)
    ref = ec.radau_end(pkg, orc, name)
    run = ec.host_run(pkg, orc, name, 0, rtol=1e-10, atol=1e-16)
    e = close_states(run["y"], ref, rtol=1e-6, floor=1e-14)
    drift = float(np.max(np.abs(run["E"] / run["E"][0] - 1.0)))
    print(f"\n  {name}: T_end {run['y'][-1]:.1f} K (Radau {ref[-1]:.1f}), t_ign {run['t_ign']:.3g} s, "
          f"error {e:.3g} of the 1e-6 bar, E drift {drift:.3g}, {int(run['stats'][0])} steps")
    want_T, want_tign = {"h2o2": (2963.5, 5.8e-5), "gri": (2925.9, 1.06e-3)}[name]
    assert abs(ref[-1] - want_T) <= 0.06 and abs(run["t_ign"] / want_tign - 1.0) <= 0.05
    assert e <= 0.5, (name, e)
    assert drift <= 1e-6                      # (a truncation-level drift, not a missing term)
