"""Shared cases of the group-engine energy tests (test_energy_group_kernels.py, test_energy_group_gpu.py; test
infrastructure). tests/energy_cases.py keys its regimes by files of the mechanism library; the mechanisms here are
written at test time (GRI subsets, H2/O2 with inert species), so the CPU statement (br_integrate_host on
energy_cases.rhs_fn), the Radau reference and the host energy drift are built here, in energy_cases' form, once per
process (callers must not modify them). Everything in this module runs on the CPU."""
import os

import numpy as np

import energy_cases as ec
from test_gpu_parity import _h2o2_with_inerts
from test_group_kernels import S24, subset_mechanism

S8 = "H2 H O O2 OH H2O HO2 H2O2".split()
# regimes of the written mechanisms (none starts at a Tmid); Radau at rtol 1e-8: T passes T0 + 400 K at 3.3e-5 s
# (s8) and 1.07e-3 s (s24), T_end 3342.9 K and 2944.7 K at conv = 0
REGIMES = {
    "s8": dict(species=S8, x={"H2": 0.6, "O2": 0.4}, p=1e5, T0=1100.0, tf=1e-3),
    "s24": dict(species=S24, x={"CH4": 0.1, "O2": 0.2, "N2": 0.7}, p=1e5, T0=1500.0, tf=5e-3),
}
_cache = {}


def written(pkg, orc, tmp_path_factory, key, conv):
    """(product mechanism, oracle mechanism) of a written mechanism: "s8", "s24" (GRI subsets) or "h2o2_n<ng>" (H2/O2
    with inert species up to ng); one directory per process and key"""
    ck = ("mech", key, conv)
    if ck not in _cache:
        dk = ("dir", key)
        if dk not in _cache:
            tmp = tmp_path_factory.mktemp("eg_" + key)
            _cache[dk] = (_h2o2_with_inerts(tmp, int(key.split("_n")[1])) if key.startswith("h2o2_n")
                          else subset_mechanism(tmp, REGIMES[key]["species"], name=key))
        d = _cache[dk]
        _cache[ck] = (pkg.Mechanism.from_files(d, gas_mech="mech.dat", conv=conv),
                      orc.Mech(os.path.join(d, "mech.dat"), os.path.join(d, "therm.dat"), None, conv=conv))
    return _cache[ck]


def regime(pkg, orc, tmp_path_factory, key, conv):
    """(pm, om, y0 = [u0, T0], tf) of a REGIMES entry, as energy_cases.mechs"""
    pm, om = written(pkg, orc, tmp_path_factory, key, conv)
    r = REGIMES[key]
    u0 = pm.initial_state(r["T0"], r["p"], pm.mole_fractions(r["x"]))
    return pm, om, np.append(u0, r["T0"]), r["tf"]


def radau_end(pkg, orc, tmp_path_factory, key):
    """[u, T] at tf from SciPy's Radau at rtol 1e-10 / atol 1e-16, conv = 0 (energy_cases.radau_end's settings)"""
    ck = ("radau", key)
    if ck not in _cache:
        from scipy.integrate import solve_ivp
        pm, om, y0, tf = regime(pkg, orc, tmp_path_factory, key, 0)
        sol = solve_ivp(ec.rhs_fn(pm, om), (0.0, tf), y0, method="Radau", rtol=1e-10, atol=1e-16)
        assert sol.status == 0, sol.message
        _cache[ck] = sol.y[:, -1].copy()
    return _cache[ck]


def host_run(pkg, orc, tmp_path_factory, key, conv, rtol=1e-6, atol=1e-10):
    """The CPU statement of an energy run of a REGIMES entry, as energy_cases.host_run: accepted steps t, Y, the end
    state y, stats, and E = internal_energy at every step"""
    ck = ("host", key, conv, rtol, atol)
    if ck not in _cache:
        pm, om, y0, tf = regime(pkg, orc, tmp_path_factory, key, conv)
        rows = []
        status, y, st = pkg._lib.integrate_host(ec.rhs_fn(pm, om), y0, tf, rtol=rtol, atol=atol,
                                                on_step=lambda t, u: rows.append((t, u)))
        assert status == 0, (key, conv, status)
        t = np.array([r[0] for r in rows])
        Y = np.array([r[1] for r in rows])
        if t[-1] - t[-2] <= 1e-12 * tf:          # (the tf row repeats the last accepted step, which lands on tf)
            t, Y = np.delete(t, -2), np.delete(Y, -2, axis=0)
        _cache[ck] = dict(t=t, Y=Y, y=y, stats=st, E=pm.internal_energy(Y[:, :-1], Y[:, -1]))
    return _cache[ck]
