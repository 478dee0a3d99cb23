"""The clock columns of br_stats (cyc_rhs, cyc_jac, cyc_lu, cyc_sol, cyc_ctl, cyc_clk) in every engine:
all 0 from the product library, per-phase shader clocks from the diagnostic build (libbrhip_diag.so).
Every engine writes the record through the named br_stats fields; a swapped or shifted column shows
here as a zero, a phase sum above the reactor's own clock, or GRI's phases out of their measured order.

_lib reads BRHIP_LIB at import, so each library runs in a child process of its own (this file as a
script), which integrates the four small cases one after another (BRHIP_ENGINE is read per call).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "batchreactor.jl_amd")
CLOCKS = ("cyc_rhs", "cyc_jac", "cyc_lu", "cyc_sol", "cyc_ctl", "cyc_clk")
PHASES = CLOCKS[:5]
DETERMINISTIC = ("nsteps", "nfe", "nje", "nsetups", "nni", "ncfn", "netf", "status", "t_end", "t_ign", "ign_rate",
                 "ign_dt", "nfe_dq")
# case -> (BRHIP_ENGINE or None for the mechanism's default, mechanism file, reactors, kernel)
CASES = {"quad": (None, "h2o2.dat", 8, "k_group<16, 9>"), "lane": ("lane", "h2o2.dat", 8, "k_lane<9>"),
         "wave": ("wave", "h2o2.dat", 8, "k_integrate<16>"), "gri": (None, "grimech.dat", 4, "k_integrate<56>")}


def _child():
    """integrate every case with the library BRHIP_LIB names; one JSON line {case: {field: [per reactor]}}"""
    sys.path.insert(0, ROOT)
    import _pkgload
    pkg = _pkgload.load()
    lib = os.path.join(ROOT, "tests", "golden", "lib")
    out = {}
    for case, (engine, mech_file, N, kernel) in CASES.items():
        if engine is None:
            os.environ.pop("BRHIP_ENGINE", None)
        else:
            os.environ["BRHIP_ENGINE"] = engine
        m = pkg.Mechanism.from_files(lib, gas_mech=mech_file)
        eng = pkg.Engine(m, device=0)
        assert eng.kernel_name == kernel, (case, eng.kernel_name)
        rng = np.random.default_rng(7)                       # the inputs of smoke()
        T = rng.uniform(1100.0, 1300.0, N)
        x = m.mole_fractions({"H2": 0.25, "O2": 0.25, "N2": 0.5} if mech_file == "h2o2.dat"
                             else {"CH4": 0.25, "O2": 0.5, "N2": 0.25})
        U0 = np.stack([m.initial_state(T[i], 1e5, x) for i in range(N)])
        _, st = eng.integrate(T, np.ones(N), U0, 1e-2)
        eng.close()
        out[case] = {k: [float(v) for v in st[k]] for k in CLOCKS + DETERMINISTIC + ("cyc_total",)}
    print(json.dumps(out))


def run_library(path):
    """the stats of every case from library `path`, in a fresh process under its own time limit"""
    env = dict(os.environ, BRHIP_LIB=path)
    env.pop("BRHIP_ENGINE", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (path, r.stderr[-2000:])
    st = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    return {c: {k: np.array(v) for k, v in d.items()} for c, d in st.items()}


def check_common(st):
    for case, s in st.items():
        for k in DETERMINISTIC:   # (both mechanisms have the ignition marker species: t_ign is tracked)
            assert np.all(np.isfinite(s[k])), (case, k, s[k])
        assert np.all(s["nsteps"] > 0), (case, s["nsteps"])


def check_product(st):
    check_common(st)
    for case, s in st.items():
        for k in CLOCKS:
            assert np.all(s[k] == 0.0), (case, k, s[k])
        assert np.all(s["cyc_total"] > 0), (case, s["cyc_total"])
        assert np.all(s["status"] == 0), (case, s["status"])


def check_diag(st):
    check_common(st)
    for case, s in st.items():
        print(case, {k: s[k].tolist() for k in CLOCKS})
        for k in CLOCKS:
            assert np.all(s[k] > 0), (case, k, s[k])
        if case != "lane":   # (the lane engine's first refill interval opens before cyc_clk's origin)
            total = sum(s[k] for k in PHASES)
            assert np.all(total <= s["cyc_clk"]), (case, total, s["cyc_clk"])
    g = {k: float(np.sum(st["gri"][k])) for k in PHASES}
    # the order of DESIGN.md section 3's measured GRI shares: Jacobian 6 %, solve 15 %, LU 26 %, RHS 27 %
    assert g["cyc_jac"] < g["cyc_sol"] < g["cyc_lu"] and g["cyc_jac"] < g["cyc_rhs"], g


@pytest.mark.gpu
@pytest.mark.parametrize("library,check", [("libbrhip.so", check_product), ("libbrhip_diag.so", check_diag)],
                         ids=["product", "diagnostic"])
def test_clock_columns(gpu, library, check):
    check(run_library(os.path.join(PKG, library)))


if __name__ == "__main__":
    _child()
