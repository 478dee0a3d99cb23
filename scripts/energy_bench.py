"""Cost of an adiabatic constant-volume run (br_opts.energy) on the wavefront engine: kernel ms and steps/s of the
same reactors run isothermally with CVODE's DQ Jacobian and adiabatically (the energy instance: ng + 1 equations,
DQ Jacobian over ng + 1 columns, the T-only constants refreshed whenever an RHS sees another T), H2/O2 on
k_integrate<16> and GRI on k_integrate<56>. Prints one JSON line; profiles/energy_ab.json keeps a run of it.
With BRHIP_LIB set to the phase-clock build it also reports the share of the reactor clocks spent in the RHS
interval, which contains the refresh.  usage: python scripts/energy_bench.py [N_h2o2] [N_gri]"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["BRHIP_ENGINE"] = "wave"
import _pkgload  # noqa: E402

pkg = _pkgload.load()
from batchreactor_amd import ensemble  # noqa: E402

LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "lib")
CASES = {"h2o2": (dict(gas_mech="h2o2.dat"), 2e-3), "gri": (dict(gas_mech="grimech.dat"), 1e-2)}


def timed(eng, reps, *a, **kw):
    eng.integrate(*a, **kw)                               # warm-up
    ms, st = [], None
    for _ in range(reps):
        _, st = eng.integrate(*a, **kw)
        ms.append(eng.last_kernel_ms())
    clk = float(st["cyc_clk"].sum())                      # > 0 in the phase-clock build only (BRHIP_LIB=libbrhip_diag.so)
    rhs_share = float(st["cyc_rhs"].sum()) / clk if clk > 0 else None
    return ms, st, rhs_share


def main():
    n = {"h2o2": int(sys.argv[1]) if len(sys.argv) > 1 else 4096, "gri": int(sys.argv[2]) if len(sys.argv) > 2 else 4096}
    out = {}
    for case, (files, tf) in CASES.items():
        pm = pkg.Mechanism.from_files(LIB, **files)
        N = n[case]
        T, Asv, U0 = ensemble.make_inputs(pm, case, 0, N)
        eng = pkg.Engine(pm)
        tfv = np.full(N, tf)
        res = {}
        for name, kw in (("isothermal DQ", dict(dq_jacobian=True)), ("adiabatic", dict(energy="adiabatic"))):
            ms, st, share = timed(eng, 3, T, Asv, U0, tfv, **kw)
            mean, steps = float(np.mean(ms)), float(st["nsteps"].sum())
            res[name] = {"kernel_ms": mean, "kernel_ms_runs": [float(x) for x in ms], "steps": steps,
                         "nfe": float(st["nfe"].sum() + st["nfe_dq"].sum()), "failed": int((st["status"] != 0).sum()),
                         "steps_per_s": steps / (mean * 1e-3)}
            if share is not None:
                res[name]["rhs_share"] = share
            if "T_end" in st:
                res[name]["T_end_mean"] = float(st["T_end"].mean())
        res["steps_per_s_ratio"] = res["adiabatic"]["steps_per_s"] / res["isothermal DQ"]["steps_per_s"]
        out[case] = {"reactors": N, "tf": tf, "kernel": eng.kernel_name, **res}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
