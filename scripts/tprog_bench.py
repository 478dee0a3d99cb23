"""Cost of a temperature-programme run on the wavefront engine: kernel ms and steps/s of the same reactors
run isothermally, with a constant programme (never refreshes) and with a ramp (refreshes at every step
attempt), for the GRI and the surface-only bench configs. Prints one JSON line; profiles/tprog_ab.json
keeps a run of it. With BRHIP_LIB set to the phase-clock build it also reports the share of the reactor
clocks spent in the RHS interval, which contains the refresh.  usage: python scripts/tprog_bench.py [N_gri] [N_surf]"""
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
CASES = {"gri": (dict(gas_mech="grimech.dat"), 1e-2, 100.0),
         "surf": (dict(surface_mech="ch4ni.xml", gasphase=["CH4", "H2O", "H2", "CO", "CO2", "O2", "N2"]), 1.0, 150.0)}


def timed(eng, reps, *a, **kw):
    eng.integrate(*a, **kw)                               # warm-up
    ms, st = [], None
    for _ in range(reps):
        _, st = eng.integrate(*a, **kw)
        ms.append(eng.last_kernel_ms())
    clk = float(st["cyc_clk"].sum())                      # > 0 in the phase-clock build only (BRHIP_LIB=libbrhip_diag.so)
    rhs_share = float(st["cyc_rhs"].sum()) / clk if clk > 0 else None
    return (float(np.mean(ms)), float(np.min(ms)), float(np.max(ms)), float(st["nsteps"].sum()),
            float(st["nfe"].sum() + st["nfe_dq"].sum()), rhs_share)


def main():
    n = {"gri": int(sys.argv[1]) if len(sys.argv) > 1 else 8192, "surf": int(sys.argv[2]) if len(sys.argv) > 2 else 16384}
    out = {}
    for case, (files, tf, dT) in CASES.items():
        pm = pkg.Mechanism.from_files(LIB, **files)
        N = n[case]
        T, Asv, U0 = ensemble.make_inputs(pm, case, 0, N)
        eng = pkg.Engine(pm)
        tfv = np.full(N, tf)
        const = (np.zeros((N, 1)), T[:, None].copy())
        ramp = (np.stack([np.zeros(N), tfv], axis=1), np.stack([T, T + dT], axis=1))
        res = {}
        for name, Targ, kw in (("isothermal", T, {}), ("constant programme", None, dict(tprog=const)),
                               ("ramp", None, dict(tprog=ramp))):
            mean, lo, hi, steps, nfe, share = timed(eng, 3, Targ, Asv, U0, tfv, **kw)
            res[name] = {"kernel_ms": mean, "kernel_ms_min": lo, "kernel_ms_max": hi, "steps": steps, "nfe": nfe,
                         "steps_per_s": steps / (mean * 1e-3)}
            if share is not None:   # the refresh runs inside the RHS interval of the phase clocks: the ramp's
                res[name]["rhs_share"] = share   # rhs_share minus the constant programme's is the refresh's share
        out[case] = {"reactors": N, "tf": tf, "ramp_K": dT, "kernel": eng.kernel_name, **res}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
