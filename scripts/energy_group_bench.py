"""Adiabatic constant-volume reactors (br_opts.energy) on the wavefront energy instance against the group energy
instance (k_group<GL, NM, true>: four or two reactors per wave), the same reactors in one process: H2/O2 (quad,
<16, 16>) and the 24-species GRI subset of the tests (pair, <32, 32>). One warm-up each, then five timed pairs,
alternating the two engines (BRHIP_ENGINE is read at every launch). Per engine: kernel ms per run
(last_kernel_ms), steps, nfe + nfe_dq, failures, reactors/s, steps/s and the spread of its five runs; the ratio
group / wave of reactors/s; the worst close_states (rtol 1e-4) between the two engines' end states and T_end.
Prints one JSON line; profiles/energy_group_ab.json keeps a run of it.
usage: python scripts/energy_group_bench.py [N_h2o2] [N_s24]"""
import json
import os
import pathlib
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _pkgload  # noqa: E402

pkg = _pkgload.load()
from batchreactor_amd import ensemble  # noqa: E402
from test_gpu_parity import close_states  # noqa: E402
from test_group_kernels import S24, subset_mechanism  # noqa: E402

LIB = os.path.join(ROOT, "tests", "golden", "lib")
PAIRS = 5


def cases(tmp, n_h2o2, n_s24):
    pm = pkg.Mechanism.from_files(LIB, gas_mech="h2o2.dat")
    T, Asv, U0 = ensemble.make_inputs(pm, "h2o2", 0, n_h2o2)
    yield "h2o2", "quad", pm, T, Asv, U0, 2e-3
    d = subset_mechanism(pathlib.Path(tmp), S24, name="s24")
    pm = pkg.Mechanism.from_files(d, gas_mech="mech.dat")
    T = np.random.default_rng(0).uniform(1450.0, 1700.0, n_s24)
    x = pm.mole_fractions({"CH4": 0.1, "O2": 0.2, "N2": 0.7})
    U0 = np.stack([pm.initial_state(Ti, 1e5, x) for Ti in T])
    yield "s24", "pair", pm, T, np.ones(n_s24), U0, 5e-3


def main():
    n_h2o2 = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
    n_s24 = int(sys.argv[2]) if len(sys.argv) > 2 else 16384
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for case, group, pm, T, Asv, U0, tf in cases(tmp, n_h2o2, n_s24):
            N = len(T)
            eng = pkg.Engine(pm)
            tfv = np.full(N, tf)
            engines = {"wave": "wave", "group": group}
            res = {k: {"kernel_ms_runs": []} for k in engines}
            last = {}
            for rep in range(PAIRS + 1):                      # rep 0: the warm-up of each
                for k, env in engines.items():
                    os.environ["BRHIP_ENGINE"] = env
                    if rep == 0:
                        res[k]["kernel"] = eng.energy_kernel_name
                        res[k]["launch"] = eng.energy_launch_info()
                    last[k] = eng.integrate(T, Asv, U0, tfv, energy="adiabatic")
                    if rep:
                        res[k]["kernel_ms_runs"].append(eng.last_kernel_ms())
            for k in engines:
                U, st = last[k]
                ms = res[k]["kernel_ms_runs"]
                mean, steps = float(np.mean(ms)), float(st["nsteps"].sum())
                res[k].update(kernel_ms=mean, spread_ms=float(np.ptp(ms)), steps=steps,
                              nfe=float(st["nfe"].sum() + st["nfe_dq"].sum()), failed=int((st["status"] != 0).sum()),
                              reactors_per_s=N / (mean * 1e-3), steps_per_s=steps / (mean * 1e-3),
                              T_end_mean=float(st["T_end"].mean()))
            (Uw, sw), (Ug, sg) = last["wave"], last["group"]
            worst = max(close_states(np.append(Ug[i], sg["T_end"][i]), np.append(Uw[i], sw["T_end"][i])) for i in range(N))
            out[case] = {"reactors": N, "tf": tf, **res,
                         "ratio_group_over_wave": res["group"]["reactors_per_s"] / res["wave"]["reactors_per_s"],
                         "worst_close_states_rtol_1e-4": worst}
            eng.close()
    os.environ.pop("BRHIP_ENGINE", None)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
