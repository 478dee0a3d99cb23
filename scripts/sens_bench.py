#!/usr/bin/env python3
"""Throughput of br_sensitivity: GRI-Mech (64 base reactors x all 325 reactions) and H2/O2 (4096 x 18),
the first reactors of the bench configs C3 / C2 at their tf.

Reports, per mechanism, one JSON line with
  expanded_reactors_per_s   N (2 nsel + 1) / kernel time (br_last_kernel_ms: the integrator launch alone;
                            both ensembles fit one chunk, so it is the only launch)
  sensitivities_per_s       N nsel / wall time of the whole call (table, expansion, integration, reduction,
                            copies of S and the base results)
  plain_reactors_per_s      the same number of plain reactors of the config through Engine.integrate, kernel
                            time, in the same process, with steps/s next to both: perturbed reactors take
                            different step counts, so steps/s is the like-for-like figure
What is shown is that the table, the expansion and the reduction add little beyond the integrations.

  python3 scripts/sens_bench.py [--out profiles/sens_bench.json] [--repeat 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = (("gri", 64), ("h2o2", 4096))


def run(pkg, config, nbase, repeat):
    import bench
    from batchreactor_amd import ensemble
    mech = bench.make_mech(pkg, config)
    eng = pkg.Engine(mech, device=0)
    tf = bench.CONFIGS[config]["tf"]
    T, Asv, U0 = ensemble.make_inputs(mech, config, 0, nbase)
    nsel = eng.nr
    nexp = nbase * (2 * nsel + 1)
    best = None
    for it in range(repeat + 1):                         # (the first call also allocates: not kept)
        t0 = time.perf_counter()
        out = eng.sensitivity(T, Asv, U0, tf)
        wall = time.perf_counter() - t0
        ms = eng.last_kernel_ms()
        if it and (best is None or wall < best[0]):
            best = (wall, ms, out)
    wall, ms, out = best
    # the same count of plain reactors of the config (kernel time), and the expanded ensemble's own steps
    Tp, Ap, Up = ensemble.make_inputs(mech, config, 0, nexp)
    pms, pst = None, None
    for it in range(repeat + 1):
        _, pst = eng.integrate(Tp, Ap, Up, tf)
        m = eng.last_kernel_ms()
        if it and (pms is None or m < pms):
            pms = m
    rows = 2 * nsel + 1
    tab = np.ones((rows, nsel))
    for j in range(nsel):
        tab[1 + 2 * j, j], tab[2 + 2 * j, j] = 2.0, 0.5
    rep = lambda a: np.repeat(np.asarray(a), rows, axis=0)
    _, est = eng.integrate(rep(T), rep(Asv), rep(U0), tf, rate_mult=tab,
                           rate_mult_row=np.tile(np.arange(rows, dtype=np.int32), nbase))
    esteps, psteps = float(est["nsteps"].sum()), float(pst["nsteps"].sum())
    S = out["S_tign"]
    res = {"config": config, "kernel": eng.kernel_name, "base_reactors": nbase, "reactions": nsel,
           "expanded_reactors": nexp, "kernel_ms": ms, "wall_ms": 1e3 * wall,
           "expanded_reactors_per_s": nexp / (1e-3 * ms), "expanded_steps_per_s": esteps / (1e-3 * ms),
           "sensitivities_per_s": nbase * nsel / wall, "overhead_beyond_kernel_ms": 1e3 * wall - ms,
           "plain_reactors": nexp, "plain_kernel_ms": pms, "plain_reactors_per_s": nexp / (1e-3 * pms),
           "plain_steps_per_s": psteps / (1e-3 * pms), "nbad": out["nbad"],
           "largest_abs_S_tign": float(np.nanmax(np.abs(S))), "sum_S_tign_median": float(np.nanmedian(np.nansum(S, axis=1)))}
    eng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines to this file (a JSON list)")
    ap.add_argument("--repeat", type=int, default=3)
    a = ap.parse_args()
    import _pkgload
    pkg = _pkgload.load()
    lines = []
    for config, nbase in CASES:
        lines.append(run(pkg, config, nbase, a.repeat))
        print(json.dumps(lines[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
