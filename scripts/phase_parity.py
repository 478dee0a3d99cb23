"""Ignition-phase parity: the GPU against the oracle with both sampled at their OWN ignition phases,
t = tau * t_ign (per-reactor output grids, br_opts.tout_per_reactor / br_integrate_phase), so that a
difference in the front's timing does not show up as an amplitude difference at a fixed t (VERDICT r06
"Next round" 1(a)). Writes profiles/phase_parity.json; no bound of tests/parity_bands.py is changed
here, the file is the evidence for re-deriving them.

  python3 scripts/phase_parity.py [--configs gri,gas_surf,h2o2,surf] [--sample 256] [--out PATH] [--threads T]
  python3 scripts/phase_parity.py --converged-front-only     (CPU only: the oracle against itself)

Per bench config and Jacobian kind (analytic, and CVODE's DQ Jacobian), on the first `sample` reactors of
the bench workload (ensemble.make_inputs), default tolerances (rtol 1e-6, atol 1e-10), tf of the config:

1. GPU: Engine.integrate_phase at TAU (two passes on the device: t_ign, then the states at TAU * t_ign).
2. oracle: the same two passes, per reactor (integrate_batch for t_ign, integrate_out at TAU * its own
   t_ign).
3. per phase, the band error of parity_bands.band_errors' metric between the two,
   max_k |Y_gpu - Y_orc| / (1e-4 |Y_orc| + 100 atol), summarised over the reactors; the relative t_ign
   difference; and ign_dt / t_ign of both sides per reactor -- t_ign is the midpoint of the steepest
   accepted step, so it is resolved to ign_dt only: a phase error of that size is a one-step shift of
   the marker, not a difference of the front.
4. the oracle's own spread in the same metric, with the project's realisations (parity_outliers.py): u0
   times 1 +- 1e-15 (R_U0 runs) and every rate of progress times 1 +- eps_cal (R_J runs), eps_cal from
   profiles/r06_parity_outliers.json; every realisation sampled at its own phases against the
   unperturbed oracle at its own.
A config without the ignition marker species (surface-only) has no t_ign and is recorded as skipped.

"converged_front": for tests/test_per_reactor_output.py::test_converged_front_against_oracle -- the
oracle at rtol 1e-10 / atol 1e-16 against the oracle at rtol 1e-11 / atol 1e-17 at the same times
(TAU * the first one's t_ign) on that test's 16 reactors, close_states(rtol 1e-6, floor 1e-14) per phase;
the test's front bound is 4 x the maximum over the front phases (two sides each carry that convergence
error, times the margin of 2 of parity_bands.py). CPU only: never derived from a GPU run.
The oracle is the checker here (test infrastructure), as in bench.py's cpu_baseline leg.
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import _pkgload  # noqa: E402
import oracle as orc  # noqa: E402
import parity_bands as PB  # noqa: E402
import bench  # noqa: E402

LIB = os.path.join(ROOT, "tests", "golden", "lib")
TAU = (0.5, 0.8, 0.9, 0.95, 1.0, 1.05, 1.1, 1.5, 2.0, 10.0)
FRONT = tuple(0.8 < t < 2.0 for t in TAU)          # the phases that carry the measured front bound
R_U0, R_J = 2, 4
CONVERGED_CASES = {"gri": "grimech.dat", "h2o2": "h2o2.dat"}
CONVERGED_N, CONVERGED_SEED, CONVERGED_TF = 16, 6, 1e-2


def oracle_mech(pkg, config):
    cfg = bench.CONFIGS[config]
    mech = bench.make_mech(pkg, config)
    om = orc.Mech(os.path.join(LIB, cfg["gas"]) if cfg["gas"] else None, os.path.join(LIB, "therm.dat"),
                  os.path.join(LIB, cfg["surf"]) if cfg["surf"] else None,
                  gas_species=None if cfg["gas"] else mech.gas_species)
    return mech, om


def oracle_at(om, T, A, U0, tf, grid, aj, thr, rtol=1e-6, atol=1e-10):
    """the oracle's states at the per-reactor grid (NaN entries: no output, rows of NaN)"""
    N, nt = grid.shape
    Y = np.full((N, nt, om.n), np.nan)

    def one(i):
        sel = np.isfinite(grid[i])
        if sel.any():
            _, so, Yi = om.integrate_out(T[i], A[i], U0[i], tf[i], grid[i][sel], rtol=rtol, atol=atol, analytic_jac=aj)
            if so["status"] == 0:
                Y[i, sel] = Yi

    with ThreadPoolExecutor(max(1, thr)) as ex:
        list(ex.map(one, range(N)))
    return Y


def oracle_phase(pkg, om, T, A, U0, tf, aj, thr, jitter=0.0, seed=0, rtol=1e-6, atol=1e-10):
    """the oracle's two passes: t_ign, then the states at TAU * t_ign"""
    L = orc.lib()
    L.orc_set_rop_jitter(jitter)
    L.orc_set_rop_jitter_seed(seed)
    try:
        _, st, _ = om.integrate_batch(T, A, U0, tf, rtol=rtol, atol=atol, analytic_jac=aj, nthreads=thr)
        d = {k: np.array([s[k] for s in st], dtype=float) for k in ("status", "t_ign", "ign_dt", "nsteps")}
        d["t_ign"] = np.where(d["status"] == 0, d["t_ign"], np.nan)
        grid = pkg.phase_grid(d["t_ign"], TAU, tf)
        Y = oracle_at(om, T, A, U0, tf, grid, aj, thr, rtol, atol)
    finally:
        L.orc_set_rop_jitter(0.0)
        L.orc_set_rop_jitter_seed(0)
    return d, grid, Y


def bands(Ya, Yb):
    """[N, ntau] band errors of Ya against Yb (parity_bands.band_errors' metric); NaN where either has no output"""
    return (np.abs(Ya - Yb) / (1e-4 * np.abs(Yb) + 100 * PB.ATOL)).max(axis=2)


def per_phase(W):
    out = []
    for j, tau in enumerate(TAU):
        w = W[:, j][np.isfinite(W[:, j])]
        out.append({"tau": tau, "reactors": int(len(w)),
                    "max": float(w.max()) if len(w) else None,
                    "p99": float(np.percentile(w, 99)) if len(w) else None,
                    "median": float(np.median(w)) if len(w) else None})
    return out


class OracleAsGpu:
    """--cpu-dry-run: stands in for the engine with a jittered oracle (seed 999), to check this script's
    logic on a machine without a GPU; its numbers mean nothing"""
    def __init__(self, pkg, om, thr):
        self.pkg, self.om, self.thr = pkg, om, thr
        self.ign1 = om.ign1

    def integrate_phase(self, T, A, U0, tf, tau, rtol=1e-6, atol=1e-10, dq_jacobian=False):
        d, grid, Y = oracle_phase(self.pkg, self.om, T, A, U0, tf, not dq_jacobian, self.thr, jitter=1e-15, seed=999,
                                  rtol=rtol, atol=atol)
        d["tout"], d["yout"] = grid, np.nan_to_num(Y)
        return None, d

    def close(self):
        pass


def analyse(pkg, eng, mech, om, config, aj, K, thr, eps_cal, log):
    T, A, U0 = bench.ensemble_inputs(pkg, mech, config, K)
    tf = np.full(K, bench.CONFIGS[config]["tf"])
    t0 = time.time()
    _, sg = eng.integrate_phase(T, A, U0, tf, TAU, dq_jacobian=not aj)
    so, grid_o, Yo = oracle_phase(pkg, om, T, A, U0, tf, aj, thr)
    ok = (sg["status"] == 0) & (so["status"] == 0)
    Yg = np.where(np.isfinite(sg["tout"])[:, :, None], sg["yout"], np.nan)
    Wg = bands(Yg, Yo)
    Wg[~ok] = np.nan
    log(f"  {config} {'analytic' if aj else 'DQ'}: K={K} GPU max per phase {np.round(np.nanmax(Wg, 0), 3)} "
        f"({time.time() - t0:.1f} s)")
    series = []
    rng = np.random.default_rng(20250711)
    for r in range(R_U0):
        Up = U0 * (1 + 1e-15 * rng.standard_normal(U0.shape))
        sr, _, Yr = oracle_phase(pkg, om, T, A, Up, tf, aj, thr)
        W = bands(Yr, Yo)
        W[(sr["status"] != 0) | (so["status"] != 0)] = np.nan
        series.append(W)
        log(f"    self-spread u0 #{r}: max per phase {np.round(np.nanmax(W, 0), 3)}")
    for r in range(R_J):
        sr, _, Yr = oracle_phase(pkg, om, T, A, U0, tf, aj, thr, jitter=eps_cal, seed=1 + r)
        W = bands(Yr, Yo)
        W[(sr["status"] != 0) | (so["status"] != 0)] = np.nan
        series.append(W)
        log(f"    self-spread jitter #{r}: max per phase {np.round(np.nanmax(W, 0), 3)}")
    with np.errstate(all="ignore"):
        Wself = np.nanmax(np.stack(series), axis=0) if series else np.full_like(Wg, np.nan)
        rel = np.abs(sg["t_ign"] - so["t_ign"]) / so["t_ign"]
        rg, ro = sg["ign_dt"] / sg["t_ign"], so["ign_dt"] / so["t_ign"]
    rel_ok = rel[ok & np.isfinite(rel)]

    def lst(a):   # (7 significant digits: these columns are for reading, the summaries use full precision)
        return [None if not np.isfinite(v) else float(f"{v:.7g}") for v in a]

    return {"jacobian": "analytic" if aj else "dq", "sample": int(K), "scored": int(ok.sum()),
            "failed_either": int((~ok).sum()),
            "realisations": {"u0_1e-15": R_U0, "rop_jitter_eps_cal": R_J}, "eps_cal": eps_cal,
            "gpu_vs_oracle": per_phase(Wg), "oracle_self_spread": per_phase(Wself),
            "t_ign_rel_diff": {"max": float(rel_ok.max()) if len(rel_ok) else None,
                               "p99": float(np.percentile(rel_ok, 99)) if len(rel_ok) else None,
                               "median": float(np.median(rel_ok)) if len(rel_ok) else None},
            "per_reactor": {"t_ign_gpu": lst(sg["t_ign"]), "t_ign_orc": lst(so["t_ign"]), "t_ign_rel_diff": lst(rel),
                            "ign_dt_over_t_ign_gpu": lst(rg), "ign_dt_over_t_ign_orc": lst(ro)}}


def converged_inputs(pm, case, N, seed):
    """the inputs of tests/test_gpu_parity.py's tight-tolerance tests (its _ignition_inputs, gas cases)"""
    # (a test module as a library: the helper lives only there, and the test this serves must use the
    # very same inputs; importing it needs pytest)
    from test_gpu_parity import _ignition_inputs
    return _ignition_inputs(pm, case, N, seed)


def converged_front(pkg, thr, log):
    """the oracle's own convergence error at the phases, rtol 1e-10 against rtol 1e-11 (see the module text)"""
    res = {"reactors": CONVERGED_N, "inputs": f"_ignition_inputs(case, {CONVERGED_N}, seed {CONVERGED_SEED}), tf {CONVERGED_TF}",
           "metric": "close_states(rtol 1e-6, floor 1e-14) of oracle(rtol 1e-10, atol 1e-16) against "
                     "oracle(rtol 1e-11, atol 1e-17) at tau * t_ign of the first",
           "rule": "front bound = 4 x raw_max (front phases: 0.8 < tau < 2)", "tau": list(TAU), "cases": {}}
    for case, gas in CONVERGED_CASES.items():
        pm = pkg.Mechanism.from_files(LIB, gas_mech=gas)
        om = orc.Mech(os.path.join(LIB, gas), os.path.join(LIB, "therm.dat"))
        T, A, U0 = converged_inputs(pm, case, CONVERGED_N, CONVERGED_SEED)
        tf = np.full(CONVERGED_N, CONVERGED_TF)
        res["cases"][case] = {}
        for aj in (True, False):
            sa, grid, Ya = oracle_phase(pkg, om, T, A, U0, tf, aj, thr, rtol=1e-10, atol=1e-16)
            Yb = oracle_at(om, T, A, U0, tf, grid, aj, thr, rtol=1e-11, atol=1e-17)
            assert np.all(sa["status"] == 0)
            E = (np.abs(Ya - Yb) / (1e-6 * np.abs(Yb) + 1e-14)).max(axis=2)          # [N, ntau]
            assert np.all(np.isfinite(E) == np.isfinite(grid))
            with np.errstate(all="ignore"):
                pm_ = np.nanmax(E, axis=0)
            raw = float(np.nanmax(E[:, np.array(FRONT)]))
            res["cases"][case]["analytic" if aj else "dq"] = {
                "per_phase_max": [None if not np.isfinite(v) else float(v) for v in pm_],
                "outputs_per_phase": np.isfinite(grid).sum(axis=0).tolist(), "raw_max": raw, "bound": 4 * raw}
            log(f"  converged front {case} {'analytic' if aj else 'DQ'}: raw max {raw:.4g} -> bound {4 * raw:.4g}; "
                f"per phase {np.round(pm_, 4)}")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="gri,gas_surf,h2o2,surf")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "phase_parity.json"))
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--sample", type=int, default=256)
    ap.add_argument("--calibration", default=os.path.join(ROOT, "profiles", "r06_parity_outliers.json"),
                    help="the analysis whose rhs_calibration.eps_cal sets the rop jitter of the self-spread runs")
    ap.add_argument("--converged-front-only", action="store_true", help="CPU only: the oracle against itself")
    ap.add_argument("--no-converged-front", action="store_true")
    ap.add_argument("--cpu-dry-run", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    pkg = _pkgload.load()
    if not os.path.exists(orc.LIB):
        orc.build()
    log = lambda s: print(s, flush=True)  # noqa: E731
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    res = {"metric": "per reactor and phase tau = t / t_ign (each side at its own t_ign): "
                     "max_k |Y_a - Y_b| / (1e-4 |Y_b| + 100 atol), the bands of tests/parity_bands.py",
           "tau": list(TAU), "rtol": 1e-6, "atol": 1e-10,
           "t_ign_resolution": "t_ign is the midpoint of the steepest accepted step: resolved to ign_dt "
                               "(per_reactor.ign_dt_over_t_ign_*)",
           "configs": {}}

    def dump():
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)

    if not args.converged_front_only:
        cal = json.load(open(args.calibration))["configs"]
        for config in args.configs.split(","):
            mech, om = oracle_mech(pkg, config)
            res["configs"][config] = {}
            if not om.ign1:
                res["configs"][config] = {"skipped": "no ignition marker species in the mechanism: no t_ign, no phases"}
                log(f"  {config}: skipped (no ignition marker)")
                dump()
                continue
            eng = OracleAsGpu(pkg, om, args.threads) if args.cpu_dry_run else pkg.Engine(mech)
            for aj in (True, False):
                jac = "analytic" if aj else "dq"
                eps = float(cal[config][jac]["rhs_calibration"]["eps_cal"])
                res["configs"][config][jac] = analyse(pkg, eng, mech, om, config, aj, args.sample, args.threads, eps, log)
                dump()
            eng.close()
    if not args.no_converged_front:
        res["converged_front"] = converged_front(pkg, args.threads, log)
    dump()
    print("wrote", args.out)


if __name__ == "__main__":
    main()
