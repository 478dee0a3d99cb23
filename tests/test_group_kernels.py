"""The group engines' device code (k_group<GL, NM>, brhip_group.hpp) against references, kernel by
kernel: g_init_tconst / g_rhs / g_jac_cols through br_debug_group_eval against the oracle's rhs and
jac, g_pivot / g_lu / g_solve through br_debug_group_lu_solve against numpy, on all four built
instances, and whole integrations of group-eligible mechanisms WITH falloff reactions (Lindemann,
Troe with 3 and 4 parameters, irreversible reactions, gas + surface chemistry in one group engine).

The falloff mechanisms are subsets of GRI-Mech 3.0 written at test time (subset_mechanism): the
reactions of tests/golden/lib/grimech.dat whose species all lie in a given list.
"""

import os
import re
import shutil

import numpy as np
import pytest

from conftest import LIB
from test_gpu_parity import TH, _h2o2_with_inerts, _small_surface_mech, _states, close_states

pytestmark = pytest.mark.gpu

S16 = "H2 H O O2 OH H2O HO2 H2O2 CO CO2 HCO CH2O CH3 CH4 N2 AR".split()
S24 = S16 + "CH2 CH2(S) CH2OH CH3O CH3OH C2H4 C2H5 C2H6".split()
S32 = S16 + "C CH CH2 CH2(S) CH2OH CH3O CH3OH C2H C2H2 C2H3 C2H4 C2H5 C2H6 HCCO CH2CO HCCOH".split()
S12 = "H2 H O O2 OH H2O HO2 H2O2 CO CO2 CH4 N2".split()
SUBSETS = {"s16": (S16, None), "s24": (S24, None), "s32": (S32, None), "s12+ch4ni": (S12, "ch4ni.xml")}


def _equation_species(eq):
    """species names of a CHEMKIN reaction equation (stoichiometric coefficients and M dropped)"""
    eq = eq.replace("(+M)", "")
    out = []
    for side in re.split(r"<=>|=>|=", eq):
        for term in side.split("+"):
            name = re.sub(r"^\d+", "", term.strip())
            if name and name != "M":
                out.append(name)
    return out


def subset_mechanism(tmp_path, species, troe3=False, surface=None, name="sub"):
    """Write <tmp_path>/<name>/mech.dat: the species block `species` and every reaction of GRI-Mech 3.0
    (tests/golden/lib/grimech.dat) whose species all lie in it, with its LOW / TROE / DUPLICATE lines
    and its efficiency lines filtered down to `species`; therm.dat (and the surface mechanism file
    `surface`) copied alongside. troe3: drop the fourth TROE number of the first Troe reaction.
    Returns the directory."""
    keep = set(species)
    lines = open(os.path.join(LIB, "grimech.dat"), encoding="latin-1").read().split("\n")
    start = next(i for i, ln in enumerate(lines) if ln.strip().upper().startswith("REACTIONS"))
    out = ["ELEMENTS", "O  H  C  N  AR", "END", "SPECIES"]
    out += [" ".join(species[i:i + 8]) for i in range(0, len(species), 8)]
    out += ["END", lines[start]]
    taking, cut = False, troe3
    for ln in lines[start + 1:]:
        body = ln.split("!", 1)[0].strip()
        if not body:
            continue
        if body.upper() == "END":
            break
        if "=" in body:                                       # a reaction line
            taking = all(s in keep for s in _equation_species("".join(body.split()[:-3])))
            if taking:
                out.append(ln)
            continue
        if not taking:
            continue
        up = body.upper()
        if up.startswith("DUP") or up.startswith("LOW"):
            out.append(ln)
        elif up.startswith("TROE"):
            if cut:
                nums = up.split("/")[1].split()
                assert len(nums) == 4, ln
                ln = "     TROE/ " + "  ".join(nums[:3]) + " /"
                cut = False
            out.append(ln)
        else:                                                 # efficiencies: NAME/ value/ ...
            parts = [p.strip() for p in body.split("/")]
            pairs = [(parts[i], parts[i + 1]) for i in range(0, len(parts) - 1, 2) if parts[i]]
            pairs = [(k, v) for k, v in pairs if k in keep]
            if pairs:
                out.append(" ".join(f"{k}/{v}/" for k, v in pairs))
    out.append("END")
    d = tmp_path / name
    d.mkdir()
    (d / "mech.dat").write_text("\n".join(out) + "\n")
    shutil.copy(TH, d / "therm.dat")
    if surface:
        shutil.copy(os.path.join(LIB, surface), d / surface)
    return str(d)


def subset_pair(pkg, orc, tmp_path, key, conv=None, troe3=True):
    """product and oracle mechanisms of a SUBSETS entry"""
    species, surf = SUBSETS[key]
    conv = orc.CONV_REFERENCE if conv is None else conv
    d = subset_mechanism(tmp_path, species, troe3=troe3, surface=surf, name=key.replace("+", "_"))
    pm = pkg.Mechanism.from_files(d, gas_mech="mech.dat", surface_mech=surf, conv=conv)
    om = orc.Mech(os.path.join(d, "mech.dat"), os.path.join(d, "therm.dat"), os.path.join(d, surf) if surf else None,
                  conv=conv)
    return pm, om


# ---------------------------------------------------------------------------------------------
# a. g_init_tconst + g_rhs + g_jac_cols against the oracle
# ---------------------------------------------------------------------------------------------
def _eval_mechs(pkg, orc, tmp_path, mech, conv):
    """(pm, om, engine name, kernel name) of a case of test_group_rhs_jacobian_parity"""
    if mech in SUBSETS:
        pm, om = subset_pair(pkg, orc, tmp_path, mech, conv)
        return pm, om, {"s16": ("quad", "k_group<16, 16>"), "s24": ("pair", "k_group<32, 24>"),
                        "s32": ("pair", "k_group<32, 32>"), "s12+ch4ni": ("pair", "k_group<32, 32>")}[mech]
    if mech == "h2o2":
        pm = pkg.Mechanism.from_files(LIB, gas_mech="h2o2.dat", conv=conv)
        om = orc.Mech(os.path.join(LIB, "h2o2.dat"), TH, None, conv=conv)
        return pm, om, ("quad", "k_group<16, 9>")
    if mech in ("h2o2_n16", "h2o2_n17"):
        n = int(mech[-2:])
        d = _h2o2_with_inerts(tmp_path, n)
        pm = pkg.Mechanism.from_files(d, gas_mech="mech.dat", conv=conv)
        om = orc.Mech(os.path.join(d, "mech.dat"), os.path.join(d, "therm.dat"), None, conv=conv)
        return pm, om, (("quad", "k_group<16, 16>") if n == 16 else ("pair", "k_group<32, 24>"))
    if mech == "ni_small":
        pm, om = _small_surface_mech(pkg, orc, tmp_path)
        pm = pkg.Mechanism.from_files(str(tmp_path / "smallsurf"), surface_mech="h2coni.xml",
                                      gasphase=pm.gas_species, conv=conv)
        om.set_conv(conv)
        return pm, om, ("quad", "k_group<16, 16>")
    assert mech == "ch4ni"
    gas = ["CH4", "H2O", "H2", "CO", "CO2", "O2", "N2"]
    pm = pkg.Mechanism.from_files(LIB, surface_mech="ch4ni.xml", gasphase=gas, conv=conv)
    om = orc.Mech(None, TH, os.path.join(LIB, "ch4ni.xml"), gas_species=gas, conv=conv)
    return pm, om, ("pair", "k_group<32, 24>")


def _wide_states(pm, N, seed):
    """states as test_gpu_parity._states builds them (compositions, coverages), T in 700-2000 K (both
    NASA ranges, both sides of the Troe exponentials), p log-uniform in 1e3-1e7 Pa (falloff reactions on
    both sides of Pr = 1), Asv in [1, 100], small negative entries in the second half"""
    _, _, x, th = _states(pm, N, seed)
    rng = np.random.default_rng(1000 + seed)
    T = rng.uniform(700.0, 2000.0, N)
    p = np.exp(rng.uniform(np.log(1e3), np.log(1e7), N))
    Asv = np.exp(rng.uniform(0, np.log(100), N))
    U = np.stack([pm.initial_state(T[i], p[i], x[i], th[i] if pm.ns else None) for i in range(N)])
    neg = rng.random(U.shape) < 0.15
    U[N // 2:] = np.where(neg[N // 2:], -1e-3 * np.abs(U[N // 2:]), U[N // 2:])
    return T, Asv, U


_EVAL_CASES = [(m, c) for m in ("h2o2", "h2o2_n16", "ni_small", "s16", "h2o2_n17", "ch4ni", "s24", "s32", "s12+ch4ni")
               for c in (0, 19, 23) if c != 23 or m in ("ni_small", "ch4ni", "s12+ch4ni")]


@pytest.mark.parametrize("mech,conv", _EVAL_CASES, ids=[f"{m}-conv{c}" for m, c in _EVAL_CASES])
def test_group_rhs_jacobian_parity(pkg, orc, gpu, monkeypatch, tmp_path, mech, conv):
    """The group engines' own RHS and analytic Jacobian (g_init_tconst, g_rhs, g_jac_cols, evaluated by
    br_debug_group_eval in k_group's LDS blocks and global slots, each group several reactors in turn)
    against the oracle's rhs / jac at the bars of test_rhs_and_jacobian_parity: |du - do| <= 1e-11
    (max_j |Jo_kj| max|u| + |do|), row-wise |J - Jo| / max_j |Jo_kj| < 1e-11. conv 0 (textbook), 19
    (reference) and, with surface species, 23 (reference + documented coverage equation: Asv_th = 1).
    37 states: not a multiple of the groups per workgroup and more than the groups of the check's grid;
    one state has the reactants of a falloff reaction at exactly 0."""
    assert (orc.CONV_REFERENCE, orc.CONV_REFERENCE | orc.CONV_DOC_COVG) == (19, 23)
    pm, om, (engine, kernel) = _eval_mechs(pkg, orc, tmp_path, mech, conv)
    monkeypatch.setenv("BRHIP_ENGINE", engine)
    eng = pkg.Engine(pm)
    assert eng.engine == engine and eng.kernel_name == kernel, (eng.engine, eng.kernel_name)
    N = 37
    t = pm.tables
    fo = np.flatnonzero(t["g_tb"] == 2) if pm.nrg else np.zeros(0, int)
    T, Asv, U = _wide_states(pm, N, 31)
    ref = [None] * N
    for i in range(N):
        for k in range(20):   # a state the oracle cannot evaluate is replaced (another seed), not masked
            if k:
                Tk, Ak, Uk = _wide_states(pm, N, 31 + 97 * k)
                T[i], Asv[i], U[i] = Tk[i], Ak[i], Uk[i]
            if i == 5 and len(fo):
                U[i, t["g_f"][fo[0], :t["g_nf"][fo[0]]]] = 0.0
            do, _, _ = om.rhs(T[i], Asv[i], U[i])
            Jo = om.jac(T[i], Asv[i], U[i])
            if np.all(np.isfinite(do)) and np.all(np.isfinite(Jo)):
                ref[i] = (do, Jo)
                break
        assert ref[i] is not None, i
    assert T.min() < 1000.0 < T.max()
    du, J = eng.group_eval(T, Asv, U)
    e_du = e_j = 0.0
    for i in range(N):
        do, Jo = ref[i]
        scale = np.abs(Jo).max(1) * np.abs(U[i]).max() + np.abs(do) + 1e-300
        e_du = max(e_du, float(np.max(np.abs(du[i] - do) / scale)))
        js = np.abs(Jo).max(1, keepdims=True) + 1e-300
        e_j = max(e_j, float(np.max(np.abs(J[i] - Jo) / js)))
    print(f"group_eval {mech} conv {conv}: worst du {e_du / 1e-11:.3g}, worst J {e_j / 1e-11:.3g} (units of the 1e-11 bar)")
    for i in range(N):
        do, Jo = ref[i]
        scale = np.abs(Jo).max(1) * np.abs(U[i]).max() + np.abs(do) + 1e-300
        assert np.all(np.abs(du[i] - do) <= 1e-11 * scale), (mech, conv, i)
        js = np.abs(Jo).max(1, keepdims=True) + 1e-300
        assert np.max(np.abs(J[i] - Jo) / js) < 1e-11, (mech, conv, i)


def test_group_eval_needs_a_group_instance(pkg, gpu):
    """br_debug_group_eval on a mechanism without a group instance (GRI, n = 53): BR_ERR_UNSUPPORTED"""
    pm = pkg.Mechanism.from_files(LIB, gas_mech="grimech.dat")
    eng = pkg.Engine(pm)
    z = np.zeros((1, pm.n))
    one = np.ones(1)
    L = pkg._lib
    rc = L.lib().br_debug_group_eval(eng.h, 1, L.dptr(one), L.dptr(one), L.dptr(z), L.dptr(z.copy()),
                                     L.dptr(np.zeros((1, pm.n, pm.n))))
    assert rc == -30


# ---------------------------------------------------------------------------------------------
# b, c. g_pivot + g_lu + g_solve against numpy
# ---------------------------------------------------------------------------------------------
def _getrf_order(A):
    """pivot order of SUNDIALS denseGETRF in float64: at step k the first row of largest |a_ik| among
    the (already interchanged) rows k..n-1; returns orig, orig[s] = the original row at position s"""
    A = A.copy()
    n = A.shape[0]
    orig = np.arange(n)
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))   # (argmax: the first of equal maxima)
        if p != k:
            A[[k, p]] = A[[p, k]]
            orig[[k, p]] = orig[[p, k]]
        if A[k, k] == 0.0:
            break
        A[k + 1:, k] /= A[k, k]
        A[k + 1:, k + 1:] -= np.outer(A[k + 1:, k], A[k, k + 1:])
    return orig


def _group_lu(pkg, gl, nm, J, g, b):
    import ctypes as C
    N, n = b.shape
    x = np.zeros((N, n))
    f = np.full(N, -1, np.int32)
    perm = np.full((N, n), -1, np.int32)
    L = pkg._lib
    ip = C.POINTER(C.c_int)
    rc = L.lib().br_debug_group_lu_solve(gl, nm, N, n, L.dptr(J), L.dptr(g), L.dptr(b), L.dptr(x),
                                         f.ctypes.data_as(ip), perm.ctypes.data_as(ip))
    assert rc == 0, L.lib().br_last_error()
    return x, f, perm


def _lu_inputs(n, N, seed):
    """the ill-scaled Newton matrices of test_batched_lu_solve"""
    rng = np.random.default_rng(seed)
    J = rng.standard_normal((N, n, n)) * np.exp(rng.uniform(-8, 8, (N, n, 1)))
    g = np.exp(rng.uniform(-12, -2, N))
    b = rng.standard_normal((N, n))
    return J, g, b


def _backward_ok(J, g, b, x, i):
    n = b.shape[1]
    A = np.eye(n) - g[i] * J[i]
    res = A @ x[i] - b[i]
    return np.max(np.abs(res)) <= 1e-12 * (np.abs(A).sum(1).max() * np.abs(x[i]).max() + np.abs(b[i]).max())


_LU_CASES = [(16, 9, 1), (16, 9, 5), (16, 9, 9), (16, 16, 10), (16, 16, 16), (32, 24, 17), (32, 24, 20), (32, 24, 24),
             (32, 32, 25), (32, 32, 32)]


@pytest.mark.parametrize("gl,nm,n", _LU_CASES)
def test_group_lu_solve(pkg, gpu, gl, nm, n):
    """The group engines' register-resident LU and solve (g_pivot, g_lu, g_solve: DPP row broadcasts, the
    permlane16 swap of 32-lane groups, bpermute row interchanges, the three-round pivot search) on the
    matrices of test_batched_lu_solve: 1e-12 backward error, and the row order must be denseGETRF's (the
    first row of largest |a_ik|). Planted in column 0 of I - gamma J (gamma a power of two, so the
    planted values are exact; the rest continuous random): +v / -v ties (the lower row wins, either
    sign order), values that differ in the low word only (v, v (1 + 2^-40), v (1 + 2^-40): the middle row
    wins), and a column of one magnitude (no interchange) next to matrices that interchange."""
    N = 67   # not a multiple of the groups per wave: the last wave is partly idle
    J, g, b = _lu_inputs(n, N, 100 * nm + n)
    planted = {}
    if n >= 5:
        r1, r2, r3 = 1, n // 2 + 1, n - 1
        assert r1 < r2 < r3
        J[12, 0, 0], J[12, 2, 0] = 0.0, 3.0 / g[12]   # |a_20| = 3 > a_00 = 1: the wave mate of 13 interchanges
        for i, kind in ((8, "pm"), (9, "mp"), (10, "low"), (13, "flat"), (66, "low"), (65, "pm")):
            g[i] = 2.0 ** np.round(np.log2(g[i]))
            big = np.ldexp(1.25, int(np.ceil(np.log2(4 * np.abs(J[i, :, 0]).max() + 4 / g[i]))))   # > every |a_i0|
            if kind == "pm":
                J[i, r1, 0], J[i, r2, 0] = -big, big        # a = +v, -v
            elif kind == "mp":
                J[i, r1, 0], J[i, r2, 0] = big, -big        # a = -v, +v
            elif kind == "low":
                J[i, r1, 0], J[i, r2, 0], J[i, r3, 0] = big, -big * (1 + 2.0 ** -40), big * (1 + 2.0 ** -40)
            else:
                J[i, :, 0] = np.where(np.arange(n) % 2, 1.0, -1.0) / g[i]   # a_i0 = -1, +1, ...
                J[i, 0, 0] = 0.0                                            # a_00 = 1
            planted[i] = {"pm": r1, "mp": r1, "low": r2, "flat": 0}[kind]
            a0 = np.abs((np.arange(n) == 0) - g[i] * J[i, :, 0])      # |column 0| of I - gamma J, exact
            assert int(np.argmax(a0)) == planted[i]                  # (argmax: the first of the largest)
            assert np.sum(a0 == a0.max()) == (n if kind == "flat" else 2)
            if kind == "low":
                assert a0[r1] < a0[r2] and a0[r1].view(np.uint64) >> 32 == a0[r2].view(np.uint64) >> 32
    x, f, perm = _group_lu(pkg, gl, nm, J, g, b)
    assert np.all(f == 0)
    for i in range(N):
        assert _backward_ok(J, g, b, x, i), i
        assert sorted(perm[i]) == list(range(n)), (i, perm[i])
        assert np.array_equal(perm[i], _getrf_order(np.eye(n) - g[i] * J[i])), (i, planted.get(i))
        if i in planted:
            assert perm[i][0] == planted[i], (i, perm[i])
    if n >= 5:   # the flat column sits in one wave with matrices that interchanged at step 0
        assert 12 // (64 // gl) == 13 // (64 // gl)
        assert perm[13][0] == 0 and perm[12][0] != 0


@pytest.mark.parametrize("gl,nm,n", _LU_CASES)
def test_group_lu_zero_pivot_flag(pkg, gpu, gl, nm, n):
    """g_lu's zero-pivot flag: column k of I - gamma J exactly zero (gamma = 0.5, J[:, k] = 2 e_k) for
    k = 0, n // 2, n - 1 gives fail = k + 1; the non-singular matrices sharing the waves are unaffected
    (fail = 0, 1e-12 backward error)."""
    N = 67
    J, g, b = _lu_inputs(n, N, 200 * nm + n)
    ks = sorted({0, n // 2, n - 1})
    sing = {}
    for c, i in enumerate(range(1, N, 3)):
        k = ks[c % len(ks)]
        g[i] = 0.5
        J[i, :, k] = 0.0
        J[i, k, k] = 2.0
        assert not np.any((np.eye(n) - g[i] * J[i])[:, k])
        sing[i] = k
    x, f, perm = _group_lu(pkg, gl, nm, J, g, b)
    for i in range(N):
        if i in sing:
            assert f[i] == sing[i] + 1, (i, f[i], sing[i])
        else:
            assert f[i] == 0 and _backward_ok(J, g, b, x, i), (i, f[i])


def test_group_lu_solve_rejects_other_instances(pkg, gpu):
    """(gl, nm) other than the four built instances, or n > nm: BR_ERR_INPUT"""
    import ctypes as C
    L = pkg._lib
    ip = C.POINTER(C.c_int)
    for gl, nm, n in ((16, 12, 4), (32, 16, 4), (8, 8, 4), (16, 9, 10), (32, 24, 25), (32, 32, 33), (16, 16, 0)):
        m = max(n, 1)
        z = np.zeros((1, m, m))
        v = np.zeros((1, m))
        f = np.zeros(1, np.int32)
        p = np.zeros((1, m), np.int32)
        rc = L.lib().br_debug_group_lu_solve(gl, nm, 1, n, L.dptr(z), L.dptr(np.ones(1)), L.dptr(v), L.dptr(v.copy()),
                                             f.ctypes.data_as(ip), p.ctypes.data_as(ip))
        assert rc == -10, (gl, nm, n, rc)


# ---------------------------------------------------------------------------------------------
# d. integrations of the falloff mechanisms on the group engines
# ---------------------------------------------------------------------------------------------
def ignition_mixtures(pm, N, seed, Tlo=1300.0):
    """N CH4/O2/N2 mixtures, phi in [0.6, 1.4], T in [Tlo, 1500] K, p in [1, 5] bar; Asv = 1, or in
    [1, 100] per reactor with surface species"""
    rng = np.random.default_rng(seed)
    T = rng.uniform(Tlo, 1500.0, N)
    p = rng.uniform(1e5, 5e5, N)
    phi = rng.uniform(0.6, 1.4, N)
    X = np.zeros((N, pm.ng))
    xo2 = 0.4
    X[:, pm.gas_species.index("O2")] = xo2
    X[:, pm.gas_species.index("CH4")] = phi * xo2 / 2.0
    X[:, pm.gas_species.index("N2")] = 1.0 - xo2 - phi * xo2 / 2.0
    U0 = np.stack([pm.initial_state(T[i], p[i], X[i]) for i in range(N)])
    Asv = np.exp(rng.uniform(0, np.log(100), N)) if pm.ns else np.ones(N)
    return T, Asv, U0


@pytest.mark.parametrize("key,engine,kernel", [("s16", "quad", "k_group<16, 16>"), ("s24", "pair", "k_group<32, 24>"),
                                               ("s32", "pair", "k_group<32, 32>"), ("s12+ch4ni", "pair", "k_group<32, 32>")],
                         ids=["s16-quad", "s24-pair", "s32-pair", "s12+ch4ni-pair"])
def test_group_engine_falloff_integration(pkg, orc, gpu, monkeypatch, tmp_path, key, engine, kernel):
    """The group engines on mechanisms with falloff reactions (GRI-Mech subsets of 16 / 24 / 32 species;
    12 gas species + the Ni surface mechanism), igniting CH4/O2/N2 mixtures, pattern and bars of
    test_group_engine_register_widths: end states at rtol 1e-10 / atol 1e-16 against the oracle to 1e-6
    relative (floor 1e-14) with the analytic and the DQ Jacobian on both sides, n RHS per DQ Jacobian,
    ignition times within two ignition steps at default tolerances, the wavefront engine's end states."""
    pm, om = subset_pair(pkg, orc, tmp_path, key)
    monkeypatch.setenv("BRHIP_ENGINE", engine)
    eng = pkg.Engine(pm)
    assert eng.engine == engine and eng.kernel_name == kernel, eng.kernel_name
    N, tf = 32, 1e-2
    # (the 12-species list has CH4 but no CH3: CH4 reacts on the surface only, the radical pool grows
    # from the surface products, and below ~1440 K d X_OH / dt is still rising at tf)
    T, Asv, U0 = ignition_mixtures(pm, N, 5, Tlo=1450.0 if pm.ns else 1300.0)
    Ug = None
    for dq in (False, True):
        U, st = eng.integrate(T, Asv, U0, tf, rtol=1e-10, atol=1e-16, dq_jacobian=dq)
        assert np.all(st["status"] == 0), (dq, np.unique(st["status"]))
        if dq:
            assert np.all(st["nfe_dq"] == st["nje"] * pm.n)
        else:
            Ug = U
        Uo, so, bad = om.integrate_batch(T, Asv, U0, tf, rtol=1e-10, atol=1e-16, analytic_jac=not dq)
        assert bad == 0 and all(s["status"] == 0 for s in so)
        assert all(s["t_ign"] < tf for s in so), [s["t_ign"] for s in so]
        for i in range(N):
            assert close_states(U[i], Uo[i], rtol=1e-6, floor=1e-14) <= 1.0, (dq, i)
    U, st = eng.integrate(T, Asv, U0, tf)
    _, so, bad = om.integrate_batch(T, Asv, U0, tf, analytic_jac=True)
    assert bad == 0
    for i in range(N):
        assert so[i]["t_ign"] < tf, (i, so[i]["t_ign"])
        assert abs(st["t_ign"][i] - so[i]["t_ign"]) <= 2 * max(st["ign_dt"][i], so[i]["ign_dt"]) + 1e-4 * so[i]["t_ign"], i
    monkeypatch.setenv("BRHIP_ENGINE", "wave")
    Uw, sw = eng.integrate(T, Asv, U0, tf, rtol=1e-10, atol=1e-16)
    assert np.all(sw["status"] == 0)
    assert max(close_states(Ug[i], Uw[i], rtol=1e-6, floor=1e-14) for i in range(N)) <= 1.0
