"""Prescribed temperature programmes T(t) (br_opts.ntprog), the part that needs no GPU: the new br_opts
fields and their place, the host-side checks of a programme (they run before the handle is looked at),
TemperatureProgram against the header's formula, and the host CVODE's time argument: f sees the time
CVODE evaluates it at, and an RHS failure leaves the last accepted state."""
import ctypes as C

import numpy as np
import pytest

NEW = [("ntprog", C.c_int), ("tprog_t", "dp"), ("tprog_T", "dp"), ("ntprog_rows", C.c_int), ("tprog_row", "ip")]
BR_ERR_RHS, BR_ERR_INPUT, BR_ERR_UNSUPPORTED = -8, -10, -30


def _header_formula(kt, kT, t):
    """include/brhip.h, written out: T_j + (t - t_j) * ((T_{j+1} - T_j) / (t_{j+1} - t_j)) on t_j <= t < t_{j+1},
    the last knot's T at and beyond it; NaN knot times are trailing padding. One scalar at a time."""
    nk = sum(1 for x in kt if x == x)
    j = 0
    while j + 1 < nk and t >= kt[j + 1]:
        j += 1
    if j + 1 >= nk:
        return kT[j]
    return kT[j] + (t - kt[j]) * ((kT[j + 1] - kT[j]) / (kt[j + 1] - kt[j]))


def test_opts_fields_sit_between_yout_and_dq_jacobian(pkg):
    """the five fields follow yout; dq_jacobian .. tout_per_reactor stay the struct's tail in their order (the
    bindings' tests pin that tail), and every field up to yout keeps its offset"""
    L = pkg._lib
    names = [f[0] for f in L.Opts._fields_]
    k = names.index("ntprog")
    assert names[k - 1] == "yout" and names[k:k + 5] == [n for n, _ in NEW]
    assert names[k + 5:] == ["dq_jacobian", "nmult", "rate_mult", "rate_mult_row", "tout_per_reactor"]
    types = {"dp": L.dp, "ip": L.ip}
    assert [f[1] for f in L.Opts._fields_[k:k + 5]] == [types.get(t, t) for _, t in NEW]
    assert L.Opts.ntprog.offset == L.Opts.yout.offset + 8 and L.Opts.tprog_row.offset + 8 == L.Opts.dq_jacobian.offset
    import os, re
    from conftest import ROOT
    jl = re.sub(r"#[^\n]*", "", open(os.path.join(ROOT, "julia", "BatchReactorHIP.jl")).read())
    body = jl.split("\nstruct BrOpts")[1].split("\nend")[0]
    jnames = [f.split("::")[0].strip() for ln in body.split("\n") for f in ln.split(";") if "::" in f]
    assert jnames == names                                              # Julia mirrors the same order
    assert "with_tprog(o::BrOpts" in jl and "with_tprog" in jl.split("\nexport ")[1]
    assert L.lib().br_version() >= 220
    o = L.Opts()
    assert o.ntprog == 0 and not o.tprog_t and not o.tprog_T and o.ntprog_rows == 0 and not o.tprog_row
    assert "br_debug_tprog_eval" in L.EXPORTS


def _opts(pkg, kt, kT, rows=None):
    L = pkg._lib
    kt = np.ascontiguousarray(kt, np.float64)
    kT = np.ascontiguousarray(kT, np.float64)
    o = L.Opts(rtol=1e-6, atol=1e-10, max_steps=100)
    o.ntprog, o.ntprog_rows = kt.shape[1], kt.shape[0]
    o.tprog_t, o.tprog_T = L.dptr(kt), L.dptr(kT)
    keep = [kt, kT]
    if rows is not None:
        rows = np.ascontiguousarray(rows, np.int32)
        o.tprog_row = L.iptr(rows)
        keep.append(rows)
    return o, keep


def _integrate_no_handle(pkg, o, N):
    """br_integrate with a NULL handle: a programme is checked before the handle is looked at, so a bad one
    is named, and a good one gets as far as 'bad argument'. Nothing reaches a GPU."""
    L = pkg._lib
    u, tf = np.ones((N, 3)), np.ones(N)
    rc = L.lib().br_integrate(None, N, None, None, L.dptr(u), L.dptr(tf), C.byref(o), None)
    return rc, L.lib().br_last_error().decode()


GOOD_T = [[0.0, 1.0, 2.0]] * 4
GOOD_K = [[900.0, 1000.0, 950.0]] * 4


def _with(row, col, v, base):
    a = np.array(base, dtype=np.float64)
    a[row, col] = v
    return a


@pytest.mark.parametrize("name,kt,kT,rows,N,expect", [
    ("descending", _with(2, 2, 0.5, GOOD_T), GOOD_K, None, 4, ("reactor 2", "row 2", "ascending")),
    ("first knot", _with(1, 0, 0.1, GOOD_T), GOOD_K, None, 4, ("reactor 1", "row 1", "first knot")),
    ("interior NaN", _with(3, 1, np.nan, GOOD_T), GOOD_K, None, 4, ("reactor 3", "row 3", "NaN")),
    ("T zero", GOOD_T, _with(0, 1, 0.0, GOOD_K), None, 4, ("reactor 0", "row 0", "finite and > 0")),
    ("T negative", GOOD_T, _with(2, 0, -5.0, GOOD_K), None, 4, ("reactor 2", "row 2", "finite and > 0")),
    ("T inf", GOOD_T, _with(1, 2, np.inf, GOOD_K), None, 4, ("reactor 1", "row 1", "finite and > 0")),
    ("T NaN", GOOD_T, _with(1, 2, np.nan, GOOD_K), None, 4, ("reactor 1", "row 1", "finite and > 0")),
    # a shared table: the reactor named is the first one that uses the bad row
    ("shared bad row", _with(1, 2, 0.5, GOOD_T[:2]), GOOD_K[:2], [0, 0, 1, 1, 0], 5, ("reactor 2", "row 1", "ascending")),
    ("row index", GOOD_T[:2], GOOD_K[:2], [0, 1, 2, 0, 0], 5, ("tprog_row[2] = 2", "reactor 2")),
    ("row index < 0", GOOD_T[:2], GOOD_K[:2], [0, -1, 0, 0, 0], 5, ("tprog_row[1] = -1", "reactor 1")),
    ("NULL rows, nrows != N", GOOD_T, GOOD_K, None, 5, ("ntprog_rows must be N = 5",)),
])
def test_bad_programmes_are_refused_with_the_reactor_named(pkg, name, kt, kT, rows, N, expect):
    o, keep = _opts(pkg, kt, kT, rows)
    rc, msg = _integrate_no_handle(pkg, o, N)
    assert rc == BR_ERR_INPUT, (name, rc, msg)
    for e in expect:
        assert e in msg, (name, msg)


def test_a_good_programme_passes_the_checks(pkg):
    """... and the call then stops at the missing handle; trailing NaN padding and equal knot times (a
    jump) are fine, the temperature under a padding entry is not read"""
    kt = np.array([[0.0, 1.0, 1.0, 2.0], [0.0, 3.0, np.nan, np.nan]])
    kT = np.array([[900.0, 950.0, 1000.0, 1000.0], [800.0, 900.0, -1.0, np.nan]])
    o, keep = _opts(pkg, kt, kT, [0, 1, 1])
    rc, msg = _integrate_no_handle(pkg, o, 3)
    assert rc == BR_ERR_INPUT and msg == "bad argument", (rc, msg)


def test_sensitivity_with_a_programme_is_unsupported(pkg):
    """a host-side answer, before the handle or any launch"""
    L = pkg._lib
    o, keep = _opts(pkg, GOOD_T, GOOD_K)
    z = np.ones((4, 3))
    rc = L.lib().br_sensitivity(None, 4, L.dptr(z), None, L.dptr(z), L.dptr(z), C.byref(o), 2.0, 1, None, None, None,
                                None, None, None)
    assert rc == BR_ERR_UNSUPPORTED, (rc, L.lib().br_last_error())
    assert b"temperature programme" in L.lib().br_last_error()


def test_temperature_program_is_the_headers_formula(pkg):
    TP = pkg.TemperatureProgram
    p = TP.from_knots([0.0, 0.5, 0.5, 2.0, 7.0], [300.0, 400.0, 450.0, 1200.0, 1000.0])   # a jump at 0.5
    ts = np.concatenate([np.linspace(0.0, 9.0, 181), p.t, np.nextafter(p.t, np.inf), np.nextafter(p.t[1:], 0.0)])
    want = np.array([_header_formula(p.t, p.T, t) for t in ts])
    np.testing.assert_array_equal(p(ts), want)                          # the same three operations: the same bits
    assert p(0.0) == 300.0 and p(0.5) == 450.0 and p(2.0) == 1200.0      # on the knots: the knot's T (the later of a jump)
    assert p(7.0) == 1000.0 and p(1e9) == 1000.0                         # at and beyond the last knot: held
    assert isinstance(p(1.0), float)
    r = TP.ramp(300.0, 2.0, 900.0)                                       # 2 K/s up to 900 K
    assert r.t.tolist() == [0.0, 300.0] and r.T.tolist() == [300.0, 900.0]
    assert r(150.0) == 600.0 and r(1e4) == 900.0
    assert TP.ramp(900.0, -3.0, 300.0)(100.0) == 600.0                   # cooling
    assert TP.constant(1000.0)(5.0) == 1000.0
    with pytest.raises(ValueError, match="never reaches"):
        TP.ramp(300.0, -1.0, 900.0)
    for bad in (([0.1, 1.0], [1.0, 1.0]), ([0.0, 2.0, 1.0], [1.0, 1.0, 1.0]), ([0.0, 1.0], [1.0, 0.0]),
                ([0.0, np.nan, 1.0], [1.0, 1.0, 1.0]), ([0.0, 1.0], [1.0])):
        with pytest.raises(ValueError, match="tprog"):
            TP.from_knots(*bad)
    # ragged rows: the table pads with NaN times, and a padded row evaluates as the programme itself
    kt, kT, rows = pkg.tprog.table([p, r], [1, 0, 1], 3)
    assert kt.shape == (2, 5) and np.isnan(kt[1, 2:]).all() and rows.dtype == np.int32
    np.testing.assert_array_equal(pkg.tprog.evaluate(kt[1], kT[1], ts), r(ts))
    np.testing.assert_array_equal(pkg.tprog.evaluate(kt[0], kT[0], ts), want)
    kt1, _, rows1 = pkg.tprog.table(r, None, 4)                           # one programme: shared by all
    assert kt1.shape == (1, 2) and rows1.tolist() == [0, 0, 0, 0]
    for kw in (dict(tprog=[p, r], tprog_row=None), dict(tprog=[p, r], tprog_row=[0, 1]), dict(tprog=None, tprog_row=[0] * 3),
               dict(tprog=[p, r], tprog_row=[0.0, 1.0, 0.0]), dict(tprog=(np.zeros((2, 2)), np.ones((2, 3))), tprog_row=None)):
        with pytest.raises(ValueError, match="tprog"):
            pkg.tprog.table(kw["tprog"], kw["tprog_row"], 3)


def test_host_cvode_time_dependent_rhs_against_scipy(pkg):
    """u' = A u + g(t) problems whose right-hand side depends on t: integrate_host must hand f the time CVODE
    evaluates it at. Against SciPy's Radau at rtol 1e-10 and the closed form, to the tolerance of
    test_host_cvode_robertson_against_scipy (1e-4 relative + 1e-9)."""
    from scipy.integrate import solve_ivp
    L = pkg._lib
    w = 3.0

    def f1(t, y):                                     # u' = -u + sin(w t); stiff companion v' = -1e4 (v - cos t)
        return np.array([-y[0] + np.sin(w * t), -1e4 * (y[1] - np.cos(t))])

    def f2(t, y):                                     # a kinked forcing (a ramp that stops), as a programme has
        return np.array([-50.0 * (y[0] - min(t, 0.3)), y[0] - y[1]])
    for f, y0, tf in ((f1, [1.0, 1.0], 2.0), (f2, [0.0, 0.0], 1.0)):
        seen = []
        status, u, st = L.integrate_host(lambda t, y: (seen.append(t), f(t, y))[1], y0, tf)
        assert status == 0
        ref = solve_ivp(f, (0.0, tf), y0, method="Radau", rtol=1e-10, atol=1e-14).y[:, -1]
        assert np.all(np.abs(u - ref) <= 1e-4 * np.abs(ref) + 1e-9), (u, ref)
        # the first evaluation is at t0, the initial-step estimate's at tn + hg > t0 (not at tn), none past tf
        assert seen[0] == 0.0 and 0.0 < seen[1] < 1e-3 and max(seen) <= tf
    t = 2.0
    exact = (1.0 + w / (1 + w * w)) * np.exp(-t) + (np.sin(w * t) - w * np.cos(w * t)) / (1 + w * w)
    status, u, st = L.integrate_host(f1, [1.0, 1.0], t)
    assert abs(u[0] - exact) <= 1e-4 * abs(exact) + 1e-9


def test_host_cvode_rhs_failure_leaves_the_last_accepted_state(pkg):
    """An RHS that fails after a few steps: BR_ERR_RHS, and u / t_end are the state and time of the last
    on_step call (the last accepted step), not the predicted state of the attempt that failed."""
    L = pkg._lib
    n = 2
    steps, calls = [], [0]
    fail_at = [None]

    def rhs(_user, t, up, dup):
        calls[0] += 1
        if len(steps) >= 6:                            # after the fifth accepted step (row 0 is t = 0)
            fail_at[0] = t
            return 1
        dup[0] = -up[0] + np.sin(3.0 * t)
        dup[1] = -1e3 * (up[1] - np.cos(t))
        return 0

    def on_step(_user, t, up):
        steps.append((t, [up[0], up[1]]))
    u = np.array([1.0, 1.0])
    st = np.zeros(L.NSTAT)
    fr, fs = L.RHS_FN(rhs), L.STEP_FN(on_step)
    status = L.lib().br_integrate_host(n, fr, None, L.dptr(u), 5.0, 1e-6, 1e-10, 1000, fs, None, L.dptr(st))
    assert status == BR_ERR_RHS and st[7] == BR_ERR_RHS
    assert len(steps) == 6 and st[0] == 5                               # five accepted steps, then the failure
    t_last, u_last = steps[-1]
    assert st[13] == t_last, (st[13], t_last)                           # t_end: the last accepted time ...
    assert fail_at[0] > t_last                                          # (the failing attempt was past it)
    assert u.tolist() == u_last, (u, u_last)                            # ... and its state, bit for bit
