"""The host side of the per-reactor rate multipliers and br_sensitivity, without a GPU: the new br_opts
fields in every binding and their defaults, the packed-order permutation a multiplier row is read through
(csrc/mech_pack_dump), and the Python argument checks that run before the library is called."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import LIB, ROOT
from test_julia_binding import _ARG, _header, _julia, _split_top

_PACK_DUMP = os.path.join(ROOT, "batchreactor.jl_amd", "mech_pack_dump")
NEW_FIELDS = [("nmult", "int", "Cint", C.c_int), ("rate_mult", "constdouble*", "Ptr{Float64}", None),
              ("rate_mult_row", "constint*", "Ptr{Cint}", None)]


def _bare_engine(pkg, n=9, nr=18):
    e = pkg.Engine.__new__(pkg.Engine)                 # no handle: nothing here may reach the GPU
    e.device, e.ign1, e.n, e.nr, e.h = 0, 0, n, nr, None
    return e


def test_new_opts_fields_in_every_binding_and_their_defaults(pkg):
    _, structs, protos = _header()
    L = pkg._lib
    # the three fields sit between dq_jacobian and tout_per_reactor, which stays the last field
    assert [(n, t) for n, t, _ in structs["br_opts"][-4:-1]] == [(n, t) for n, t, _, _ in NEW_FIELDS]
    assert L.Opts._fields_[-4:-1] == [("nmult", C.c_int), ("rate_mult", L.dp), ("rate_mult_row", L.ip)]
    assert [n for n, _, _ in structs["br_opts"]] == [f[0] for f in L.Opts._fields_]
    assert structs["br_opts"][-5][0] == "dq_jacobian" and structs["br_opts"][-1][0] == "tout_per_reactor"
    # every field up to dq_jacobian keeps the offset it had
    assert (L.Opts.dq_jacobian.offset < L.Opts.nmult.offset < L.Opts.rate_mult.offset < L.Opts.rate_mult_row.offset
            < L.Opts.tout_per_reactor.offset)
    assert L.Opts.nmult.offset == L.Opts.dq_jacobian.offset + 4
    assert L.lib().br_version() >= 210                     # (the layout change is visible to a caller)
    o = _bare_engine(pkg)._opts(1e-6, 1e-10, 100)
    assert o.nmult == 0 and not o.rate_mult and not o.rate_mult_row and o.tout_per_reactor == 0
    grid = np.zeros((5, 3))
    og = _bare_engine(pkg)._opts(1e-6, 1e-10, 100, tout=grid, yout=np.zeros((5, 3, 9)), dq_jacobian=True)
    assert (og.tout_per_reactor, og.dq_jacobian, og.nout, og.nmult) == (1, 1, 3, 0)
    assert L.Opts().nmult == 0 and not L.Opts().rate_mult
    m = np.ones((2, 18))
    rows = np.zeros(5, np.int32)
    o = _bare_engine(pkg)._opts(1e-6, 1e-10, 100, mult=m, mult_row=rows)
    assert o.nmult == 2 and C.addressof(o.rate_mult.contents) == m.ctypes.data
    assert C.addressof(o.rate_mult_row.contents) == rows.ctypes.data
    # Julia: the struct, the keyword constructor's defaults, the constructor that sets a table
    _, src, _, jstructs, _ = _julia()
    assert jstructs["BrOpts"][-4:-1] == [(n, jt) for n, _, jt, _ in NEW_FIELDS]
    ctor = src.split("\nBrOpts(;")[1].split("\n\n")[0]
    assert re.search(r"Cint\(dq_jacobian\), Cint\(0\), C_NULL, C_NULL,\s*Cint\(tout_per_reactor\)\)", ctor), ctor
    assert "with_rate_mult(o::BrOpts, mult::Matrix{Float64}" in src
    assert len(re.findall(r"BrOpts\(o(?:pts)?\.rtol", src)) == 2       # the two positional copies carry 16 fields
    for m_ in re.finditer(r"BrOpts\((o(?:pts)?\.rtol.*?)\)\n", src, re.S):
        assert len(_split_top(m_.group(1))) == 16, m_.group(1)


def test_br_sensitivity_is_bound_in_python_and_julia(pkg):
    """br_sensitivity has a `const int*` argument; the Julia wrapper binds it with @ccall, argument by
    argument in the prototype's order. Checked here against the header the same way the ccall bindings are."""
    _, _, protos = _header()
    ret, cargs = protos["br_sensitivity"]
    assert ret == "int" and len(cargs) == 15
    L = pkg._lib
    assert "br_sensitivity" in L.EXPORTS
    raw = open(os.path.join(ROOT, "julia", "BatchReactorHIP.jl")).read()
    m = re.search(r"@ccall lib\.br_sensitivity\((.*?)\)::Cint\)", raw, re.S)
    assert m, "no @ccall of br_sensitivity"
    jt = [a.rsplit("::", 1)[1].strip() for a in _split_top(m.group(1))]
    assert len(jt) == len(cargs), (jt, cargs)
    table = dict(_ARG)
    table["constint*"] = {"Ptr{Cint}"}
    for k, (ct, t) in enumerate(zip(cargs, jt)):
        assert t in table[ct], (k, ct, t)
    assert "function ignition_sensitivity(" in raw and "ignition_sensitivity" in raw.split("\nexport ")[1]
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "ignition_sensitivity" in doc and "sens=true" in doc


@pytest.mark.parametrize("gas,surf,gasphase", [("h2o2.dat", None, None), ("grimech.dat", None, None),
                                               ("grimech.dat", "ch4ni.xml", None)], ids=["h2o2", "gri", "gri+ni"])
def test_multiplier_row_through_the_packed_order(pkg, tmp_path, gas, surf, gasphase):
    """mech_pack keeps, with the packed tables, the gas reaction of br_mech_desc at every packed position
    (g_perm: falloff, then +M, then elementary). A multiplier row in the caller's order read through it
    scales, at every packed position, exactly the reaction whose Arrhenius parameters sit there: packing
    the mechanism with A_r m_r gives g_par[4 i] = g_par0[4 i] m[g_perm[i]], bit for bit (m a power of two),
    and the surface reactions keep their order."""
    out = tmp_path / "packed"
    out.mkdir()
    cmd = [_PACK_DUMP, str(out), os.path.join(LIB, "therm.dat"), os.path.join(LIB, gas),
           os.path.join(LIB, surf) if surf else "-"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    pm = pkg.Mechanism.from_files(LIB, gas_mech=gas, surface_mech=surf)
    nrg, nrs = pm.nrg, pm.nrs
    perm = np.frombuffer((out / "g_perm.bin").read_bytes(), np.int32)
    tb = np.asarray(pm.tables["g_tb"])
    assert sorted(perm.tolist()) == list(range(nrg))
    assert perm.tolist() == [r for p in (2, 1, 0) for r in range(nrg) if tb[r] == p]
    assert not np.array_equal(perm, np.arange(nrg))                    # (the order does differ from the caller's)
    gpar = np.frombuffer((out / "g_par.bin").read_bytes(), np.float64).reshape(-1, 4)[:nrg]
    m = 2.0 ** ((np.arange(nrg + nrs) * 7) % 11 - 5)                  # a row in the caller's order, all distinct exponents mod 11
    A = np.asarray(pm.tables["g_arr"])[:, 0]
    np.testing.assert_array_equal(gpar[:, 0], A[perm])                  # packed position i holds reaction perm[i]
    np.testing.assert_array_equal(gpar[:, 0] * m[:nrg][perm], (A * m[:nrg])[perm])
    # a position read without the permutation would take another reaction's multiplier
    assert np.any(m[:nrg][perm] != m[:nrg])
    if nrs:
        spar = np.frombuffer((out / "s_par.bin").read_bytes(), np.float64).reshape(-1, 4)[:nrs]
        np.testing.assert_array_equal(spar[:, 0], np.asarray(pm.tables["s_arr"])[:, 0])   # surface: the caller's order


def test_wrong_multiplier_arguments_raise_before_the_library(pkg, monkeypatch):
    def no_lib():
        raise AssertionError("the library was called")
    monkeypatch.setattr(pkg._lib, "lib", no_lib)
    e = _bare_engine(pkg)
    U0 = np.ones((5, 9))
    bad = [dict(rate_mult=np.ones((5, 17))), dict(rate_mult=np.ones(18)), dict(rate_mult=np.ones((4, 18))),
           dict(rate_mult=np.ones((0, 18)), rate_mult_row=np.zeros(5, np.int32)),
           dict(rate_mult=np.ones((2, 18)), rate_mult_row=np.zeros(4, np.int32)),
           dict(rate_mult=np.ones((2, 18)), rate_mult_row=np.zeros(5)),
           dict(rate_mult_row=np.zeros(5, np.int32))]
    for kw in bad:
        with pytest.raises(ValueError, match="rate_mult"):
            e.integrate(1000.0, 1.0, U0, 1e-3, **kw)
        with pytest.raises(ValueError, match="rate_mult"):
            e.integrate_phase(1000.0, 1.0, U0, 1e-3, [1.0], **kw)
        with pytest.raises(ValueError, match="rate_mult"):
            pkg.integrate_multi([e, e], 1000.0, 1.0, U0, 1e-3, **kw)
    with pytest.raises(ValueError, match="nmult"):
        e.integrate_device(8, 8, 8, 8, 8, 5, rate_mult=8, nmult=4)
    with pytest.raises(ValueError, match="rate_mult_row without"):
        e.integrate_device(8, 8, 8, 8, 8, 5, rate_mult_row=8)
    for kw, msg in ((dict(factor=1.0), "factor"), (dict(factor=np.inf), "factor"), (dict(reactions=[]), "reactions"),
                    (dict(reactions=[0, 18]), "reactions"), (dict(reactions=[-1]), "reactions"),
                    (dict(reactions=[0.5]), "reactions")):
        with pytest.raises(ValueError, match=msg):
            e.sensitivity(1000.0, 1.0, U0, 1e-3, **kw)
    # what passes the checks: the table as float64 C array, the rows as int32
    m, rows = pkg.engine.rate_mult_table([[1, 2]] * 3, [0, 2, 1, 0], 4, 2)
    assert m.dtype == np.float64 and m.flags.c_contiguous and rows.dtype == np.int32 and rows.tolist() == [0, 2, 1, 0]
    assert pkg.engine.rate_mult_table(None, None, 4, 2) == (None, None)
