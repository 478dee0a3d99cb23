"""Adiabatic reactors in the group engines (k_group<GL, NM, true>), the part that needs no GPU: the two new entry
points in the library, the header and every binding, and their answers before a handle is looked at."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT

BR_ERR_INPUT = -10
NEW = ("br_mech_energy_launch_info", "br_debug_group_energy_eval")


def test_exports_version_and_bindings(pkg):
    """Both symbols are in libbrhip.so, in include/brhip.h and in _lib.EXPORTS; br_version() tells the ABI that has
    them; the Python wrappers and the Julia function exist; br_opts did not change with them (its checks are
    test_energy_host's)."""
    L = pkg._lib
    lib = L.lib()
    assert lib.br_version() >= 231
    hdr = open(os.path.join(ROOT, "include", "brhip.h")).read()
    for sym in NEW:
        assert sym in L.EXPORTS and hasattr(lib, sym), sym
        assert re.search(rf"\bint\s+{sym}\(", hdr), sym
    E = pkg.Engine
    assert callable(E.energy_launch_info) and callable(E.group_energy_eval)
    assert isinstance(E.energy_kernel_name, property) and isinstance(E.kernel_name, property)
    jl = open(os.path.join(ROOT, "julia", "BatchReactorHIP.jl")).read()
    assert "function energy_launch_info(m::Ptr{Cvoid})" in jl and "(:br_mech_energy_launch_info, lib)" in jl


def test_null_handle_is_an_input_error(pkg):
    """BR_ERR_INPUT from both calls on a null handle, with every other argument in order: nothing reaches a GPU."""
    L = pkg._lib
    lib = L.lib()
    e, rpb, wpc, res, lds = C.c_int(7), C.c_int(7), C.c_int(7), C.c_int(7), C.c_longlong(7)
    assert lib.br_mech_energy_launch_info(None, C.byref(e), C.byref(rpb), C.byref(wpc), C.byref(lds), C.byref(res)) == BR_ERR_INPUT
    assert lib.br_last_error().decode()
    assert (e.value, rpb.value, wpc.value, lds.value, res.value) == (7, 7, 7, 7, 7)      # nothing written
    assert lib.br_mech_energy_launch_info(None, None, None, None, None, None) == BR_ERR_INPUT
    T, u, du = np.full(2, 1000.0), np.ones((2, 3)), np.zeros((2, 4))
    assert lib.br_debug_group_energy_eval(None, 2, L.dptr(T), L.dptr(u), 0, None, None, L.dptr(du)) == BR_ERR_INPUT
    assert lib.br_last_error().decode() and not du.any()
