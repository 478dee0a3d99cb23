"""The wavefront engine's chemistry in the integrator's own configuration, kernel by kernel: init_tconst<CPL,
true>, rhs and jacobian through br_debug_wave_eval (wave_ctx<CPL, NMAX> of the mechanism's k_integrate instance,
its reactors per workgroup on one table block, slots and LDS blocks reused at another T, J read as the LU reads
it) against the oracle's rhs and jac on all five instances, the refresh of the T-only constants in a live slot
(temperature programmes) bit for bit, and per-reactor rate multipliers on gas and surface reactions."""

import os

import numpy as np
import pytest

from conftest import LIB
from test_gpu_parity import _mechs
from test_group_kernels import _wide_states, subset_mechanism
from test_lane_kernels import assert_parity, multiplier_rows, reference_states

pytestmark = pytest.mark.gpu

KERNELS = {"h2o2": "k_integrate<16>", "surf": "k_integrate<32>", "gri": "k_integrate<56>", "gri47+ni": "k_integrate<64>",
           "gas_surf": "k_integrate<72>"}
SURFACE = ("surf", "gri47+ni", "gas_surf")


def wave_pair(pkg, orc, tmp_path, mech, conv=None):
    """product and oracle mechanisms of a KERNELS entry (gri47+ni: GRI-Mech without six species + the Ni
    surface mechanism, n = 60, as test_remaining_integrator_instances builds it)"""
    if mech != "gri47+ni":
        return _mechs(pkg, orc, mech, conv)
    conv = orc.CONV_REFERENCE if conv is None else conv
    gri = pkg.Mechanism.from_files(LIB, gas_mech="grimech.dat").gas_species
    species = [s for s in gri if s not in ("AR", "C3H7", "C3H8", "CH2CHO", "CH3CHO", "HCNO")]
    d = subset_mechanism(tmp_path, species, surface="ch4ni.xml")
    pm = pkg.Mechanism.from_files(d, gas_mech="mech.dat", surface_mech="ch4ni.xml", conv=conv)
    om = orc.Mech(os.path.join(d, "mech.dat"), os.path.join(d, "therm.dat"), os.path.join(d, "ch4ni.xml"), conv=conv)
    assert pm.n == 60
    return pm, om


def _wave_engine(pkg, monkeypatch, pm, mech):
    monkeypatch.setenv("BRHIP_ENGINE", "wave")
    eng = pkg.Engine(pm)
    assert eng.engine == "wave" and eng.kernel_name == KERNELS[mech], (eng.engine, eng.kernel_name)
    return eng


def assert_slots_reused(eng, N):
    """br_debug_wave_eval's grid (include/brhip.h): one workgroup of rpb waves up to 4 rpb reactors, two above;
    wave w takes reactors w, w + waves, ...: every wave of the grid gets at least two"""
    rpb = eng.launch_info["reactors_per_workgroup"]
    waves = rpb * min(2, (N + 4 * rpb - 1) // (4 * rpb))
    assert 1 <= rpb <= 16 and N >= 2 * waves, (rpb, waves, N)
    return waves


_EVAL_CASES = [(m, c) for m in KERNELS for c in (0, 19, 23) if c != 23 or m in SURFACE]


@pytest.mark.parametrize("mech,conv", _EVAL_CASES, ids=[f"{m}-conv{c}" for m, c in _EVAL_CASES])
def test_wave_rhs_jacobian_parity(pkg, orc, gpu, monkeypatch, tmp_path, mech, conv):
    """init_tconst<CPL, true>, rhs and jacobian as k_integrate<16 | 32 | 56 | 64 | 72> runs them (br_debug_wave_eval)
    against the oracle's rhs / jac at the bars of test_group_rhs_jacobian_parity. conv 0 (textbook), 19
    (reference) and, with surface species, 23 (Asv_th = 1). 37 states on one workgroup of the integrator's
    size (two where it has fewer than 10 waves): every wave evaluates at least two reactors, one after the
    other in its slot (asserted from the launch geometry); T 700-2000 K, p 1e3-1e7 Pa, Asv in [1, 100];
    state 5 has the reactants of the first falloff reaction at exactly 0."""
    assert (orc.CONV_REFERENCE, orc.CONV_REFERENCE | orc.CONV_DOC_COVG) == (19, 23)
    pm, om = wave_pair(pkg, orc, tmp_path, mech, conv)
    eng = _wave_engine(pkg, monkeypatch, pm, mech)
    assert_slots_reused(eng, 37)
    T, Asv, U, ref = reference_states(pm, om, 37, 31)
    assert Asv.min() >= 1.0 and Asv.max() <= 100.0
    du, J = eng.wave_eval(T, Asv, U)
    assert_parity(f"wave_eval {mech} conv {conv}", U, du, J, ref)


@pytest.mark.parametrize("switch", ["BRHIP_JFAST", "BRHIP_SPREAD"])
def test_wave_parity_host_layout_switches(pkg, orc, gpu, monkeypatch, tmp_path, switch):
    """the same on GRI with the A/B layouts behind the host switches: the general column-list Jacobian,
    scatter lists in first-appearance order. The switches are read when the handle is made; that the other
    layout was built shows in the bits: another summation order in J (JFAST) or in du (SPREAD) than the
    default handle's, which was made before the switch was set."""
    pm, om = wave_pair(pkg, orc, tmp_path, "gri")
    monkeypatch.delenv(switch, raising=False)
    eng0 = _wave_engine(pkg, monkeypatch, pm, "gri")
    monkeypatch.setenv(switch, "0")
    eng = _wave_engine(pkg, monkeypatch, pm, "gri")
    T, Asv, U, ref = reference_states(pm, om, 37, 31)
    du, J = eng.wave_eval(T, Asv, U)
    assert_parity(f"wave_eval gri {switch}=0", U, du, J, ref)
    du0, J0 = eng0.wave_eval(T, Asv, U)
    changed = J if switch == "BRHIP_JFAST" else du
    assert not _bits_equal(changed, J0 if switch == "BRHIP_JFAST" else du0), switch
    du1, J1 = eng.wave_eval(T, Asv, U)
    assert _bits_equal(du1, du) and _bits_equal(J1, J)        # (run to run the bits stand: the layout made them differ)


def _bits_equal(a, b):
    return np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("mech", list(KERNELS))
def test_wave_tconst_refresh_in_a_live_slot(pkg, orc, gpu, monkeypatch, tmp_path, mech):
    """The refresh of a temperature-programme run (tprog_refresh: wave_sync, then init_tconst<CPL, true> at the
    new T in a slot whose constants were built at T_prev and have been read by an RHS) leaves nothing of
    T_prev behind: (du, J) with T_prev equal the call without it bit for bit. 16 of 37 reactors go down
    through 1000 K, the NASA-7 mid-range temperature, 14 up, 7 stay on their side."""
    pm, _ = wave_pair(pkg, orc, tmp_path, mech)
    eng = _wave_engine(pkg, monkeypatch, pm, mech)
    N = 37
    assert_slots_reused(eng, N)
    _, Asv, U = _wide_states(pm, N, 31)
    rng = np.random.default_rng(77)
    lo, hi = rng.uniform(300.0, 1000.0, N), rng.uniform(1000.0, 2000.0, N)
    kind = np.arange(N) % 5                               # 0, 1: down; 2, 3: up; 4: both above
    T = np.where(kind < 2, lo, hi)
    T_prev = np.where(kind < 2, hi, np.where(kind < 4, lo, hi[::-1]))
    down = (T_prev >= 1000.0) & (T < 1000.0)
    up = (T_prev < 1000.0) & (T >= 1000.0)
    assert down.sum() >= (N + 2) // 3 and up.sum() >= (N + 2) // 3, (down.sum(), up.sum())
    assert np.all(T_prev != T)
    du0, J0 = eng.wave_eval(T, Asv, U)
    du1, J1 = eng.wave_eval(T, Asv, U, T_prev=T_prev)
    assert np.any(du0 != 0.0) and np.any(J0 != 0.0)
    assert _bits_equal(du1, du0), np.flatnonzero(np.any(du1 != du0, axis=1))
    assert _bits_equal(J1, J0), np.flatnonzero(np.any(J1 != J0, axis=(1, 2)))
    dup, _ = eng.wave_eval(T_prev, Asv, U)                # (T_prev is another evaluation)
    assert np.all(np.any(dup != du0, axis=1))


@pytest.mark.parametrize("mech", ["gri", "surf"])
def test_wave_multipliers_parity(pkg, orc, gpu, monkeypatch, tmp_path, mech):
    """Per-reactor rate multipliers through init_tconst<CPL, true> (gas_tconst / surf_tconst), gas reactions on
    GRI and surface reactions on the Ni mechanism: every second reactor's reactions at factors from {0, 0.5,
    1, 2, 7.3}, the falloff reactions among them, against the oracle with set_rxn_mult at the same bars; a
    table of ones gives the bits of the call without one."""
    pm, om = wave_pair(pkg, orc, tmp_path, mech)
    eng = _wave_engine(pkg, monkeypatch, pm, mech)
    assert (pm.nrs > 0) == (mech == "surf") and eng.nr == pm.nrg + pm.nrs
    N = 37
    assert_slots_reused(eng, N)
    mult = multiplier_rows(pm, N, 7)
    T, Asv, U, ref = reference_states(pm, om, N, 31, mult)
    du, J = eng.wave_eval(T, Asv, U, rate_mult=mult)
    assert_parity(f"wave_eval {mech} with multipliers", U, du, J, ref)
    du0, J0 = eng.wave_eval(T, Asv, U)
    du1, J1 = eng.wave_eval(T, Asv, U, rate_mult=np.ones((1, eng.nr)), rate_mult_row=np.zeros(N, np.int32))
    assert _bits_equal(du1, du0) and _bits_equal(J1, J0)
    assert not np.array_equal(du, du0)
    assert _bits_equal(du[0::2], du0[0::2]) and _bits_equal(J[0::2], J0[0::2])   # (the rows of ones)
