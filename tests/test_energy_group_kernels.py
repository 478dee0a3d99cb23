"""The right-hand side of the group engines' energy instances (k_group<GL, NM, true>, brhip_group.hpp) through
br_debug_group_energy_eval -- their own device functions, workgroup shape, LDS blocks, global slots and refresh path
-- against oracle.rhs at the clamped T and dT/dt from Mechanism.thermo_e_cv, on all four instances and at the
widths where T sits on the last column of the register tile or the last lane of the group; which engine an energy
run would use (br_mech_energy_launch_info); and the mechanisms without a group energy instance."""
import os

import numpy as np
import pytest

import energy_group_cases as egc
from conftest import LIB
from test_gpu_parity import SURF_GAS, TH, _scale, _states

pytestmark = pytest.mark.gpu

R_GAS = 8.31446261815324
# mechanism, ng, (GL, NM) of its energy instance (from ng + 1)
CASES = [("s8", 8, 16, 9),           # T on lane 8, the tile's last column
         ("h2o2", 9, 16, 16),        # one shape up from the isothermal <16, 9>
         ("h2o2_n15", 15, 16, 16),   # T on the group's last lane
         ("h2o2_n16", 16, 32, 24),   # one shape up from the isothermal <16, 16>: another group width
         ("s24", 24, 32, 32),        # 129 reactions with Troe falloff
         ("h2o2_n31", 31, 32, 32)]   # T on lane 31


def _mechs(pkg, orc, tmp_path_factory, mech, conv):
    if mech == "h2o2":
        return (pkg.Mechanism.from_files(LIB, gas_mech="h2o2.dat", conv=conv),
                orc.Mech(os.path.join(LIB, "h2o2.dat"), TH, None, conv=conv))
    return egc.written(pkg, orc, tmp_path_factory, mech, conv)


@pytest.mark.parametrize("conv", [0, 19], ids=["textbook", "reference"])
@pytest.mark.parametrize("mech,ng,gl,nm", CASES, ids=[c[0] for c in CASES])
def test_group_energy_rhs_against_the_oracle(pkg, orc, gpu, monkeypatch, tmp_path_factory, mech, ng, gl, nm, conv):
    """test_energy_rhs_against_the_oracle's ensemble and bars on the group energy instances. N = 4 x the groups of a
    workgroup (16 quad, 8 pair) + 3: two workgroups, every group evaluates at least a second reactor in the slot of
    its first. Temperatures uniform in 300 .. 3200 K, the first four 1000 K (a Tmid), 150 K and 6500 K (clamped)
    and the mechanism's largest Tmid; with and without a 3-row multiplier table that has one zero entry. Species
    rows to 1e-11 of M_k sum_r |nu_kr q_r|, dT/dt to 1e-11 of sum_k |e_k w_k| / sum_k c_k cv_k (the wavefront
    instance sits at 6e-14 and 1.5e-14 of them; the group sums add in another order). The worst of each is
    printed; DESIGN.md records them."""
    pm, om = _mechs(pkg, orc, tmp_path_factory, mech, conv)
    assert pm.ns == 0 and pm.ng == ng
    eng = pkg.Engine(pm)
    code = -(100 * gl + nm)
    mine, other = ("quad", "pair") if gl == 16 else ("pair", "quad")
    monkeypatch.setenv("BRHIP_ENGINE", mine)
    info = eng.energy_launch_info()
    assert info["engine"] == code and info["reactors_per_workgroup"] == 4 * (64 // gl)
    assert info["resident"] > 0 and info["resident"] % info["reactors_per_workgroup"] == 0
    assert eng.energy_kernel_name == f"k_group<{gl}, {nm}, true>"
    for env in (other, "wave", "lane", None):   # every other setting: the wavefront energy instance
        if env is None:
            monkeypatch.delenv("BRHIP_ENGINE")
        else:
            monkeypatch.setenv("BRHIP_ENGINE", env)
        assert eng.energy_launch_info()["engine"] == 0, env
        assert eng.energy_kernel_name == f"k_integrate<{16 if ng + 1 <= 16 else 32}, false, true>"
    monkeypatch.setenv("BRHIP_ENGINE", mine)
    N = 4 * info["reactors_per_workgroup"] + 3
    _, p, x, _ = _states(pm, N, 21)
    rng = np.random.default_rng(22)
    T = rng.uniform(300.0, 3200.0, N)
    T[:4] = [1000.0, 150.0, 6500.0, pm.nasa[:, 0].max()]
    assert np.any(pm.nasa[:, 0] == 1000.0) and (T < 1000.0).sum() > 3 and (T > 1500.0).sum() > 3
    Tc = pm.clamp_T(T)
    U = np.stack([pm.initial_state(Tc[i], p[i], x[i]) for i in range(N)])
    mult = rng.uniform(0.5, 2.0, (3, pm.nrg))
    mult[1, 0] = 0.0
    rows = (np.arange(N) % 3).astype(np.int32)
    worst = [0.0, 0.0]
    for m in (None, mult):
        du = eng.group_energy_eval(T, U) if m is None else eng.group_energy_eval(T, U, rate_mult=m, rate_mult_row=rows)
        assert du.shape == (N, pm.ng + 1)
        for i in range(N):
            for r in range(pm.nrg):
                v = 1.0 if m is None else m[rows[i], r]
                om.set_rxn_mult(r, v, v)
            do = om.rhs(float(Tc[i]), 1.0, U[i])[0]
            c = U[i] / pm.molwt
            qg, qs = om.rop(float(Tc[i]), R_GAS * Tc[i] * c.sum(), c / c.sum())
            sc = _scale(pm, qg, qs) * pm.molwt
            e, cv = pm.thermo_e_cv(T[i])
            w = do / pm.molwt
            Td = pm.energy_rhs(do, U[i], T[i])
            sT = np.sum(np.abs(e * w)) / np.sum(c * cv)
            worst[0] = max(worst[0], float(np.max(np.abs(du[i, :-1] - do) / (sc + 1e-300))))
            worst[1] = max(worst[1], abs(du[i, -1] - Td) / sT)
            assert np.all(np.abs(du[i, :-1] - do) <= 1e-11 * sc + 1e-300), (mech, conv, m is not None, i)
            assert abs(du[i, -1] - Td) <= 1e-11 * sT, (mech, conv, m is not None, i, du[i, -1], Td)
    for r in range(pm.nrg):
        om.set_rxn_mult(r, 1.0, 1.0)
    print(f"\n  {mech} conv {conv} <{gl}, {nm}>: worst species row {worst[0] / 1e-11:.3g}, worst dT/dt {worst[1] / 1e-11:.3g} "
          f"(units of 1e-11)")
    eng.close()


def test_group_energy_eval_needs_an_instance(pkg, orc, gpu, monkeypatch, tmp_path_factory):
    """BR_ERR_UNSUPPORTED from br_debug_group_energy_eval where no group energy instance exists: H2/O2 with inerts at
    ng = 32 (ng + 1 = 33), GRI-Mech (54), and the Ni/CH4 surface mechanism; an energy run of the first two under
    BRHIP_ENGINE=pair would use the wavefront energy instance."""
    monkeypatch.setenv("BRHIP_ENGINE", "pair")
    pm32, _ = egc.written(pkg, orc, tmp_path_factory, "h2o2_n32", 0)
    gri = pkg.Mechanism.from_files(LIB, gas_mech="grimech.dat")
    sm = pkg.Mechanism.from_files(LIB, surface_mech="ch4ni.xml", gasphase=SURF_GAS)
    assert pm32.ng == 32 and gri.ng + 1 > 32 and sm.ns > 0
    for pm in (pm32, gri, sm):
        eng = pkg.Engine(pm)
        x = np.full(pm.ng, 1.0 / pm.ng)
        u0 = pm.initial_state(1000.0, 1e5, x)
        with pytest.raises(RuntimeError, match=r"-30: mechanism has no group energy instance"):
            eng.group_energy_eval([1000.0], u0[None, :pm.ng])
        if pm.ns == 0:
            assert eng.energy_launch_info()["engine"] == 0
        else:
            with pytest.raises(RuntimeError, match=r"-30: br_opts.energy: mechanisms with surface species"):
                eng.energy_launch_info()
        eng.close()
