"""Engine: a compiled mechanism resident on one GPU (br_mech handle) and the batched hot-path
operators on it. This is the host mirror of the reference's operator interface:

  rates(...)      <- GasphaseReactions / SurfaceReactions.calculate_molar_production_rates!
                     (src/BatchReactor.jl:344,:355), batched
  rhs(...)        <- residual!(du,u,p,t) (src/BatchReactor.jl:312-376), batched
  jacobian(...)   <- the dense Jacobian CVODE forms inside CVODE_BDF() (:138-141,:210)
  integrate(...)  <- solve(ODEProblem(residual!,u0,(0,tf),params), CVODE_BDF();
                     reltol=1e-6, abstol=1e-10, save_everystep=false) (:138-141,:204-210)

Arrays are reactor-major: u[N, n], n = ng + ns, u = [rho*Y_k ; theta_k].
"""
import ctypes as C

import numpy as np

from . import _lib
from . import tprog as _tprog
from .mechanism import Mechanism

STAT_FIELDS = ("nsteps", "nfe", "nje", "nsetups", "nni", "ncfn", "netf", "status", "cyc_total", "cyc_rhs",
               "cyc_jac", "cyc_lu", "cyc_sol", "t_end", "cyc_ctl", "cyc_clk", "t_ign", "ign_rate", "ign_dt",
               "nfe_dq")
IGNITION_MARKER = "OH"   # the reference golden's ignition marker: max dX_OH/dt


def output_grid(tout, N):
    """The tout argument of the integrate calls as a C array: a 1-D grid shared by all reactors, or a
    2-D [N, nout] array, row i the ascending output times of reactor i (br_opts.tout_per_reactor; NaN
    = no output, trailing padding only). Returns (array or None, per_reactor). Raises ValueError for
    any other shape, before the library is called."""
    if tout is None:
        return None, False
    to = np.ascontiguousarray(tout, dtype=np.float64)
    if to.ndim == 1:
        return to, False
    if to.ndim != 2 or to.shape[0] != N:
        raise ValueError(f"tout must be [nout] or [N, nout] with N = {N}, got shape {to.shape}")
    return to, True


def phase_grid(t_ign, tau, tf):
    """Per-reactor output grid at the ignition phases tau: tout[i, j] = tau[j] * t_ign[i], NaN (no
    output) where t_ign[i] is NaN or the product exceeds tf[i]. tau ascending and positive, so the NaNs
    of a row are trailing. Pure numpy; the CPU mirror of br_phase_tout_dev, bit for bit (one rounded
    product per entry)."""
    t_ign = np.atleast_1d(np.asarray(t_ign, dtype=np.float64))
    tau = np.atleast_1d(np.asarray(tau, dtype=np.float64))
    tf = np.broadcast_to(np.asarray(tf, dtype=np.float64), t_ign.shape)
    p = t_ign[:, None] * tau[None, :]
    with np.errstate(invalid="ignore"):
        return np.where(p <= tf[:, None], p, np.nan)


def energy_mode(energy):
    """The energy argument of the integrate calls as br_opts.energy: None / False / 0 = the temperature is
    prescribed (isothermal or a programme), "adiabatic" (or 1) = adiabatic constant-volume reactors, T a state
    component (BR_ENERGY_ADIABATIC_V). Other integers pass through for the library to reject; any other
    value raises ValueError."""
    if energy is None or energy is False:
        return 0
    if isinstance(energy, str):
        if energy == "adiabatic":
            return _lib.ENERGY_ADIABATIC_V
        raise ValueError(f"energy must be None or 'adiabatic', got {energy!r}")
    if isinstance(energy, (int, np.integer)):
        return int(energy)
    raise ValueError(f"energy must be None or 'adiabatic', got {energy!r}")


def rate_mult_table(rate_mult, rate_mult_row, N, nr):
    """The rate_mult / rate_mult_row arguments of the integrate calls as C arrays (br_opts.rate_mult):
    rate_mult [nmult, nr] float64 with nr = nrg + nrs (gas reactions in mechanism order, then surface
    reactions), rate_mult_row [N] int32 giving each reactor's row, or None: then the table is dense,
    nmult == N. Returns (table or None, rows or None). Shapes are checked here (ValueError, before the
    library is called); the values -- finite, >= 0, rows in range -- by the library."""
    if rate_mult is None:
        if rate_mult_row is not None:
            raise ValueError("rate_mult_row without rate_mult")
        return None, None
    m = np.ascontiguousarray(rate_mult, dtype=np.float64)
    if m.ndim != 2 or m.shape[1] != nr or m.shape[0] < 1:
        raise ValueError(f"rate_mult must be [nmult, {nr}] (gas reactions, then surface reactions), got shape {m.shape}")
    if rate_mult_row is None:
        if m.shape[0] != N:
            raise ValueError(f"rate_mult has {m.shape[0]} rows for N = {N} reactors: pass rate_mult_row, or one row per reactor")
        return m, None
    rows = np.asarray(rate_mult_row)
    if rows.shape != (N,) or not np.issubdtype(rows.dtype, np.integer):
        raise ValueError(f"rate_mult_row must be {N} integers, got shape {rows.shape} of {rows.dtype}")
    return m, np.ascontiguousarray(rows, dtype=np.int32)


class Engine:
    def __init__(self, mech: Mechanism, device: int = 0):
        L = _lib.lib()
        self.mech = mech
        self.device = device
        t = mech.tables
        self._keep = []

        def d(a):
            a = np.ascontiguousarray(a, dtype=np.float64)
            self._keep.append(a)
            return _lib.dptr(a)

        def i(a):
            a = np.ascontiguousarray(a, dtype=np.int32)
            self._keep.append(a)
            return _lib.iptr(a)

        desc = _lib.MechDesc(
            mech.ng, mech.ns, mech.nrg, mech.nrs, mech.conv, mech.p_std,
            d(mech.molwt), d(mech.nasa),
            i(t["g_nf"]), i(t["g_nr"]), i(t["g_f"]), i(t["g_r"]), i(t["g_rev"]), i(t["g_tb"]),
            d(t["g_arr"]), d(t["g_low"]), i(t["g_troe_n"]), d(t["g_troe"]), d(t["g_eff"]),
            mech.site_density, d(mech.sigma),
            i(t["s_nf"]), i(t["s_np"]), i(t["s_f"]), i(t["s_p"]), i(t["s_stick"]), d(t["s_arr"]),
            i(t["s_ncov"]), i(t["s_cov_sp"]), d(t["s_cov_eps"]))
        h = C.c_void_p()
        _lib.check(L.br_mech_create(C.byref(desc), device, C.byref(h)))
        self.h = h
        self.n, self.ng, self.ns = mech.n, mech.ng, mech.ns
        self.nr = mech.nrg + mech.nrs   # row length of a rate-multiplier table
        # 1-based br_opts.ignition_species (0: the mechanism has no OH, t_ign not tracked)
        self.ign1 = mech.gas_species.index(IGNITION_MARKER) + 1 if IGNITION_MARKER in mech.gas_species else 0
        self.nmax = 16 if self.n <= 16 else 32 if self.n <= 32 else 56 if self.n <= 56 else 64 if self.n <= 64 else 72   # kernel tile

    @property
    def kernel_name(self) -> str:
        """the integrator kernel br_integrate_dev launches for this mechanism"""
        nm = _lib.lib().br_mech_engine(self.h)
        if nm < 0:   # group engine: -(100 * group width + register width)
            return f"k_group<{-nm // 100}, {-nm % 100}>"
        return f"k_lane<{nm}>" if nm > 0 else f"k_integrate<{self.nmax}>"

    @property
    def engine(self) -> str:
        """'lane' (one reactor per lane, small gas mechanisms), 'quad' / 'pair' (four / two reactors
        per wavefront, one per 16- / 32-lane group, n <= 16 / 32) or 'wave' (one reactor per wavefront)"""
        nm = _lib.lib().br_mech_engine(self.h)
        if nm < 0:
            return "quad" if -nm // 100 == 16 else "pair"
        return "lane" if nm > 0 else "wave"

    @property
    def launch_info(self) -> dict:
        """launch geometry of the engine in use (wave / group / lane): reactors per workgroup, resident
        waves per CU, LDS bytes per workgroup (br_mech_launch_info)"""
        rpb, wpc, lds = C.c_int(), C.c_int(), C.c_longlong()
        _lib.check(_lib.lib().br_mech_launch_info(self.h, C.byref(rpb), C.byref(wpc), C.byref(lds)))
        return {"reactors_per_workgroup": rpb.value, "waves_per_cu": wpc.value, "lds_bytes_per_workgroup": lds.value}

    def energy_launch_info(self) -> dict:
        """engine and launch geometry of an energy run (energy="adiabatic") of this mechanism under the current
        BRHIP_ENGINE (br_mech_energy_launch_info): "engine" 0 = the wavefront energy instance, -(100 GL + NM) = the
        group energy instance k_group<GL, NM, true>; reactors per workgroup, resident waves per CU, LDS bytes per
        workgroup, and "resident", the reactors in flight at once on its persistent grid"""
        e, rpb, wpc, lds, res = C.c_int(), C.c_int(), C.c_int(), C.c_longlong(), C.c_int()
        _lib.check(_lib.lib().br_mech_energy_launch_info(self.h, C.byref(e), C.byref(rpb), C.byref(wpc), C.byref(lds),
                                                         C.byref(res)))
        return {"engine": e.value, "reactors_per_workgroup": rpb.value, "waves_per_cu": wpc.value,
                "lds_bytes_per_workgroup": lds.value, "resident": res.value}

    @property
    def energy_kernel_name(self) -> str:
        """the integrator kernel an energy run (energy="adiabatic") of this mechanism launches"""
        e = self.energy_launch_info()["engine"]
        if e < 0:
            return f"k_group<{-e // 100}, {-e % 100}, true>"
        nsys = self.ng + 1
        return f"k_integrate<{16 if nsys <= 16 else 32 if nsys <= 32 else 56}, false, true>"

    def close(self):
        if getattr(self, "h", None):
            _lib.lib().br_mech_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _arr(a, N, dtype=np.float64):
        return np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype), (N,)))

    def rates(self, T, p, x, theta=None):
        x = np.ascontiguousarray(np.atleast_2d(x), dtype=np.float64)
        N = x.shape[0]
        T, p = self._arr(T, N), self._arr(p, N)
        th = None if (theta is None or self.ns == 0) else np.ascontiguousarray(np.atleast_2d(theta), dtype=np.float64)
        w = np.zeros((N, self.ng))
        s = np.zeros((N, self.n))
        _lib.check(_lib.lib().br_rates(self.h, N, _lib.dptr(T), _lib.dptr(p), _lib.dptr(x), _lib.dptr(th),
                                       _lib.dptr(w), _lib.dptr(s)))
        return w, s

    def rhs(self, T, Asv, u):
        u = np.ascontiguousarray(np.atleast_2d(u), dtype=np.float64)
        N = u.shape[0]
        T, A = self._arr(T, N), self._arr(Asv, N)
        du = np.zeros_like(u)
        _lib.check(_lib.lib().br_rhs(self.h, N, _lib.dptr(T), _lib.dptr(A), _lib.dptr(u), _lib.dptr(du)))
        return du

    def jacobian(self, T, Asv, u):
        u = np.ascontiguousarray(np.atleast_2d(u), dtype=np.float64)
        N = u.shape[0]
        T, A = self._arr(T, N), self._arr(Asv, N)
        J = np.zeros((N, self.n, self.n))
        _lib.check(_lib.lib().br_jacobian(self.h, N, _lib.dptr(T), _lib.dptr(A), _lib.dptr(u), _lib.dptr(J)))
        return J

    def group_eval(self, T, Asv, u):
        """(du, J) as the group integrator of this mechanism evaluates them (br_debug_group_eval: the
        device functions, LDS blocks and global slots of k_group); du [N, n], J [N, n, n] as jacobian()"""
        u = np.ascontiguousarray(np.atleast_2d(u), dtype=np.float64)
        N = u.shape[0]
        T, A = self._arr(T, N), self._arr(Asv, N)
        du = np.zeros_like(u)
        J = np.zeros((N, self.n, self.n))
        _lib.check(_lib.lib().br_debug_group_eval(self.h, N, _lib.dptr(T), _lib.dptr(A), _lib.dptr(u), _lib.dptr(du),
                                                  _lib.dptr(J)))
        return du, J

    def lane_eval(self, T, u, rate_mult=None, rate_mult_row=None):
        """(du, J) as the lane integrator of this mechanism evaluates them (br_debug_lane_eval: lane_tconst,
        lane_rhs, lane_jac in k_lane's LDS rows and global rows); rate_mult / rate_mult_row as integrate"""
        u = np.ascontiguousarray(np.atleast_2d(u), dtype=np.float64)
        N = u.shape[0]
        T = self._arr(T, N)
        mult, mrow = self._mult(rate_mult, rate_mult_row, N)
        du = np.zeros_like(u)
        J = np.zeros((N, self.n, self.n))
        _lib.check(_lib.lib().br_debug_lane_eval(self.h, N, _lib.dptr(T), _lib.dptr(u), 0 if mult is None else mult.shape[0],
                                                 _lib.dptr(mult), _lib.iptr(mrow), _lib.dptr(du), _lib.dptr(J)))
        return du, J

    @staticmethod
    def lane_lu(nm, J, gamma, b, skip=None, fill=-7.0):
        """(x, fail, piv) of the lane integrator's register LU and solve, k_lane<nm> (br_debug_lane_lu_solve):
        x [N, n], fail [N], piv [N, n] the pivot row of each step. skip [N]: matrices left out; their x
        entries keep `fill`, their fail and piv entries -1."""
        b = np.ascontiguousarray(b, dtype=np.float64)
        N, n = b.shape
        J = np.ascontiguousarray(J, dtype=np.float64)
        g = np.ascontiguousarray(gamma, dtype=np.float64)
        sk = None if skip is None else np.ascontiguousarray(skip, dtype=np.int32)
        x = np.full((N, n), fill)
        f = np.full(N, -1, np.int32)
        piv = np.full((N, n), -1, np.int32)
        _lib.check(_lib.lib().br_debug_lane_lu_solve(nm, N, n, _lib.dptr(J), _lib.dptr(g), _lib.dptr(b), _lib.iptr(sk),
                                                     _lib.dptr(x), _lib.iptr(f), _lib.iptr(piv)))
        return x, f, piv

    @staticmethod
    def wave_lu(J0, gamma0, b, J1=None, gamma1=None, perm_in=None, wpb=1, dirty=True, fill=-7.0):
        """(x, fail, perm, F) of the wavefront integrator's LU and solve (br_debug_wave_lu: lu_factor / lu_solve, for
        n > 64 lu_factor2 / lu_solve2, in k_integrate's order of calls). Leg A factors I - gamma0 J0 with the rows
        placed as perm_in [N, n] says (None: the identity) and solves b; leg B factors I - gamma1 J1 (None: leg A's
        matrix) in leg A's pivot order and solves b. x [2, N, n] (entries of a matrix with a zero pivot keep `fill`),
        fail [2, N], perm [2, N, n] (the original row of each step), F [2, N, W] the factor workspace in the device
        layout (include/brhip.h). wpb: waves per workgroup; dirty: NaNs in the workspace before leg A."""
        b = np.ascontiguousarray(b, dtype=np.float64)
        N, n = b.shape
        c = lambda a, t=np.float64: None if a is None else np.ascontiguousarray(a, dtype=t)
        J0, J1, g0, g1, pin = c(J0), c(J1), c(gamma0), c(gamma1), c(perm_in, np.int32)
        nmax = 16 if n <= 16 else 32 if n <= 32 else 56 if n <= 56 else 64 if n <= 64 else 72
        W = (nmax + 1) * 80 if nmax > 64 else nmax * nmax + 64
        x = np.full((2, N, max(n, 0)), fill)
        f = np.full((2, N), -1, np.int32)
        perm = np.full((2, N, max(n, 0)), -1, np.int32)
        F = np.zeros((2, N, W))
        _lib.check(_lib.lib().br_debug_wave_lu(N, n, int(wpb), int(bool(dirty)), _lib.dptr(J0), _lib.dptr(J1), _lib.dptr(g0),
                                               _lib.dptr(g1), _lib.dptr(b), _lib.iptr(pin), _lib.dptr(x), _lib.iptr(f),
                                               _lib.iptr(perm), _lib.dptr(F)))
        return x, f, perm, F

    def wave_eval(self, T, Asv, u, T_prev=None, rate_mult=None, rate_mult_row=None):
        """(du, J) as the wavefront integrator of this mechanism evaluates them (br_debug_wave_eval: k_integrate's
        instance width, reactors per workgroup, slots and init_tconst). T_prev [N]: the T-only constants are
        built at T_prev first and refreshed to T in the live slot, as in a temperature-programme run."""
        u = np.ascontiguousarray(np.atleast_2d(u), dtype=np.float64)
        N = u.shape[0]
        T, A = self._arr(T, N), self._arr(Asv, N)
        Tp = None if T_prev is None else self._arr(T_prev, N)
        mult, mrow = self._mult(rate_mult, rate_mult_row, N)
        du = np.zeros_like(u)
        J = np.zeros((N, self.n, self.n))
        _lib.check(_lib.lib().br_debug_wave_eval(self.h, N, _lib.dptr(T), _lib.dptr(A), _lib.dptr(u), _lib.dptr(Tp),
                                                 0 if mult is None else mult.shape[0], _lib.dptr(mult), _lib.iptr(mrow),
                                                 _lib.dptr(du), _lib.dptr(J)))
        return du, J

    def energy_eval(self, T, u, rate_mult=None, rate_mult_row=None):
        """du [N, ng + 1] = (du_0 .. du_{ng-1}, dT/dt) as the energy instance of the wavefront integrator evaluates
        it at the states (u, T) (br_debug_energy_eval: its launch shape, slots and refresh path)."""
        u = np.ascontiguousarray(np.atleast_2d(u), dtype=np.float64)
        N = u.shape[0]
        T = self._arr(T, N)
        mult, mrow = self._mult(rate_mult, rate_mult_row, N)
        du = np.zeros((N, self.ng + 1))
        _lib.check(_lib.lib().br_debug_energy_eval(self.h, N, _lib.dptr(T), _lib.dptr(u), 0 if mult is None else mult.shape[0],
                                                   _lib.dptr(mult), _lib.iptr(mrow), _lib.dptr(du)))
        return du

    def group_energy_eval(self, T, u, rate_mult=None, rate_mult_row=None):
        """du [N, ng + 1] as energy_eval, as the energy instance of the group engine evaluates it (br_debug_group_energy_eval:
        k_group<GL, NM, true>'s device functions, LDS blocks, global slots and refresh path; does not read
        BRHIP_ENGINE). The library answers -30 when the mechanism has no such instance."""
        u = np.ascontiguousarray(np.atleast_2d(u), dtype=np.float64)
        N = u.shape[0]
        T = self._arr(T, N)
        mult, mrow = self._mult(rate_mult, rate_mult_row, N)
        du = np.zeros((N, self.ng + 1))
        _lib.check(_lib.lib().br_debug_group_energy_eval(self.h, N, _lib.dptr(T), _lib.dptr(u),
                                                         0 if mult is None else mult.shape[0], _lib.dptr(mult), _lib.iptr(mrow),
                                                         _lib.dptr(du)))
        return du

    def _mult(self, rate_mult, rate_mult_row, N):
        """rate_mult_table for this mechanism's nrg + nrs reactions; (None, None) without multipliers"""
        if rate_mult is None and rate_mult_row is None:
            return None, None
        return rate_mult_table(rate_mult, rate_mult_row, N, self.nr)

    def _opts(self, rtol, atol, max_steps, trace_cap=0, unstable_factor=0.0, tout=None, yout=None, dq_jacobian=False,
              mult=None, mult_row=None, prog=None, energy=0, T_end=None, T_out=None):
        nout = 0 if tout is None else tout.shape[-1]   # tout: [nout], or [N, nout] (one row per reactor)
        o = _lib.Opts(rtol, atol, max_steps, self.device, 0.0, trace_cap, unstable_factor, self.ign1, nout=nout,
                      tout=_lib.dptr(tout) if nout else None, yout=_lib.dptr(yout) if nout else None, dq_jacobian=int(dq_jacobian),
                      tout_per_reactor=int(nout > 0 and tout.ndim == 2))
        if mult is not None:   # (arrays from rate_mult_table; the caller keeps them alive for the call)
            o.nmult, o.rate_mult = mult.shape[0], _lib.dptr(mult)
            o.rate_mult_row = _lib.iptr(mult_row) if mult_row is not None else None
        if prog is not None and prog[0] is not None:   # (kt, kT, rows) from tprog.table, kept alive by the caller
            kt, kT, rows = prog
            o.ntprog, o.ntprog_rows = kt.shape[1], kt.shape[0]
            o.tprog_t, o.tprog_T, o.tprog_row = _lib.dptr(kt), _lib.dptr(kT), _lib.iptr(rows)
        if energy:   # (T_end [N], T_out [N, nout]: host arrays the caller keeps alive for the call)
            o.energy, o.T_end, o.T_out = int(energy), _lib.dptr(T_end), _lib.dptr(T_out)
        return o

    def integrate(self, T, Asv, u0, tf, rtol=1e-6, atol=1e-10, max_steps=100000, trace_cap=0, tout=None,
                  unstable_factor=0.0, dq_jacobian=False, rate_mult=None, rate_mult_row=None, tprog=None,
                  tprog_row=None, energy=None):
        """Integrate N reactors 0 -> tf. With trace_cap > 0 also returns the per-step rows
        trace[N, trace_cap+1, 2n+4] = (t, h, q, p_last, u[n], y_last[n]): u the accepted state, y_last
        and p_last the state and pressure of the step's last RHS evaluation (save_data semantics).
        With tout (ascending output times) the stats dict also carries "yout" [N, nout, n], the
        states at those times (CVODE CV_NORMAL output, the step sequence is unchanged). tout is one
        1-D grid for all reactors or a 2-D [N, nout] array, row i reactor i's own grid (NaN = no output,
        trailing padding only; rows of yout without an output stay 0).
        dq_jacobian: CVODE's difference-quotient Jacobian (the reference's setting), both engines.
        rate_mult [nmult, nrg + nrs] scales the net rate of reaction r of reactor i by
        rate_mult[row(i), r] (gas reactions in mechanism order, then surface reactions; forward and
        reverse together; 0 switches a reaction off); rate_mult_row [N] gives the rows, None = one row
        per reactor.
        tprog: a prescribed temperature programme T(t) (tprog.TemperatureProgram: one for all reactors, a
        sequence -- one per reactor, or the rows tprog_row [N] selects -- or a pair (t, T) of [nrows, nk]
        knot arrays). T is then not read (None is fine), u0 is the caller's state at T(0), and the run
        uses the wavefront engine.
        energy="adiabatic": adiabatic constant-volume reactors (br_opts.energy): T is T(0) and becomes a state
        component, the stats carry "T_end" [N] and, with tout, "T_out" [N, nout]; gas-only mechanisms, CVODE's DQ
        Jacobian (dq_jacobian is not read), not together with tprog. The wavefront engine runs it, or, with env
        BRHIP_ENGINE = quad (ng + 1 <= 16) / pair (ng + 1 <= 32), the group engine's energy instance
        (energy_launch_info, energy_kernel_name)."""
        u = np.array(np.atleast_2d(u0), dtype=np.float64, order="C")
        N = u.shape[0]
        mult, mrow = self._mult(rate_mult, rate_mult_row, N)
        prog = _tprog.table(tprog, tprog_row, N)
        en = energy_mode(energy)
        to, _ = output_grid(tout, N)
        T = None if (T is None and prog[0] is not None) else self._arr(T, N)
        A, tf = self._arr(Asv, N), self._arr(tf, N)
        st = np.zeros((N, _lib.NSTAT))
        yo = None if to is None else np.zeros((N, to.shape[-1], self.n))
        Te = np.zeros(N) if en else None
        To = np.zeros((N, to.shape[-1])) if (en and to is not None) else None
        o = self._opts(rtol, atol, max_steps, trace_cap, unstable_factor, to, yo, dq_jacobian, mult, mrow, prog, en, Te, To)
        L = _lib.lib()
        if trace_cap > 0:
            tr = np.zeros((N, trace_cap + 1, 2 * self.n + 4))
            _lib.check(L.br_integrate_traced(self.h, N, _lib.dptr(T), _lib.dptr(A), _lib.dptr(u), _lib.dptr(tf),
                                             C.byref(o), _lib.dptr(st), _lib.dptr(tr)))
        else:
            tr = None
            _lib.check(L.br_integrate(self.h, N, _lib.dptr(T), _lib.dptr(A), _lib.dptr(u), _lib.dptr(tf),
                                      C.byref(o), _lib.dptr(st)))
        stats = {k: st[:, i] for i, k in enumerate(STAT_FIELDS)}
        if yo is not None:
            stats["yout"] = yo
        if Te is not None:
            stats["T_end"] = Te
        if To is not None:
            stats["T_out"] = To
        return (u, stats, tr) if trace_cap > 0 else (u, stats)

    def integrate_device(self, T_ptr, Asv_ptr, u_ptr, tf_ptr, stats_ptr, N, stream_ptr=None, rtol=1e-6,
                         atol=1e-10, max_steps=100000, tout_ptr=None, yout_ptr=None, nout=0, tout_per_reactor=False,
                         dq_jacobian=False, rate_mult=None, rate_mult_row=None, nmult=0, tprog_t=None, tprog_T=None,
                         ntprog=0, ntprog_rows=0, tprog_row=None, energy=None, T_end_ptr=None, T_out_ptr=None):
        """Device-resident variant: raw device pointers (e.g. torch tensor data_ptr()). Dense output
        with tout_ptr / yout_ptr / nout: device arrays tout [nout], or [N, nout] with tout_per_reactor
        (e.g. what phase_tout_device built), and yout [N, nout, n]. Rate multipliers: rate_mult is the
        device pointer of a float64 [nmult, nrg + nrs] table, rate_mult_row that of int32 [N] row indices
        (None: nmult == N, row i); the library trusts the device arrays. Temperature programmes: tprog_t /
        tprog_T the device pointers of float64 [ntprog_rows, ntprog] knot arrays, tprog_row that of int32 [N]
        (None: ntprog_rows == N); T_ptr is then not read. energy="adiabatic" as integrate: T_ptr is T(0),
        T_end_ptr / T_out_ptr the device pointers of float64 [N] / [N, nout] outputs (either may be None)."""
        o = self._opts(rtol, atol, max_steps, dq_jacobian=dq_jacobian)
        o.energy = energy_mode(energy)
        if o.energy:
            o.T_end = C.cast(C.c_void_p(T_end_ptr), _lib.dp) if T_end_ptr else None
            o.T_out = C.cast(C.c_void_p(T_out_ptr), _lib.dp) if T_out_ptr else None
        if tprog_t or tprog_T:
            if not (tprog_t and tprog_T) or ntprog < 1 or ntprog_rows < 1 or (not tprog_row and ntprog_rows != N):
                raise ValueError(f"tprog needs tprog_t, tprog_T, ntprog >= 1, ntprog_rows >= 1, and ntprog_rows == N = {N} "
                                 f"without tprog_row; got ntprog = {ntprog}, ntprog_rows = {ntprog_rows}")
            o.ntprog, o.ntprog_rows = int(ntprog), int(ntprog_rows)
            o.tprog_t, o.tprog_T = C.cast(C.c_void_p(tprog_t), _lib.dp), C.cast(C.c_void_p(tprog_T), _lib.dp)
            o.tprog_row = C.cast(C.c_void_p(tprog_row), _lib.ip) if tprog_row else None
        elif tprog_row:
            raise ValueError("tprog_row without tprog_t / tprog_T")
        if rate_mult:
            if nmult < 1 or (not rate_mult_row and nmult != N):
                raise ValueError(f"rate_mult needs nmult >= 1, and nmult == N = {N} without rate_mult_row; got {nmult}")
            o.nmult = int(nmult)
            o.rate_mult = C.cast(C.c_void_p(rate_mult), _lib.dp)
            o.rate_mult_row = C.cast(C.c_void_p(rate_mult_row), _lib.ip) if rate_mult_row else None
        elif rate_mult_row:
            raise ValueError("rate_mult_row without rate_mult")
        if nout and tout_ptr and yout_ptr:
            o.nout, o.tout_per_reactor = int(nout), int(bool(tout_per_reactor))
            o.tout, o.yout = C.cast(C.c_void_p(tout_ptr), _lib.dp), C.cast(C.c_void_p(yout_ptr), _lib.dp)
        _lib.check(_lib.lib().br_integrate_dev(self.h, N, C.c_void_p(T_ptr), C.c_void_p(Asv_ptr),
                                               C.c_void_p(u_ptr), C.c_void_p(tf_ptr), C.byref(o),
                                               C.c_void_p(stats_ptr), C.c_void_p(stream_ptr or 0)))

    def integrate_phase(self, T, Asv, u0, tf, tau, rtol=1e-6, atol=1e-10, max_steps=100000, dq_jacobian=False,
                        rate_mult=None, rate_mult_row=None, tprog=None, tprog_row=None, energy=None):
        """Ignition-phase sampling (br_integrate_phase): the states at t = tau[j] * t_ign[i], two passes
        on the device from the same u0 (t_ign, then the outputs at the grid br_phase_tout_dev builds).
        Returns (u, stats) as integrate, with stats["tout"] [N, ntau] (phase_grid(t_ign, tau, tf): NaN
        where t_ign is unknown or the phase is past tf) and stats["yout"] [N, ntau, n] (rows of NaN
        entries stay 0). Needs the ignition marker species in the mechanism. rate_mult / rate_mult_row and
        tprog / tprog_row as integrate: both passes run with them. energy="adiabatic" as integrate: both passes
        run with it, stats["T_end"] [N] and stats["T_out"] [N, ntau] (T at the phases) are pass 2's."""
        u = np.array(np.atleast_2d(u0), dtype=np.float64, order="C")
        N = u.shape[0]
        mult, mrow = self._mult(rate_mult, rate_mult_row, N)
        prog = _tprog.table(tprog, tprog_row, N)
        tau = np.ascontiguousarray(np.atleast_1d(tau), dtype=np.float64)
        if tau.ndim != 1 or tau.size == 0:
            raise ValueError(f"tau must be a non-empty 1-D array, got shape {tau.shape}")
        T = None if (T is None and prog[0] is not None) else self._arr(T, N)
        A, tf = self._arr(Asv, N), self._arr(tf, N)
        st = np.zeros((N, _lib.NSTAT))
        to = np.zeros((N, tau.size))
        yo = np.zeros((N, tau.size, self.n))
        en = energy_mode(energy)
        Te = np.zeros(N) if en else None
        To = np.zeros((N, tau.size)) if en else None
        o = self._opts(rtol, atol, max_steps, dq_jacobian=dq_jacobian, mult=mult, mult_row=mrow, prog=prog, energy=en,
                       T_end=Te, T_out=To)
        _lib.check(_lib.lib().br_integrate_phase(self.h, N, _lib.dptr(T), _lib.dptr(A), _lib.dptr(u), _lib.dptr(tf),
                                                 C.byref(o), _lib.dptr(st), tau.size, _lib.dptr(tau), _lib.dptr(to),
                                                 _lib.dptr(yo)))
        stats = {k: st[:, i] for i, k in enumerate(STAT_FIELDS)}
        stats["tout"], stats["yout"] = to, yo
        if en:
            stats["T_end"], stats["T_out"] = Te, To
        return u, stats

    def sensitivity(self, T, Asv, u0, tf, factor=2.0, reactions=None, states=False, rtol=1e-6, atol=1e-10,
                    max_steps=100000, dq_jacobian=False, tprog=None, tprog_row=None, energy=None):
        """Brute-force logarithmic sensitivities to the rate constants (br_sensitivity), built and reduced
        on the device: every base reactor is integrated with each selected reaction's rate times and
        over `factor`. reactions: 0-based indices (gas reactions in mechanism order, then surface
        reactions), None = all. Returns a dict with
          "S_tign" [N, nsel]: d ln t_ign / d ln k_r (central difference; only with the ignition marker
                   species in the mechanism),
          "S_u" [N, nsel, n] (with states=True): d u_k(tf) / d ln k_r,
          "u" [N, n] and "stats": the unperturbed end states and stats, as integrate's,
          "nbad": entries set to NaN (a perturbed run failed, or has no t_ign),
          "reactions": the indices used.
        tprog: not supported here (the library answers BR_ERR_UNSUPPORTED). energy="adiabatic": the expanded
        reactors run adiabatically from T = T(0), S_tign is the adiabatic ignition-delay sensitivity."""
        u0 = np.ascontiguousarray(np.atleast_2d(u0), dtype=np.float64)
        N = u0.shape[0]
        prog = _tprog.table(tprog, tprog_row, N)
        if not (np.isfinite(factor) and factor > 1.0):
            raise ValueError(f"factor must be finite and > 1, got {factor}")
        if reactions is None:
            rx = np.arange(self.nr, dtype=np.int32)
        else:
            rx = np.asarray(reactions)
            if rx.ndim != 1 or rx.size == 0 or not np.issubdtype(rx.dtype, np.integer):
                raise ValueError("reactions must be a non-empty 1-D sequence of integers")
            if rx.min() < 0 or rx.max() >= self.nr:
                raise ValueError(f"reactions must be in [0, {self.nr}), got {rx.min()} .. {rx.max()}")
            rx = np.ascontiguousarray(rx, dtype=np.int32)
        T, A, tf = self._arr(T, N), self._arr(Asv, N), self._arr(tf, N)
        nsel = rx.size
        St = np.zeros((N, nsel)) if self.ign1 else None
        Su = np.zeros((N, nsel, self.n)) if states else None
        u = np.zeros((N, self.n))
        st = np.zeros((N, _lib.NSTAT))
        nbad = C.c_longlong(0)
        o = self._opts(rtol, atol, max_steps, dq_jacobian=dq_jacobian, prog=prog, energy=energy_mode(energy))
        _lib.check(_lib.lib().br_sensitivity(self.h, N, _lib.dptr(T), _lib.dptr(A), _lib.dptr(u0), _lib.dptr(tf),
                                             C.byref(o), float(factor), nsel, _lib.iptr(rx), _lib.dptr(St),
                                             _lib.dptr(Su), _lib.dptr(u), _lib.dptr(st), C.byref(nbad)))
        out = {"u": u, "stats": {k: st[:, i] for i, k in enumerate(STAT_FIELDS)}, "nbad": nbad.value,
               "reactions": rx}
        if St is not None:
            out["S_tign"] = St
        if Su is not None:
            out["S_u"] = Su
        return out

    def phase_tout_device(self, stats, tau, tf, out=None, stream_ptr=None):
        """br_phase_tout_dev on torch tensors of this engine's device: stats [N, NSTAT] as
        integrate_device wrote it, tau [ntau] (ascending, positive), tf [N], all float64 and contiguous.
        Returns tout [N, ntau] = tau[j] * t_ign[i] (NaN: t_ign unknown or past tf), a per-reactor grid
        for br_integrate_dev; asynchronous on the stream (default: torch's current stream of the
        tensors' device). br_phase_tout_dev selects no device itself, so the launch is made with the
        tensors' device current."""
        import torch
        N, ntau = stats.shape[0], tau.shape[0]
        for name, t, shape in (("stats", stats, (N, _lib.NSTAT)), ("tau", tau, (ntau,)), ("tf", tf, (N,))):
            if tuple(t.shape) != shape or t.dtype != torch.float64 or not t.is_contiguous() or not t.is_cuda:
                raise ValueError(f"{name}: contiguous float64 device tensor of shape {shape} expected")
        if out is None:
            out = torch.empty((N, ntau), dtype=torch.float64, device=stats.device)
        elif tuple(out.shape) != (N, ntau) or out.dtype != torch.float64 or not out.is_contiguous() or not out.is_cuda:
            raise ValueError(f"out: contiguous float64 device tensor of shape {(N, ntau)} expected")
        with torch.cuda.device(stats.device):
            if stream_ptr is None:
                stream_ptr = torch.cuda.current_stream(stats.device).cuda_stream
            _lib.check(_lib.lib().br_phase_tout_dev(N, C.c_void_p(stats.data_ptr()), ntau, C.c_void_p(tau.data_ptr()),
                                                    C.c_void_p(tf.data_ptr()), C.c_void_p(out.data_ptr()),
                                                    C.c_void_p(stream_ptr or 0)))
        return out

    def last_kernel_ms(self):
        ms = np.zeros(1)
        _lib.check(_lib.lib().br_last_kernel_ms(self.h, _lib.dptr(ms)))
        return float(ms[0])


def integrate_multi(engines, T, Asv, u0, tf, rtol=1e-6, atol=1e-10, max_steps=100000, tout=None, rate_mult=None,
                    rate_mult_row=None, tprog=None, tprog_row=None, energy=None):
    """br_integrate_multi: the ensemble split into contiguous slices over `engines` (one Engine per
    GPU, same mechanism), integrated concurrently; returns (u, stats) in ensemble order. tout as
    Engine.integrate: [nout], or [N, nout] for per-reactor grids (sliced with the ensemble). rate_mult /
    rate_mult_row and tprog / tprog_row as Engine.integrate (the row indices, or the rows of a dense table,
    are sliced too). energy="adiabatic" as Engine.integrate: stats carry "T_end" and, with tout, "T_out"."""
    e0 = engines[0]
    u = np.array(np.atleast_2d(u0), dtype=np.float64, order="C")
    N = u.shape[0]
    mult, mrow = e0._mult(rate_mult, rate_mult_row, N)
    prog = _tprog.table(tprog, tprog_row, N)
    to, _ = output_grid(tout, N)
    T = None if (T is None and prog[0] is not None) else e0._arr(T, N)
    A, tf = e0._arr(Asv, N), e0._arr(tf, N)
    st = np.zeros((N, _lib.NSTAT))
    yo = None if to is None else np.zeros((N, to.shape[-1], e0.n))
    en = energy_mode(energy)
    Te = np.zeros(N) if en else None
    To = np.zeros((N, to.shape[-1])) if (en and to is not None) else None
    o = e0._opts(rtol, atol, max_steps, 0, 0.0, to, yo, mult=mult, mult_row=mrow, prog=prog, energy=en, T_end=Te, T_out=To)
    L = _lib.lib()
    hs = (C.c_void_p * len(engines))(*[e.h.value for e in engines])
    _lib.check(L.br_integrate_multi(hs, len(engines), N, _lib.dptr(T), _lib.dptr(A), _lib.dptr(u), _lib.dptr(tf),
                                    C.byref(o), _lib.dptr(st)))
    stats = {k: st[:, i] for i, k in enumerate(STAT_FIELDS)}
    if yo is not None:
        stats["yout"] = yo
    if Te is not None:
        stats["T_end"] = Te
    if To is not None:
        stats["T_out"] = To
    return u, stats
