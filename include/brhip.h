/*
 * brhip.h -- C-ABI of libbrhip.so, the MI355X (gfx950) batched stiff-kinetics engine that
 * sits behind BatchReactor.jl's hot path. Plain C types only; fp64 everywhere; int status
 * return (0 = OK, negative = error class, message via br_last_error()).
 *
 * Reference interfaces each entry point replaces (paths relative to the reference root):
 *   br_mech_create   <- compile_gaschemistry / SurfaceReactions.compile_mech /
 *                       IdealGas.create_thermo results (src/BatchReactor.jl:254,265,287):
 *                       the host flattens the compiled mechanism into br_mech_desc.
 *   br_mech_parse /  <- the same three compilers reading the mechanism library files
 *   br_mech_compile     (src/BatchReactor.jl:242-287); br_read_batch_xml <- input_data (:238-306)
 *   br_rates         <- GasphaseReactions.calculate_molar_production_rates!(g_state,gmd,thermo)
 *                       (call site src/BatchReactor.jl:355) and
 *                       SurfaceReactions.calculate_molar_production_rates!(s_state,thermo,smd)
 *                       (call site :344), batched over N states.
 *   br_rhs           <- residual!(du,u,p,t) (src/BatchReactor.jl:312-376), batched.
 *   br_jacobian      <- the dense Jacobian CVODE builds by finite differences inside
 *                       solve(..., CVODE_BDF()) (:138-141, :208-210); here analytic.
 *   br_integrate     <- solve(ODEProblem(residual!,u0,(0,tf),params), CVODE_BDF();
 *                       reltol=1e-6, abstol=1e-10, save_everystep=false)
 *                       (src/BatchReactor.jl:138-141 and :204-210), for N reactors at once.
 *   br_integrate_dev <- same, device-resident buffers on a caller stream (ensemble driver).
 *
 * Layout: per-reactor rows, reactor-major: u[N][n] with n = ng + ns and
 * u_k = rho*Y_k (kg/m3) for k < ng, theta_k for ng <= k < n (src/BatchReactor.jl:224-231).
 * A handle may be used by one host thread at a time; there is no global state.
 */
#ifndef BRHIP_H
#define BRHIP_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define BR_OK             0
#define BR_ERR_MAXSTEPS  -1   /* CVODE CV_TOO_MUCH_WORK  */
#define BR_ERR_ERRTEST   -3   /* CVODE CV_ERR_FAILURE     */
#define BR_ERR_CONV      -4   /* CVODE CV_CONV_FAILURE    */
#define BR_ERR_UNSTABLE  -7   /* NaN state (SciML ReturnCode.Unstable), or the opt-in runaway test of
                                 br_opts.unstable_factor */
#define BR_ERR_RHS       -8   /* CVODE CV_RHSFUNC_FAIL: a br_integrate_host right-hand side returned != 0 */
#define BR_ERR_INPUT    -10
#define BR_ERR_HIP      -20
#define BR_ERR_UNSUPPORTED -30

/* convention switches (bitmask); 0 = textbook CHEMKIN-II in SI units. BR_CONV_REFERENCE is what
 * the reference's GasphaseReactions does (identified from its golden output):
 * rates in mol/cm3 with Kc = Kp (p0/RT)^dnu in mol/m3, falloff rates also x [M] (mol/cm3), Troe
 * c = -4.0 - 0.67 log10 Fcent. */
#define BR_CONV_KC_UNIT_SLIP  1   /* Kc *= (1e6)^dnu for every reversible reaction          */
#define BR_CONV_FALLOFF_XM    2   /* falloff net rate *= [M] in mol/cm3 (1e-6 [M]_SI)       */
#define BR_CONV_DOC_COVG      4   /* no Asv on dtheta/dt (docs sample, predates :345)      */
#define BR_CONV_TROE_C4      16   /* Troe c = -4.0 - 0.67 log10 Fcent                       */
#define BR_CONV_REFERENCE    (BR_CONV_KC_UNIT_SLIP | BR_CONV_FALLOFF_XM | BR_CONV_TROE_C4)

/* br_opts.energy */
#define BR_ENERGY_ADIABATIC_V 1   /* adiabatic, constant volume: T is a state component */

typedef struct br_mech br_mech;

typedef struct br_mech_desc {
    int ng, ns, nrg, nrs;
    int conv;                 /* BR_CONV_* bitmask                                 */
    double p_std;             /* standard pressure for Kc [Pa]                     */
    const double* molwt;      /* [ng] kg/mol                                       */
    const double* nasa;       /* [ng][15]: Tmid, a_hi[7], a_lo[7] (NASA-7)         */
    /* gas reactions (CHEMKIN-II) */
    const int* g_nf;          /* [nrg] expanded reactant entries (<=4)             */
    const int* g_nr;          /* [nrg] expanded product entries  (<=4)             */
    const int* g_f;           /* [nrg][4] species index per entry, -1 pad          */
    const int* g_r;           /* [nrg][4]                                          */
    const int* g_rev;         /* [nrg] 1 reversible                                */
    const int* g_tb;          /* [nrg] 0 none, 1 third body (+M), 2 falloff (+M)   */
    const double* g_arr;      /* [nrg][3] A (SI), beta, Ea/R [K] (k_inf if falloff) */
    const double* g_low;      /* [nrg][3] k0: A (SI), beta, E/R                    */
    const int* g_troe_n;      /* [nrg] 0 Lindemann, else number of Troe params 3|4 */
    const double* g_troe;     /* [nrg][4] a, T***, T*, T**                         */
    const double* g_eff;      /* [nrg][ng] third-body efficiencies (tb rows)       */
    /* surface reactions */
    double site_density;      /* mol/cm2                                           */
    const double* sigma;      /* [ns] site coordination                           */
    const int* s_nf;          /* [nrs] <=6                                         */
    const int* s_np;          /* [nrs] <=6                                         */
    const int* s_f;           /* [nrs][6] combined index: gas 0..ng-1, surface ng.. */
    const int* s_p;           /* [nrs][6]                                          */
    const int* s_stick;       /* [nrs] 1 sticking coefficient reaction             */
    const double* s_arr;      /* [nrs][3] A (SI) or s0, beta, Ea [J/mol]           */
    const int* s_ncov;        /* [nrs] coverage-dependent terms (<=4)              */
    const int* s_cov_sp;      /* [nrs][4] combined species index                  */
    const double* s_cov_eps;  /* [nrs][4] J/mol                                    */
} br_mech_desc;

typedef struct br_opts {
    double rtol, atol;        /* default 1e-6 / 1e-10 (src/BatchReactor.jl:141,:210) */
    int max_steps;            /* default 100000 (Sundials.jl maxiters)             */
    int device;               /* HIP device ordinal for br_mech_create             */
    double hmax;              /* 0 = unbounded                                     */
    int trace_cap;            /* br_integrate_traced: max accepted steps recorded  */
    double unstable_factor;   /* > 0: also stop a reactor with BR_ERR_UNSTABLE once max_k |u_k|
                                 exceeds factor * sum_k |u0_k| (not a reference behaviour;
                                 default 0 = only a NaN state stops it, as SciML's check) */
    int ignition_species;     /* 1-based gas species index k+1 whose max dX_k/dt over the accepted
                                 steps marks ignition (br_stats.t_ign; OH for the reference's
                                 ignition marker); 0 = not tracked                          */
    int energy;               /* 0 (default): the reactor stays at its T[i] (or follows its programme).
                                 BR_ENERGY_ADIABATIC_V: adiabatic constant-volume reactor. The state of
                                 reactor i is (u_0 .. u_{ng-1}, T) with u_k = rho Y_k; the T argument of the
                                 entry point is T(0). The species equations are the isothermal du_k/dt
                                 evaluated at the current T (RT in the diagnosed pressure, every T-only
                                 constant with the reactor's rate multipliers), and
                                     dT/dt = - ( sum_k e_k(Tc) w_k ) / ( sum_k c_k cv_k(Tc) ),
                                     c_k = u_k / M_k,   w_k = (du_k/dt) / M_k,
                                     e_k = (h_k/RT - 1) R Tc,   cv_k = (cp_k/R - 1) R,
                                 h_k/RT and cp_k/R from species k's NASA-7 row (the low range when
                                 T < Tmid, else the high one, as for g/RT). w_k is taken from the RHS's own
                                 du_k, so the integrated system conserves E = sum_k c_k e_k(T) identically,
                                 whatever conv bits are set. Tc = T < 200 ? 200 : (T > 6000 ? 6000 : T), a
                                 NaN passes through: everything that depends on temperature (constants,
                                 thermo, RT) is evaluated at Tc, so a Newton iterate outside the fits
                                 cannot produce a NaN from log. The NaN-state check covers the T component;
                                 the opt-in unstable_factor test looks at the species only. Error weight of
                                 T: 1 / (rtol |T| + atol), as for any other component. Gas-only mechanisms
                                 with ng + 1 <= 56 (else BR_ERR_UNSUPPORTED). An energy run uses the
                                 wavefront engine, unless env BRHIP_ENGINE asks for the group engine of its
                                 width -- quad with ng + 1 <= 16, pair with 16 < ng + 1 <= 32 -- and the
                                 mechanism has a group energy instance (<= 32 third-body efficiency sets,
                                 the instance fits the LDS): then k_group<GL, NM, true> runs it, four or two
                                 reactors per wave (br_mech_energy_launch_info tells which). Either engine
                                 builds CVODE's DQ Jacobian over ng + 1 columns: dq_jacobian
                                 is not read, nfe_dq == nje * (ng + 1). Rate multipliers, tout,
                                 tout_per_reactor, the ignition marker, hmax and max_steps behave as in an
                                 isothermal run. Not together with ntprog (BR_ERR_INPUT), any other value
                                 is BR_ERR_INPUT; br_integrate_traced answers BR_ERR_UNSUPPORTED (the trace
                                 row has no T column). u, yout and their shapes do not change          */
    double* T_end;            /* [N] out, or NULL: T at t_end (the last accepted state's on failure). Host
                                 memory for the host entry points, device memory for br_integrate_dev    */
    double* T_out;            /* [N][nout] out, or NULL: T at the dense-output times; entries are left
                                 untouched where the rows of yout are. (These three sit between
                                 ignition_species and nout: the fields from yout's successor ntprog to
                                 tout_per_reactor keep their order, as the bindings' tests pin them; a caller
                                 built against the earlier header must be rebuilt, br_version() 230)     */
    int nout;                 /* dense output: number of output times (0 = none)            */
    const double* tout;       /* [nout] ascending output times, shared by all reactors (or
                                 [N][nout], one row per reactor, with tout_per_reactor); the
                                 state there is CVODE's CV_NORMAL output (CVodeGetDky(t, 0) on
                                 the step that passes t), the step sequence is unchanged     */
    double* yout;             /* [N][nout][n] states at tout (host memory for br_integrate,
                                 device memory for br_integrate_dev); rows with tout > tf are
                                 left untouched                                             */
    int ntprog;               /* knots per temperature programme; 0 (default) = none: every reactor stays
                                 at its T[i]. With a programme, reactor i's temperature at time t is the
                                 piecewise-linear interpolant of its row of knots (t_j, T_j),
                                     T(t) = T_j + (t - t_j) * ((T_{j+1} - T_j) / (t_{j+1} - t_j))
                                 for t_j <= t < t_{j+1} (this formula, in this order of operations, on
                                 host and device), held at the last knot's value for t beyond it. The T
                                 argument of the entry point is then not read and may be NULL; the caller
                                 builds u0 at T(0). Everything the right-hand side takes from T follows
                                 T(t): RT in the diagnosed pressure, the coverage factor, every T-only
                                 constant (with the reactor's rate multipliers). Each RHS is evaluated at
                                 the time CVODE hands to f; the Jacobian stays d f / d u at that T. A
                                 programme run always uses the wavefront engine (as traced runs do). The
                                 BDF is not restarted at a knot: a kink is left to the error test, as
                                 CVODE does without a tstop there. br_sensitivity with a programme
                                 returns BR_ERR_UNSUPPORTED; br_rates, br_rhs, br_jacobian take none   */
    const double* tprog_t;    /* [ntprog_rows][ntprog] knot times, ascending, tprog_t[r][0] == 0; NaN only
                                 as trailing padding of a row (ragged rows, as in tout)               */
    const double* tprog_T;    /* [ntprog_rows][ntprog] temperatures [K] at the knots, finite and > 0
                                 (entries under a NaN time are not read)                              */
    int ntprog_rows;          /* rows of tprog_t / tprog_T                                            */
    const int* tprog_row;     /* [N] row of reactor i, or NULL: then ntprog_rows == N and row i (the
                                 indirection of rate_mult_row: one ramp can serve a whole ensemble).
                                 Host memory for br_integrate, _traced, _multi (sliced with the
                                 ensemble) and _phase: every row and row index is checked before any
                                 launch, BR_ERR_INPUT names the first bad reactor and row. Device
                                 memory for br_integrate_dev, which checks the shape only. (These five
                                 sit between yout and dq_jacobian: the fields from dq_jacobian to
                                 tout_per_reactor stay the struct's tail, in their order; a caller built
                                 against the earlier header must be rebuilt, and br_version() 220 tells
                                 the layouts apart)                                                   */
    int dq_jacobian;         /* 1: CVODE's dense difference-quotient Jacobian (cvLsDenseDQJac:
                                 the reference's CVODE_BDF() setting, src/BatchReactor.jl:140,
                                 :204), n extra RHS per Jacobian, in every engine (lane,
                                 group, wavefront); 0 (default): the analytic Jacobian       */
    int nmult;                /* rows of rate_mult; 0 = no multipliers (default)            */
    const double* rate_mult;  /* [nmult][nrg+nrs] per-reactor rate multipliers, mechanism order: gas
                                 reactions as in br_mech_desc, then surface reactions. The net rate of
                                 reaction r of reactor i is scaled by m = rate_mult[row(i)][r], applied
                                 to the T-only constants: gas kf *= m before kr = kf / Kc (both
                                 directions scale, equilibrium is kept; a falloff's k0 / k_inf is
                                 untouched, so k_inf and k0 scale together), surface k *= m (sticking
                                 and Arrhenius forms; the coverage factor stays). m finite and >= 0;
                                 0 switches the reaction off. Every engine and both Jacobians honour
                                 it. Host memory for br_integrate, _traced, _multi and _phase (every
                                 entry and row index checked, BR_ERR_INPUT names the first bad one),
                                 device memory for br_integrate_dev, which trusts the arrays       */
    const int* rate_mult_row; /* [N] row of reactor i, or NULL: then nmult == N and row i.
                                 (These three sit before tout_per_reactor, which stays the last
                                 field: a caller built against the earlier header must be rebuilt,
                                 as for any growth of this struct; br_version() tells them apart) */
    int tout_per_reactor;     /* 0 (default): tout is one grid [nout] shared by all reactors.
                                 1: tout is [N][nout], row i the ascending output times of
                                 reactor i (host memory for br_integrate, _traced and _multi,
                                 device memory for br_integrate_dev); yout keeps its shape.
                                 A NaN entry means "no output": allowed only as trailing
                                 padding of a row (ragged grids), its yout rows are left
                                 untouched, like rows with tout > tf[i]. The host entry points
                                 check every row (BR_ERR_INPUT names the first bad reactor);
                                 br_integrate_dev trusts the device array                    */
} br_opts;

#define BR_NSTAT 20
typedef struct br_stats {     /* per reactor; counters as CVODE's, then device cycles */
    double nsteps, nfe, nje, nsetups, nni, ncfn, netf, status;
    double cyc_total;         /* wall clock ticks (100 MHz) for the whole reactor  */
    double cyc_rhs, cyc_jac, cyc_lu, cyc_sol;  /* shader clocks in each phase      */
    double t_end;             /* time reached                                      */
    double cyc_ctl;           /* shader clocks in the step controller (diagnostic build) */
    double cyc_clk;           /* shader clocks for the whole reactor (diagnostic build)  */
    double t_ign;             /* ignition time: midpoint of the accepted step with the largest
                                 dX_k/dt, k = br_opts.ignition_species (NaN if not tracked) */
    double ign_rate;          /* that largest dX_k/dt [1/s]                                */
    double ign_dt;            /* width of that step (the resolution of t_ign) [s]            */
    double nfe_dq;            /* RHS evaluations of the DQ Jacobian (CVODE's nfeDQ; not in nfe) */
} br_stats;
#ifdef __cplusplus   /* stats arrays are [N][BR_NSTAT] doubles: one br_stats per reactor, no padding */
static_assert(sizeof(br_stats) == BR_NSTAT * sizeof(double), "br_stats is BR_NSTAT doubles");
#endif

int         br_version(void);
const char* br_last_error(void);
int         br_device_count(void);

int br_mech_create(const br_mech_desc* desc, int device, br_mech** out);

/* ---- host mechanism compiler (C++, no GPU): the data formats the reference reads, flattened into
 * br_mech_desc. Replaces, as one step:
 *   compile_gaschemistry(get_path(lib_dir, <gas_mech>))       src/BatchReactor.jl:251-255
 *   IdealGas.create_thermo(gasphase, get_path(lib_dir, "therm.dat"))                   :242-243,:265
 *   SurfaceReactions.compile_mech(get_path(lib_dir, <surface_mech>), thermo, gasphase) :283-287
 * gas_mech_path: CHEMKIN-II mechanism, or NULL/"" for surface-only runs, whose gas species are then
 * the space-separated names of `gasphase` (the <gasphase> tag, :256-260). surf_mech_path: surface
 * XML or NULL. conv: BR_CONV_* bits (BR_CONV_REFERENCE = the reference's gas kinetics). The
 * tables are bit-identical to the Python host compiler's (batchreactor.jl_amd/mechanism.py). */
typedef struct br_host_mech br_host_mech;
int br_mech_parse(const char* gas_mech_path, const char* therm_path, const char* surf_mech_path,
                  const char* gasphase, int conv, br_host_mech** out);
/* desc's pointers point into h: valid until br_host_mech_free(h) */
int br_host_mech_desc(const br_host_mech* h, br_mech_desc* desc);
int br_host_mech_sizes(const br_host_mech* h, int* ng, int* ns, int* nrg, int* nrs);
/* name of species i (gas species 0..ng-1 in mechanism order, then surface species), upper case */
int br_host_mech_species(const br_host_mech* h, int i, char* buf, size_t n);
/* initial coverages of the surface species (<site><initial>, the u0 tail of :228-230) */
int br_host_mech_theta0(const br_host_mech* h, double* theta0 /*[ns]*/);
int br_host_mech_free(br_host_mech* h);
/* br_mech_parse + br_mech_create in one call */
int br_mech_compile(const char* gas_mech_path, const char* therm_path, const char* surf_mech_path,
                    const char* gasphase, int conv, int device, br_mech** out);

/* batch.xml (input_data, src/BatchReactor.jl:238-306; schema docs/src/index.md:80-123). Asv is 1
 * when the tag is missing (the reference's behaviour). The composition is the
 * <molefractions> list (comp_is_mass = 0) or else <massfractions> (1), names upper case. */
#define BR_BATCH_MAXCOMP 64
typedef struct br_batch_input {
    char gas_mech[256];
    char surface_mech[256];
    char gasphase[1024];      /* space-separated gas species names (surface-only runs) */
    double T, p, Asv, time;
    int has_T, has_p, has_Asv, has_time;
    int ncomp, comp_is_mass;
    char comp_names[BR_BATCH_MAXCOMP][32];
    double comp_values[BR_BATCH_MAXCOMP];
} br_batch_input;
int br_read_batch_xml(const char* path, br_batch_input* out);
int br_mech_destroy(br_mech* m);
int br_mech_info(const br_mech* m, int* ng, int* ns, int* nrg, int* nrs);
/* integrator engine br_integrate* uses for this mechanism: 0 = one reactor per wavefront
 * (k_integrate), NM > 0 = one reactor per lane with NM-wide register tiles (k_lane, gas-only
 * mechanisms with n <= 12), -(100 GL + NM) < 0 = a group engine, one reactor per GL-lane group of a
 * wavefront with NM-wide register tiles (k_group<GL, NM>; GL = 16 "quad", n <= 16, the default for
 * such mechanisms; GL = 32 "pair", 16 < n <= 32; gas and surface chemistry, <= 32 third-body
 * efficiency sets). All of them take br_opts.dq_jacobian. Traced integrations always use the
 * wavefront engine; env BRHIP_ENGINE = wave | lane | quad | pair forces one where the mechanism is
 * eligible. */
int br_mech_engine(const br_mech* m);
/* launch geometry of the engine br_integrate uses for this mechanism (br_mech_engine; diagnostics):
 * reactors per workgroup, resident waves per CU (occupancy calculator: VGPRs and LDS), LDS bytes
 * per workgroup (staged tables + one block per reactor or group). Any pointer may be NULL. */
int br_mech_launch_info(const br_mech* m, int* rpb, int* waves_per_cu, long long* lds_bytes);
/* the same for an energy run (br_opts.energy) of this handle under the current BRHIP_ENGINE: *engine = 0 (the
 * wavefront energy instance) or -(100 GL + NM) (the group energy instance k_group<GL, NM, true>, (GL, NM) from
 * ng + 1: <= 9: (16, 9), <= 16: (16, 16), <= 24: (32, 24), <= 32: (32, 32)), its reactors per workgroup,
 * resident waves per CU and LDS bytes per workgroup, and *resident, the reactors in flight at once on its
 * persistent grid. The shapes are found at the first call (or energy run) and kept in the handle. Any out pointer
 * may be NULL. A null handle is BR_ERR_INPUT; a surface mechanism or ng + 1 > 56 BR_ERR_UNSUPPORTED, as an
 * energy run. */
int br_mech_energy_launch_info(br_mech* m, int* engine, int* rpb, int* waves_per_cu, long long* lds_bytes, int* resident);

/* host-buffer entry points (copy in/out); arrays are reactor-major */
int br_rates(br_mech* m, int N, const double* T, const double* p, const double* x /*[N][ng]*/,
             const double* theta /*[N][ns] or NULL*/, double* wdot /*[N][ng]*/,
             double* sdot /*[N][ng+ns] or NULL*/);
int br_rhs(br_mech* m, int N, const double* T, const double* Asv, const double* u /*[N][n]*/,
           double* du /*[N][n]*/);
int br_jacobian(br_mech* m, int N, const double* T, const double* Asv, const double* u,
                double* J /*[N][n][n] row-major d(du_i)/d(u_j)*/);
int br_integrate(br_mech* m, int N, const double* T, const double* Asv, double* u /*in/out*/,
                 const double* tf, const br_opts* opts, br_stats* stats /*[N] or NULL*/);

/* as br_integrate, and also records the state after every accepted step (the rows
 * save_data writes, src/BatchReactor.jl:383-402): trace[N][trace_cap+1][2n+4] with
 * row = (t, h, q, p_last, u[0..n-1], y[0..n-1]): u is the accepted state, y and p_last the state
 * and pressure of the last RHS evaluation of that step (save_data reads x, p and coverages from
 * the last RHS call and rho from u). Row 0 is t=0; unused rows are left as zeros. The last
 * written row is the tstop row (t = tf). */
int br_integrate_traced(br_mech* m, int N, const double* T, const double* Asv, double* u,
                        const double* tf, const br_opts* opts, br_stats* stats, double* trace);

/* multi-GPU ensemble: N reactors split into ndev contiguous slices (sizes
 * differ by at most one), slice d integrated on mechs[d] -- one handle per GPU, created with
 * br_mech_create(desc, device d, ...) -- concurrently (one host thread per handle), results
 * written back into the caller's host arrays in ensemble order. No inter-GPU traffic: every
 * slice is copied straight back to host memory. Arguments as br_integrate (opts->yout, when set,
 * is [N][nout][n] for the whole ensemble). Replaces running the reference's solve() once per
 * reactor (src/BatchReactor.jl:138-141). */
int br_integrate_multi(br_mech* const* mechs, int ndev, int N, const double* T, const double* Asv, double* u,
                       const double* tf, const br_opts* opts, br_stats* stats);

/* device-buffer entry point: all pointers are device memory on m's device; `stream` is a
 * hipStream_t (NULL = default stream). Asynchronous: returns after the launch. Calls on one
 * handle share its workspaces (work counter, Jacobian / LU slots, timing events): they must be
 * ordered on one stream (or synchronised); concurrent integrations need one handle each. */
int br_integrate_dev(br_mech* m, int N, const double* dT, const double* dAsv, double* du,
                     const double* dtf, const br_opts* opts, br_stats* dstats, void* stream);

/* ignition-phase output grid, built on the device (a small kernel on `stream`, asynchronous):
 * dtout[i][j] = dtau[j] * dstats[i].t_ign, or NaN ("no output") where t_ign is NaN (not tracked, or
 * the reactor failed before a step was accepted) or the product exceeds dtf[i]. dtau[ntau] ascending
 * and positive, so the NaNs of a row are trailing: dtout[N][ntau] is a valid per-reactor grid for
 * br_integrate_dev (br_opts.tout_per_reactor = 1, nout = ntau). All pointers are device memory; dstats
 * is what an earlier br_integrate_dev on the same stream wrote (br_opts.ignition_species != 0). For
 * device-resident ensembles: both passes run with no host round trip. The call takes no handle and
 * selects no device: the device that owns `stream` and the arrays must be the caller's current one. */
int br_phase_tout_dev(int N, br_stats* dstats /*read only*/, int ntau, const double* dtau, const double* dtf,
                      double* dtout, void* stream);

/* ignition-phase sampling, host buffers: the states at t = tau[j] * t_ign[i]. Two passes on the
 * device from the same u0: pass 1 integrates without outputs for t_ign, br_phase_tout_dev builds
 * the per-reactor grid, pass 2 integrates with it. The step sequence does not depend on the outputs,
 * so pass 2's t_ign is pass 1's and every output sits at exactly the phase asked for. tau[ntau]
 * ascending, positive and finite. Needs opts->ignition_species != 0 (else BR_ERR_INPUT);
 * opts->nout / tout / yout / tout_per_reactor are ignored. u (in: u0, out: u(tf)) and stats are pass
 * 2's, equal to a plain br_integrate's. tout[N][ntau] receives the grid (NaN = no output: t_ign
 * unknown or tau[j] t_ign[i] > tf[i]); yout[N][ntau][n] rows of NaN entries are left untouched. With
 * opts->energy both passes run with it; opts->T_end [N] and opts->T_out [N][ntau] (T at the phases, entries of
 * NaN times left untouched) are pass 2's. */
int br_integrate_phase(br_mech* m, int N, const double* T, const double* Asv, double* u, const double* tf,
                       const br_opts* opts, br_stats* stats, int ntau, const double* tau,
                       double* tout /*[N][ntau] out*/, double* yout /*[N][ntau][n] out*/);

/* brute-force logarithmic sensitivities to the rate constants, built and reduced on the device. With
 * f = factor > 1 and reaction r = rxn[j] (0-based, mechanism order as br_opts.rate_mult; rxn NULL = all
 * nrg + nrs reactions, nsel ignored):
 *   S_tign[i][j]  = (ln t_ign(k_r f) - ln t_ign(k_r / f)) / (2 ln f)   = d ln t_ign / d ln k_r
 *                   (needs opts->ignition_species, else BR_ERR_INPUT)
 *   S_u[i][j][k]  = (u_k(tf; k_r f) - u_k(tf; k_r / f)) / (2 ln f)     = d u_k(tf) / d ln k_r
 * Each base reactor is expanded on the device into 2 nsel + 1 reactors that share one multiplier table
 * (row 0 unperturbed), integrated with br_integrate_dev in chunks of base reactors sized by a memory
 * budget (env BRHIP_SENS_CHUNK = base reactors per launch overrides it; the results do not depend on
 * it), and reduced there: only S, the unperturbed end states u[N][n] and their stats cross to the host.
 * An entry is NaN when either perturbed run failed, S_tign also when either has no t_ign; *nbad counts
 * the NaN entries written. opts->rate_mult must be unset; the output fields of opts are ignored. With
 * opts->energy the expanded reactors run adiabatically (T_end and T_out are ignored) and S_tign is the
 * adiabatic ignition-delay sensitivity. Host
 * memory throughout; S_tign, S_u, u, stats and nbad may each be NULL. */
int br_sensitivity(br_mech* m, int N, const double* T, const double* Asv, const double* u0, const double* tf,
                   const br_opts* opts, double factor, int nsel, const int* rxn /*[nsel] or NULL = all*/,
                   double* S_tign /*[N][nsel] or NULL*/, double* S_u /*[N][nsel][n] or NULL*/,
                   double* u /*[N][n] out: unperturbed end states, or NULL*/, br_stats* stats /*[N] unperturbed, or NULL*/,
                   long long* nbad /*entries set to NaN, or NULL*/);

/* dense-solver check (tests): factor I - gamma_i*J_i with the engine's batched LU and solve
 * x_i = (I - gamma_i J_i)^-1 b_i. J[N][n][n] row-major; fail[i] = 0 or (k+1) for a zero pivot. */
int br_debug_lu_solve(int N, int n, const double* J, const double* gamma, const double* b, double* x, int* fail);

/* wavefront LU check (tests): the factorization and solve of k_integrate (lu_factor / lu_solve for n <= 64,
 * lu_factor2 / lu_solve2 for 64 < n <= 72, the instance of n as in a run: 16, 32, 56, 64 or 72 wide) strung
 * together as the integrator does. Per matrix i, leg A factors I - gamma0_i J0_i with original row perm_in[i][s] loaded
 * into position s (perm_in NULL: the identity, a reactor's first LU) and solves b_i; leg B factors I - gamma1_i J1_i
 * (J1 / gamma1 NULL: J0 / gamma0 again) with the rows in leg A's pivot order and solves b_i again. Outputs, leg A
 * then leg B: x[2][N][n]; fail[2][N] = 0 or (k+1) for a zero pivot -- no solve then, as in a run, and the x entries
 * keep the caller's values; perm[2][N][n], the original row of each pivot step; F[2][N][W], the factor workspace
 * after the leg in the device layout, W = nmax * nmax + 64 doubles for nmax <= 64 (column-major M with nmax rows
 * per column, rows in step order: L below the diagonal, D^-1 U above, 0 on it; then D^-1[64]) and (72 + 1) * 80 for
 * n > 64 (72 columns of 80 rows, then D^-1[80]). dirty != 0: before leg A every double of the factor workspace,
 * and in both legs every double of the saved-J block outside rows and columns < n, holds a quiet NaN (in a run the
 * factor area holds Jacobian scratch). wpb waves per workgroup, 1 .. the integrator's limit for the width (4, or 16 for
 * 32 < n <= 64, 12 above), each with its own LDS scratch and workspace slot; one workgroup up to N = 4 wpb, two
 * above, a wave taking matrices slot, slot + waves, ... in the same slot. BR_ERR_INPUT: n outside 1..72, wpb out of
 * range, a perm_in row that is no permutation of 0..n-1, a NULL array other than J1, gamma1, perm_in. */
int br_debug_wave_lu(int N, int n, int wpb, int dirty, const double* J0, const double* J1, const double* gamma0,
                     const double* gamma1, const double* b, const int* perm_in, double* x, int* fail, int* perm, double* F);

/* group-engine check (tests): RHS and analytic Jacobian as the group integrator evaluates them,
 * through the device functions, workgroup shape, LDS blocks and global slots of the instance
 * br_integrate would launch for this mechanism (BR_ERR_UNSUPPORTED when it has none, n > 32). At most
 * two workgroups: each group evaluates its reactors one after another in the same block and slot.
 * du[N][n]; J[N][n][n] row-major, d(du_i)/d(u_j), as br_jacobian. Asv may be NULL (1.0). */
int br_debug_group_eval(br_mech* m, int N, const double* T, const double* Asv, const double* u, double* du, double* J);

/* group-engine check (tests): the register-resident LU and solve of the group integrator instance
 * (gl, nm) = (16, 9), (16, 16), (32, 24) or (32, 32), n <= nm (else BR_ERR_INPUT). Arguments as
 * br_debug_lu_solve; matrix i sits in group i mod (64 / gl) of its wave. perm[N][n]: the original row
 * at each row position after the interchanges; fail[i] = 0 or (k+1) for a zero pivot (x_i = 0 then). */
int br_debug_group_lu_solve(int gl, int nm, int N, int n, const double* J, const double* gamma, const double* b,
                            double* x, int* fail, int* perm);

/* lane-engine check (tests): RHS and analytic Jacobian as the one-reactor-per-lane integrator evaluates
 * them (lane_tconst, lane_rhs, lane_jac in k_lane's workgroup shape, LDS rows and global rows;
 * BR_ERR_UNSUPPORTED when the mechanism has no lane instance: surface species or n > 12). One workgroup
 * up to N = 128, two above: a lane evaluates reactors lane + 64 (block + k blocks), k = 0, 1, ..., one after
 * another in the same rows (N = 100: lanes 0..35 take a second reactor, lanes 36..63 wait masked). nmult, rate_mult,
 * rate_mult_row: per-reactor rate multipliers as the br_opts fields of the same names (nmult = 0: none).
 * du[N][n]; J[N][n][n] row-major, as br_jacobian. */
int br_debug_lane_eval(br_mech* m, int N, const double* T, const double* u, int nmult, const double* rate_mult,
                       const int* rate_mult_row, double* du, double* J);

/* lane-engine check (tests): the register LU and solve of k_lane<nm>, nm = 9 or 12, 1 <= n <= nm (else
 * BR_ERR_INPUT). J, gamma, b, x, fail as br_debug_lu_solve; matrix i sits in lane i mod 64 of workgroup
 * i / 64. piv[N][n]: the pivot row chosen at each step (denseGETRF's p[k]); fail[i] = 0 or (k+1) for a
 * zero pivot (x_i = 0 then). skip[N] (or NULL): a matrix with skip[i] != 0 is left out, its lane idle, and
 * its x, fail and piv entries keep the caller's values. */
int br_debug_lane_lu_solve(int nm, int N, int n, const double* J, const double* gamma, const double* b, const int* skip,
                           double* x, int* fail, int* piv);

/* wavefront-engine check (tests): RHS and analytic Jacobian as k_integrate evaluates them: the
 * mechanism's instance width, its reactors per workgroup on one table block, init_tconst with the
 * multiplier path, the workspace slot layout, J read as the LU reads it. One workgroup up to N = 4 rpb
 * reactors (rpb: br_mech_launch_info of the wavefront engine), two above: a wave evaluates reactors slot,
 * slot + waves, ... one after another in the same LDS block and slot. T_prev[N] (or NULL): the
 * T-only constants are first built at T_prev and used once, then rebuilt at T in the live slot as a
 * temperature-programme run refreshes them. Multipliers as br_debug_lane_eval. Asv may be NULL (1.0). */
int br_debug_wave_eval(br_mech* m, int N, const double* T, const double* Asv, const double* u, const double* T_prev,
                       int nmult, const double* rate_mult, const int* rate_mult_row, double* du, double* J);

/* energy-run check (tests): the right-hand side of the adiabatic instances of k_integrate (br_opts.energy),
 * through their own device functions: du[i] = (du_0 .. du_{ng-1}, dT/dt) at state (u[i], T[i]). The
 * integrator's launch shape, LDS block and workspace slot (one workgroup up to N = 4 rpb reactors, two
 * above, as br_debug_wave_eval), and the refresh path: the constants and the lanes' e_k, cv_k are first built
 * at another temperature, then rebuilt at T in the live slot. T outside [200, 6000] is clamped as in a run.
 * Multipliers as br_debug_lane_eval. BR_ERR_UNSUPPORTED as an energy run. */
int br_debug_energy_eval(br_mech* m, int N, const double* T, const double* u, int nmult, const double* rate_mult,
                         const int* rate_mult_row, double* du /*[N][ng+1]*/);

/* group energy check (tests): the same right-hand side as the energy instance of the group engine evaluates it
 * (k_group<GL, NM, true>, (GL, NM) from ng + 1), through its own device functions, workgroup shape, LDS blocks and
 * global slots. At most two workgroups: each group evaluates its reactors one after another in the same block and
 * slot; the constants and the lanes' e_k, cv_k are first built at another temperature, then rebuilt at T in the
 * live slot (the refresh path). Multipliers as br_debug_lane_eval. BR_ERR_UNSUPPORTED when the mechanism has no
 * group energy instance: ng + 1 > 32, surface species, or more than 32 efficiency sets. Does not read
 * BRHIP_ENGINE. */
int br_debug_group_energy_eval(br_mech* m, int N, const double* T, const double* u, int nmult, const double* rate_mult,
                               const int* rate_mult_row, double* du /*[N][ng+1]*/);

/* temperature-programme check (tests): Tout[i][k] = T(t[i][k]) of reactor i's programme, through the
 * device evaluator the integrator calls (one thread per reactor; consecutive times of a row reuse the
 * cached segment, so ascending and descending sequences both exercise the scan). Host arrays; the
 * programme arguments as the br_opts fields of the same names and checked the same way. */
int br_debug_tprog_eval(int N, int ntprog, const double* tprog_t, const double* tprog_T, int nrows, const int* tprog_row,
                        int nt, const double* t /*[N][nt]*/, double* Tout /*[N][nt]*/);

/* User-defined chemistry: replaces solve(ODEProblem(residual!, u0, (0, tf), params), CVODE_BDF();
 * reltol, abstol, save_everystep=false, callback=FunctionCallingCallback(save_data)) with the userchem
 * residual! (src/BatchReactor.jl:51-54,:197-200,:204-210,:358-360,:371-372). The user's RHS is host
 * code (a Julia or Python function: it cannot run in a kernel), so this runs on the CPU: the same
 * CVODE 5.x restatement as the engine, with CVODE's DQ Jacobian (the reference supplies none).
 * f(user, t, u, du) returns 0 (non-zero ends the solve with BR_ERR_RHS); t is the time CVODE evaluates f
 * at (tn + hg inside the initial-step estimate, the advanced tn in a step); cb(cb_user, t, u) after every
 * accepted step and at t = 0 and t = tf (save_data's rows). u: u0 in, u(tf) out (the last accepted
 * state on failure); stats[BR_NSTAT] as br_stats. Returns 0 or a BR_ERR_* status. No GPU. */
typedef int (*br_rhs_fn)(void* user, double t, const double* u, double* du);
typedef void (*br_step_fn)(void* user, double t, const double* u);
int br_integrate_host(int n, br_rhs_fn f, void* user, double* u, double tf, double rtol, double atol, int max_steps,
                      br_step_fn cb, void* cb_user, double* stats);

/* timing helper for roofline accounting: duration (ms) of the last integrate kernel,
 * measured with HIP events on the stream it was launched on (after the stream syncs). */
int br_last_kernel_ms(br_mech* m, double* ms);

#ifdef __cplusplus
}
#endif
#endif
