// brhip_ctl.hpp -- the CVODE controller of the integrator kernels on the per-reactor LDS block: Ctl, VA,
// cv_set / cv_set_lp, ctl_post_rhs, ctl_post_solve and the difference-quotient Jacobian helpers (dq_*),
// with the CVODE constants, the kernel options (KOpts) and the phase-clock macros (BR_CLK / BR_ACC)
// they share with the three engines.
// Included by brhip.hip (first) and by scripts/micro/cvset_check.hip.
#pragma once
#include "../../include/brhip.h"
#ifndef BR_ASM_MARKS
#define BR_ASM_MARKS 0
#endif
#ifndef BR_PHASE_CLOCKS
#define BR_PHASE_CLOCKS 0   // per-phase shader-clock counters in br_stats (diagnostic build: libbrhip_diag.so)
#endif
#include "brhip_device.hpp"
// Phase clocks of the three engines, one set of macros. A reactor's accumulators (cyc_rhs, cyc_jac, cyc_lu,
// cyc_sol, cyc_ctl) and the origin of its cyc_clk: BR_CLK_BEGIN declares and starts them in one go
// (k_integrate, inside its reactor loop); the persistent loops of the group and lane engines declare
// them once (BR_CLK_VARS) and restart them per reactor (BR_CLK_START()). BR_CLK(v) opens an interval,
// BR_ACC(acc, v) adds it to acc, BR_CLK_STORE(s) writes the clock columns of br_stats s. Product build: no
// accumulators, zeros stored. Diagnostic build: shader clocks. Analysis builds (BR_ASM_MARKS): phase
// markers in the ISA listing instead (they are scheduling barriers).
#if BR_PHASE_CLOCKS
#define BR_CLK_BEGIN                                                                      \
    unsigned long long cyc_rhs = 0, cyc_jac = 0, cyc_lu = 0, cyc_sol = 0, cyc_ctl = 0;    \
    const unsigned long long cyc_all = clock64()
#define BR_CLK_VARS unsigned long long cyc_rhs = 0, cyc_jac = 0, cyc_lu = 0, cyc_sol = 0, cyc_ctl = 0, cyc_all = 0
#define BR_CLK_START() do { cyc_rhs = cyc_jac = cyc_lu = cyc_sol = cyc_ctl = 0; cyc_all = clock64(); } while (0)
#define BR_CLK_STORE(s)                                                                                            \
    do {                                                                                                           \
        (s).cyc_rhs = (double)cyc_rhs; (s).cyc_jac = (double)cyc_jac; (s).cyc_lu = (double)cyc_lu;                 \
        (s).cyc_sol = (double)cyc_sol; (s).cyc_ctl = (double)cyc_ctl; (s).cyc_clk = (double)(clock64() - cyc_all); \
    } while (0)
#define BR_CLK_VALUES (PhaseClk{cyc_rhs, cyc_jac, cyc_lu, cyc_sol, cyc_ctl, cyc_all})
#else
#define BR_CLK_BEGIN
#define BR_CLK_VARS
#define BR_CLK_START()
#define BR_CLK_STORE(s) (s).cyc_rhs = (s).cyc_jac = (s).cyc_lu = (s).cyc_sol = (s).cyc_ctl = (s).cyc_clk = 0.0
#define BR_CLK_VALUES (PhaseClk{})
#endif
// the accumulators by value, for a stats writer outside the kernel's scope (l_store_stats)
struct PhaseClk {
    unsigned long long cyc_rhs, cyc_jac, cyc_lu, cyc_sol, cyc_ctl, cyc_all;
    __device__ __forceinline__ void store(br_stats& s) const { BR_CLK_STORE(s); }
};
// column of a br_stats field in a [N][BR_NSTAT] array of doubles
#define BR_STAT_COL(f) (offsetof(br_stats, f) / sizeof(double))
#if BR_ASM_MARKS
#define BR_CLK(v) asm volatile("; BR_PHASE_BEGIN " #v)
#define BR_ACC(acc, v) asm volatile("; BR_PHASE_END " #acc)
#elif BR_PHASE_CLOCKS
#define BR_CLK(v) const unsigned long long v = clock64()
#define BR_ACC(acc, v) acc += clock64() - v
#else
#define BR_CLK(v)
#define BR_ACC(acc, v)
#endif
// Diagnostic-only instruction-count experiments (scripts/micro/exp_hooks.hpp: a phase run twice,
// extra VALU or memory work per Newton iteration) attach at these points of k_integrate; the
// product build leaves them empty.
#ifdef BR_EXPERIMENT_HOOKS
#include BR_EXPERIMENT_HOOKS
#endif
#ifndef BR_X_AFTER_RHS
#define BR_X_AFTER_RHS()
#define BR_X_AFTER_JAC()
#define BR_X_AFTER_SOLVE()
#define BR_X_AFTER_ITER()
#endif
#ifndef BR_XC_AFTER_CVSET   // ... and inside the controller (cvSet, the step-size ratio root)
#define BR_XC_AFTER_CVSET()
#define BR_XC_AFTER_ETAQ()
#endif
#ifndef BR_XG_AFTER_RHS   // the same for k_group (brhip_group.hpp)
#define BR_XG_AFTER_RHS()
#define BR_XG_AFTER_JAC()
#define BR_XG_AFTER_LU()
#define BR_XG_AFTER_SOLVE()
#endif

using namespace brhip;

namespace {

constexpr int QMAX = 5;
constexpr double HLB_FACTOR = 100.0, HUB_FACTOR = 0.1, H_BIAS = 0.5;
constexpr int MAX_ITERS = 4;
constexpr double ETAMX1 = 10000.0, ETAMX2 = 10.0, ETAMX3 = 10.0, ETAMXF = 0.2, ETAMIN = 0.1, ETACF = 0.25;
constexpr double ADDON = 1e-6, BIAS1 = 6.0, BIAS2 = 6.0, BIAS3 = 10.0, ONEPSM = 1.000001;
constexpr int SMALL_NST = 10, MXNCF = 10, MXNEF = 7, MXNEF1 = 3, SMALL_NEF = 2, LONG_WAIT = 10;
constexpr int NLS_MAXCOR = 3, MSBP = 20, LS_MSBJ = 51;
constexpr double CRDOWN = 0.3, DGMAX = 0.3, RDIV = 2.0, CORTES = 0.1, THRESH = 1.5, FUZZ = 100.0, LS_DGMAX = 0.2;
constexpr double UROUND = 2.220446049250313e-16;
enum { FIRST_CALL = 0, PREV_CONV_FAIL = 1, PREV_ERR_FAIL = 2 };
enum { NO_FAILURES = 0, FAIL_BAD_J = 1, FAIL_OTHER = 2 };

struct KOpts {
    double rtol, atol, hmax_inv, ufac;
    int max_steps, trace_cap;
    int ign;                  // gas species index of the ignition marker (-1: not tracked)
    int nout;                 // dense output: tout[nout] (device), yout[N][nout][n] (device)
    const double* tout;
    double* yout;
    int dq_jac;               // CVODE's DQ Jacobian (br_opts.dq_jacobian) instead of the analytic one (both engines)
    int defer_steps;          // k_lane: hand a reactor still running after this many steps to the
                              // wavefront engine (restart from u0); >= max_steps disables
    const int* rid_list;      // k_integrate: integrate reactors rid_list[0 .. min(*rid_count, N)) only
    const int* rid_count;
    const double* rid_t0;     // with rid_list: start time of list entry i (a deferred lane reactor
                              // continues from its last accepted state U[rid] at rid_t0[i]: CVODE
                              // restart there) and its counters so far are in stats[rid]
    int* work;                // k_integrate: persistent waves take reactor indices from this
                              // counter (nullptr: one reactor per wave, index = wave slot)
};
// Per-reactor output grids (br_opts.tout_per_reactor: tout[N][nout], one row per reactor, NaN = no output
// as trailing padding) ride in bit 0 of KOpts::tout -- the array is 8-byte aligned -- and not in a field
// or kernel argument of their own: either moves the kernel arguments, and that alone changed the
// register allocation of kernels that never read it. tout is read only under the nout guards, so a
// run without outputs never sees the tag.
inline const double* tout_tag(const double* tout, bool per_reactor) {
    return reinterpret_cast<const double*>(reinterpret_cast<size_t>(tout) | (per_reactor ? 1u : 0u));
}
// output time io of the reactor whose yout row index is orow = rid * nout + io: entry io of the shared
// grid, or entry orow of the [N][nout] array (the index the yout row already needs)
// (OPAQUE, the group engines: the wave-uniform tagged pointer goes through an opaque scalar copy at each
// use. Without it the compiler decodes the tag once in k_group's prologue, outside the nout guards, and
// the SGPRs that holds across the whole kernel, which is at the SGPR limit, shift its spills: the
// no-output instruction stream then differs from the parent's in four times as many places. In the
// wavefront and lane kernels the copy costs scratch instead, so they go without)
template <bool OPAQUE>
__device__ __forceinline__ size_t tout_bits(size_t b) {
    if constexpr (OPAQUE) asm volatile("" : "+s"(b));
    return b;
}
template <bool OPAQUE = false, class P>
__device__ __forceinline__ double tout_at(P tagged, size_t orow, int io) {
    const size_t b = tout_bits<OPAQUE>((size_t)tagged);
    return reinterpret_cast<P>(b & ~(size_t)1)[(b & 1) ? orow : (size_t)io];
}
template <bool OPAQUE = false, class P>
__device__ __forceinline__ bool tout_per_reactor(P tagged) { return (tout_bits<OPAQUE>((size_t)tagged) & 1) != 0; }
// the preludes' test "output io is at t <= t0" (it gets u0). Shared grid: !(t > t0), as ever. Per-reactor
// grid: t <= t0, which a NaN (no output) fails, so that the prelude writes no u0 for it and stops
template <bool OPAQUE = false, class P>
__device__ __forceinline__ bool tout_pre(P tagged, size_t orow, int io, double t0) {
    const double t = tout_at<OPAQUE>(tagged, orow, io);
    return tout_per_reactor<OPAQUE>(tagged) ? t <= t0 : !(t > t0);
}

// ------------------------------------------------------------------------------------
// per-reactor LDS block: [Ctl: CVODE's cv_mem scalars][Vec: per-lane vectors][Smem: rate work]
//
// The kernel keeps only the hot path inline (RHS, Jacobian, LU, solve). All step control lives
// in two __noinline__ functions that read and write this block through address-space-3
// pointers, so their register allocation is isolated from the hot path's (no spills there, and
// the VGPR file stays free for the row-per-lane Newton matrix). Every lane writes the same
// uniform value; reads go through readfirstlane, so branches on them are scalar.
// ------------------------------------------------------------------------------------
struct Ctl {
    double p_last;
    double tau[QMAX + 2], tq[6], l[QMAX + 1];
    double tn, h, rl1, gamma, gamrat, gammap, crate, delp;
    double hprime, hscale, eta, etamax, acnrm, saved_tq5, saved_t, tol;
    double hg, hub, hlb, hnew, ulimit, tstop;
    int q, qprime, L, qwait;
    int nst, nfe, nsetups, nje, nni, ncfn, netf, nstlp, nstlj;
    int ncf, nef, nstloc, status, m_it, convfail, count1, phase;
    int callSetup, jbad, jcur_nls, hnewOK, newj;
    // ignition marker (max dX_ign/dt over accepted steps) and dense-output cursor
    double ign_x, ign_t, ign_rate, t_ign, ign_dt;
    double dq_mininc;         // CVODE's DQ Jacobian: minInc of the Jacobian being built
    int nfe_dq;               // RHS evaluations of the DQ Jacobian (CVODE's nfeDQ)
    int iout;
    // per-launch constants (here rather than in registers: they are read once per step)
    double a_rtol, a_atol, a_hmax_inv, a_ufac;
    double* a_trace;
    const double* a_tout;
    double* a_yout;
    int a_max_steps, a_trace_cap, a_rid, a_n, a_ign, a_nout;
};
// (the RHS takes the start of a reactor's LDS block as its p_last)
static_assert(offsetof(Ctl, p_last) == 0, "Ctl::p_last is the first field of a reactor's LDS block");
constexpr int CTL_BYTES = (sizeof(Ctl) + 15) / 16 * 16;
enum { V_Z0 = 0, V_ACOR = QMAX + 1, V_EWT, V_TEMP, V_Y, NVEC };   // z0..z5, acor, ewt, tempv, y
// V[vec * 64 + lane] for the first component slot. Two components per lane (n = 65..72): slot 1 of
// vector j (components 64..71, lanes 0..7) at V1OFF + 8 j + lane; lanes 8..63 of slot 1 (components
// 72..127, never real) at V1OFF + 8 j + 72 + lane, a dump region whose entries alias only each other.
// Every access is then base + per-lane constant + 8 j (an immediate): no per-vector select that
// the compiler would hoist out of the integrator loop and keep live (40 VGPRs spilled at 3 waves/
// SIMD with the previous 72-wide rows and one shared dump row). 6.6 KB per gas+surface reactor.
constexpr int V1OFF = NVEC * 64;
// BR_VS32 = 1: k_integrate<32> (16 < n <= 32) keeps its vectors 32 wide (VS = 32): lanes 32..63 hold
// no component, read the entry of lane - 32 (a finite value every use of theirs masks: norms, maxima
// and outputs test component < n) and never store (VProxy below). 2.5 KB less LDS per reactor.
#ifndef BR_VS32
#define BR_VS32 1
#endif
__host__ __device__ constexpr int vec_stride(int nmax) { return (BR_VS32 && nmax == 32) ? 32 : 64; }
__host__ __device__ constexpr int nmax_of(int n) { return n <= 16 ? 16 : (n <= 32 ? 32 : (n <= 56 ? 56 : (n <= 64 ? 64 : 72))); }
__host__ __device__ inline int vec_bytes(int cpl, int vs = 64) {
    return cpl == 2 ? (V1OFF + 8 * (NVEC - 1) + 72 + 64) * 8 : NVEC * vs * 8;
}
typedef __attribute__((address_space(3))) double LDbl;
// an entry of a VS < 64 vector: loads by every lane, stores by lanes < VS only
struct VProxy {
    LDbl* a;
    bool w;
    __device__ __forceinline__ operator double() const { return *a; }
    __device__ __forceinline__ VProxy& operator=(double x) { if (w) *a = x; return *this; }
    __device__ __forceinline__ VProxy& operator=(const VProxy& o) { return *this = (double)o; }
    __device__ __forceinline__ VProxy& operator+=(double x) { return *this = (double)*this + x; }
    __device__ __forceinline__ VProxy& operator-=(double x) { return *this = (double)*this - x; }
    __device__ __forceinline__ VProxy& operator*=(double x) { return *this = (double)*this * x; }
};
// Nordsieck / work vectors in the reactor's LDS block: V.at(vec, s) = component lane + 64 s of
// vector vec. (Register-resident vectors stored to LDS around each Newton setup measured GRI
// -1.1 %, surf -11 % in round 2: the extra VGPRs cost occupancy.)
template <int CPL, int GW = 64, int VS = GW>
struct VA {
    typedef __attribute__((address_space(3))) double LD;
    LD* p;
    int lane;
    __device__ __forceinline__ decltype(auto) at(int j, int s) const {
        if constexpr (VS < GW) {
            static_assert(CPL == 1, "narrow vectors: one component per lane");
            // lanes >= VS read a real entry (lane - VS for a power-of-2 width, else the last one)
            const int li = (VS & (VS - 1)) == 0 ? (lane & (VS - 1)) : (lane < VS ? lane : VS - 1);
            return VProxy{&p[j * VS + li], lane < VS};
        } else {
            if (CPL == 1 || s == 0) return static_cast<LD&>(p[j * GW + lane]);
            return static_cast<LD&>(p[V1OFF + 8 * j + (lane < 8 ? lane : 72 + lane)]);
        }
    }
};
template <int CPL, int GW = 64> using VT = VA<CPL, GW>;
// component slot s's value of vector j for a uniform j in [0, QMAX + 1] (register arrays cannot be
// indexed dynamically: a select chain, scalar branches on the uniform j)
template <int CPL, class V_>
__device__ __forceinline__ double vget(V_& V, int j, int s) {
    double r = 0.0;
#pragma unroll
    for (int jj = 0; jj <= QMAX + 1; ++jj) if (jj == j) r = V.at(jj, s);
    return r;
}
template <int CPL, class V_>
__device__ __forceinline__ void vset(V_& V, int j, int s, double x) {
#pragma unroll
    for (int jj = 0; jj <= QMAX + 1; ++jj) if (jj == j) V.at(jj, s) = x;
}
typedef __attribute__((address_space(3))) Ctl LCtl;

__host__ __device__ inline size_t reactor_bytes(const DevMech& M) {
    return CTL_BYTES + vec_bytes(M.cpl, vec_stride(nmax_of(M.n))) + (size_t)M.rblock_bytes;
}
__host__ __device__ inline size_t wg_lds_bytes(const DevMech& M, int rpb) { return M.img_bytes + rpb * reactor_bytes(M); }
// per-reactor global workspace (doubles): saved J, LU factors, Jacobian scratch (2 per gas rxn);
// matrix columns hold 64 * CPL rows (CPL = 2 for nmax > 64)
__host__ __device__ inline int col_rows(int nmax) { return nmax > 64 ? CR2 : 64; }   // CR2 = 80 (lu_factor2)
// factors + D^-1: CPL = 1 NMAX columns of NMAX rows + 64 (lu_factor), CPL = 2 NMAX + 1 columns of CR2 rows
__host__ __device__ inline size_t lu_ws_doubles(int nmax) {
    return nmax > 64 ? (size_t)(nmax + 1) * CR2 : (size_t)nmax * nmax + WAVE;
}
// [J | LU factors, aliased by the Jacobian scratch (2 per gas reaction) | RXD: {kf, kr} per gas
// reaction]. The scratch is live only while a new J is built, and every new J is followed by a
// factorization that overwrites the old factors, so the two share one region (-5.2 KB per GRI
// slot; with NMAX-row factor columns 4096 slots of 60 KB = 245 MB against the 256 MB Infinity Cache).
__host__ __device__ inline size_t lu_area_doubles(int nmax, int nrg) {
    const size_t a = lu_ws_doubles(nmax), b = (((size_t)2 * nrg + 63) / 64) * 64;
    return a > b ? a : b;
}
__host__ __device__ inline size_t rxd_ws_off(int nmax, int nrg) {
    return (size_t)nmax * col_rows(nmax) + lu_area_doubles(nmax, nrg);
}
__host__ __device__ inline size_t ws_doubles(int nmax, int nrg) {
    return rxd_ws_off(nmax, nrg) + (((size_t)2 * nrg + 63) / 64) * 64;
}

struct WaveCtx {
    int wave, lane, rid;
    Tab tb;
    char* rbase;   // this wave's reactor block
    RView R;
};
// ws: the global workspace, NMAX-instance slots (slot = wave index rid)
template <int CPL, int NMAX>
__device__ __forceinline__ WaveCtx wave_ctx(const DevMech& M, char* smem, int rpb, double* ws) {
    WaveCtx w;
    w.wave = uni((int)(threadIdx.x >> 6));   // uniform per wave: scalar addressing of its reactor
    w.lane = threadIdx.x & 63;
    w.rid = blockIdx.x * rpb + w.wave;
    stage_tables(M, smem);
    w.tb = tab_view<CPL>(smem, M);
    w.rbase = smem + M.img_bytes + (size_t)w.wave * reactor_bytes(M);
    // (the vector width follows n, as reactor_bytes: the rates / Jacobian kernels run as NMAX 64)
    w.R = rview<CPL>(w.rbase + CTL_BYTES + vec_bytes(CPL, vec_stride(nmax_of(M.n))), M,
                     launder(ws + (size_t)w.rid * ws_doubles(NMAX, M.nrg) + rxd_ws_off(NMAX, M.nrg)));
    return w;
}

// loads from the LDS controller: ints through v_readfirstlane (SGPRs: scalar branches and loop
// bounds); doubles stay in VGPRs (every lane reads the same value; fp64 arithmetic runs on the VALU
// either way, and the two readfirstlanes per value were VALU instructions of their own: GRI +0.7 %,
// surface-only +2.7 %, round 3)
__device__ __forceinline__ double ud(const LDbl& x) { return (double)x; }
__device__ __forceinline__ int ui(const __attribute__((address_space(3))) int& x) { return uni((int)x); }
// Reactor groups: the wavefront engine runs one reactor per wave (group width GW = 64); the group
// engines (brhip_group.hpp) two or four per wave, one per 32-lane half or 16-lane DPP row (GW = 32 /
// 16), with `lane` the lane within the group. The controller's values are uniform per group: scalar
// for GW = 64 (readfirstlane: SGPRs, scalar branches), per-lane VGPRs with exec-masked branches for
// GW < 64; reductions and broadcasts over the group (DPP row butterflies, permlane16 swaps between
// the rows of a half, ds_bpermute inside the group).
template <int GW>
__device__ __forceinline__ int gui(const __attribute__((address_space(3))) int& x) {
    if constexpr (GW == 64) return uni((int)x);
    else return (int)x;
}
template <int GW>
__device__ __forceinline__ int guni(int v) {
    if constexpr (GW == 64) return uni(v);
    else return v;
}
template <int GW>
__device__ __forceinline__ double guni(double v) {
    if constexpr (GW == 64) return uni(v);
    else return v;
}
template <int GW>
__device__ __forceinline__ double gsum(double v) {
    if constexpr (GW == 64) return wave_sum(v);
    else if constexpr (GW == 32) return half_sum(v);
    else return row_sum(v);
}
template <int GW>
__device__ __forceinline__ double gmax(double v) {
    if constexpr (GW == 64) return wave_max(v);
    else if constexpr (GW == 32) return half_max(v);
    else return row_max(v);
}
// value of v in lane k of the group (k uniform per group)
template <int GW>
__device__ __forceinline__ double gbcast(double v, int k) {
    if constexpr (GW == 64) return bcast(v, k);
    else return lane_pull(v, (int)(threadIdx.x & (64 - GW)) + k);
}

// analysis builds (BR_ASM_QMARKS): region markers in the 16-lane controller's ISA listing
#ifdef BR_ASM_QMARKS
#define BR_QMARK(name) do { if constexpr (GW == 16) asm volatile("; QMARK " #name); } while (0)
#else
#define BR_QMARK(name) do { } while (0)
#endif
#ifndef BR_CTL_INLINE
#define BR_CTL_INLINE __forceinline__
#endif
enum { PH_F0 = 0, PH_HIN = 1, PH_NEWTON = 2, PH_EF1 = 3 };
// action codes returned by the controller to the hot loop
enum { A_RHS = 0, A_SOLVE = 1, A_SETUP = 2, A_DONE = 3 };

// wrms norm of the lane's component values (components lane + 64 s) with weights ewt
template <int CPL, int GW = 64>
__device__ __forceinline__ double wrms_l(const double (&v)[CPL], const double (&ewt)[CPL], int lane, int n) {
    double acc = 0.0;
#pragma unroll
    for (int s = 0; s < CPL; ++s) {
        const double t = (lane + 64 * s < n) ? v[s] * ewt[s] : 0.0;
        acc += t * t;
    }
    return guni<GW>(sqrt(gsum<GW>(acc) / n));
}
// per-component slot loops over the lane's components c = lane + 64 s
#define FOR_S for (int s = 0; s < CPL; ++s)
#define CS (lane + 64 * s)

struct CtlArgs {   // per-launch constants the controller needs, read (uniform) from the LDS controller
    double rtol, atol, hmax_inv, ufac;
    // (global-address-space pointers: generic ones compile to flat accesses, which count on both the
    // memory and the LDS counter and make the waitcnt pass fall back to full waits after them)
    BR_GLOBAL double* trace;
    const BR_GLOBAL double* tout;
    BR_GLOBAL double* yout;
    int max_steps, trace_cap, rid, n, ign, nout;
};
// uniform 64-bit pointer from the LDS controller
template <class P>
__device__ __forceinline__ P ld_ptr(const __attribute__((address_space(3))) P& f) {
    const volatile __attribute__((address_space(3))) unsigned long long& tp =
        *reinterpret_cast<const volatile __attribute__((address_space(3))) unsigned long long*>(&f);
    const unsigned long long tv = tp;
    const unsigned lo = (unsigned)uni((int)(tv & 0xffffffffull)), hi = (unsigned)uni((int)(tv >> 32));
    return reinterpret_cast<P>(((unsigned long long)hi << 32) | lo);
}
template <int GW = 64>
__device__ __forceinline__ CtlArgs load_args(LCtl* C) {
    CtlArgs a;
    a.rtol = ud(C->a_rtol); a.atol = ud(C->a_atol); a.hmax_inv = ud(C->a_hmax_inv); a.ufac = ud(C->a_ufac);
    a.trace = launder(ld_ptr(C->a_trace));
    a.tout = launder(ld_ptr(C->a_tout));
    a.yout = launder(ld_ptr(C->a_yout));
    a.max_steps = gui<GW>(C->a_max_steps); a.trace_cap = gui<GW>(C->a_trace_cap); a.rid = gui<GW>(C->a_rid); a.n = gui<GW>(C->a_n);
    a.ign = gui<GW>(C->a_ign); a.nout = gui<GW>(C->a_nout);
    return a;
}

// mole fraction of gas species k in state v (components lane + 64 s): (v_k/M_k) / sum_j v_j/M_j
template <int CPL, int GW = 64>
__device__ __forceinline__ double mole_frac_of(const double (&v)[CPL], int lane, int k) {
    const double* mw = reinterpret_cast<const double*>(br_lds);   // staged molwt[] (image offset 0)
    const int ng = MF(ng);
    double g = 0.0, c0 = 0.0, c1 = 0.0;
#pragma unroll
    FOR_S if (CS < ng) { const double c = v[s] / mw[CS]; g += c; if (s == 0) c0 = c; else c1 = c; }
    const double ck = (k < 64) ? gbcast<GW>(c0, k) : gbcast<GW>(c1, k - 64);   // k uniform: one readlane pair
    return ck / gsum<GW>(g);
}
// ignition marker after an accepted step to (tn, v): midpoint of the step with the largest dX/dt
template <int CPL, int GW = 64>
__device__ __forceinline__ void track_ignition(LCtl* C, const CtlArgs& a, int lane, double tn, const double (&v)[CPL]) {
    const double x = guni<GW>(mole_frac_of<CPL, GW>(v, lane, a.ign));
    const double t0 = ud(C->ign_t), xp = ud(C->ign_x), rate = ud(C->ign_rate);
    const double dt = tn - t0;   // > 0 (accepted step): compare without the division, divide on a new max
    if (x - xp > rate * dt) {
        const double r = (x - xp) / dt;
        if (r > rate) { C->ign_rate = r; C->t_ign = 0.5 * (t0 + tn); C->ign_dt = dt; }
    }
    C->ign_x = x; C->ign_t = tn;
}
// dense output (CVode CV_NORMAL): every tout in (t_{n-1}, t_n] from the Nordsieck array of the step
// just completed, y(t) = sum_j z_j ((t - tn)/h)^j (CVodeGetDky, k = 0)
// (EN, the energy instances: a.n = ng + 1, the yout rows keep ng entries, lane ng's value -- T -- goes to
// T_out[orow], which rides in a.trace: an energy run takes no trace)
template <int CPL, int GW = 64, int VS = GW, bool EN = false>
__device__ __forceinline__ void dense_output(LCtl* C, VA<CPL, GW, VS>& V, const CtlArgs& a, int lane, double tn, double h, int q,
                                             double tlim) {
    int io = gui<GW>(C->iout);
    while (io < a.nout) {
        // (per-reactor grids: the time sits at the yout row's own index, tout_at; a NaN there -- no
        // output -- fails the comparison and ends this reactor's outputs for good)
        const size_t orow = (size_t)a.rid * a.nout + io;
        const double t = guni<GW>(tout_at<(GW < 64)>(a.tout, orow, io));
        if (!(t <= tlim)) break;
        const double sk = (t - tn) / h;
        auto row = a.yout + orow * (EN ? a.n - 1 : a.n);
#pragma unroll
        FOR_S {
            double yv = vget<CPL>(V, q, s);
#pragma unroll
            for (int j = QMAX - 1; j >= 0; --j) if (j < q) yv = V.at(j, s) + sk * yv;
            if constexpr (EN) {
                if (CS < a.n - 1) row[CS] = yv;
                else if (CS == a.n - 1 && a.trace) a.trace[orow] = yv;
            } else {
                if (CS < a.n) row[CS] = yv;
            }
        }
        ++io;
    }
    C->iout = io;
}

// 1.0 / j for the small integers of the BDF coefficient formulas (exactly the rounded quotient)
// (j is in 1 .. QMAX + 1 at every call site; no run-time division for the impossible rest: with
// per-lane j it was evaluated on every call, ~11 VALU each)
__device__ __forceinline__ double inv_int(int j) {
    return j == 1 ? 1.0 : j == 2 ? 0.5 : j == 3 ? 1.0 / 3.0 : j == 4 ? 0.25 : j == 5 ? 0.2 : 1.0 / 6.0;
}

// the controller scalars one attempt (predict + cvSet) reads, loaded in one batch before the
// prediction's Nordsieck stores (V shares LDS with the controller: a load after a V store waits)
struct AttemptIn {
    int q, qwait, nst, nstlp;
    double h, tn, tstop, gammap;
    double tau[QMAX + 2];
};
template <int GW = 64>
__device__ __forceinline__ AttemptIn load_attempt(LCtl* C) {
    AttemptIn in;
    in.q = gui<GW>(C->q); in.qwait = gui<GW>(C->qwait); in.nst = gui<GW>(C->nst); in.nstlp = gui<GW>(C->nstlp);
    in.h = ud(C->h); in.tn = ud(C->tn); in.tstop = ud(C->tstop); in.gammap = ud(C->gammap);
#pragma unroll
    for (int i = 0; i < QMAX + 2; ++i) in.tau[i] = ud(C->tau[i]);
    return in;
}
// cvSet (BDF coefficients l[], tq[], gamma) for the current q, h, tau
template <int GW = 64>
__device__ __forceinline__ void cv_set(LCtl* C, const AttemptIn& in, double& tq4_out, double& gamrat_out) {
    const int q = in.q, qwait = in.qwait, nst = in.nst;
    const double h = in.h;
    double lv[QMAX + 1] = {1.0, 1.0, 0.0, 0.0, 0.0, 0.0};
    double tau[QMAX + 2];
#pragma unroll
    for (int i = 0; i < QMAX + 2; ++i) tau[i] = in.tau[i];
    // h / hsum_m for every m up front (hsum_m = h + tau[1] + ... + tau[m-1], summed in CVODE's
    // order): the divisions are independent, so they overlap instead of forming a chain
    double xinv[QMAX + 2];
    {
        double hs = h;
#pragma unroll
        for (int m = 2; m <= QMAX + 1; ++m) {
            hs += tau[m - 1];
            xinv[m] = h / hs;
        }
    }
    // element m of a small local array for a uniform m: a select chain over opaque copies (written
    // as a plain chain, the compiler turns it back into a dynamically indexed array in scratch
    // memory: a global-memory round trip on every cv_set)
    auto pick = [&](const double* arr, int lo, int hi, int m) {
        double v = arr[lo];
#pragma unroll
        for (int i = lo + 1; i <= QMAX + 1; ++i) {
            if (i <= hi) {
                double x = arr[i];
                asm volatile("" : "+v"(x));
                v = (m == i) ? x : v;
            }
        }
        return v;
    };
    auto xinv_at = [&](int m) { return pick(xinv, 2, QMAX + 1, m); };   // uniform m in [2, QMAX + 1]
    double xi_inv = 1.0, xistar_inv = 1.0, alpha0 = -1.0, alpha0_hat = -1.0;
    if (q > 1) {
#pragma unroll
        for (int j = 2; j < QMAX; ++j) {
            if (j < q) {
                alpha0 -= inv_int(j);
#pragma unroll
                for (int i = QMAX; i >= 1; --i) if (i <= j) lv[i] += lv[i - 1] * xinv[j];
            }
        }
        alpha0 -= inv_int(q);
        xistar_inv = -lv[1] - alpha0;
        xi_inv = xinv_at(q);
        alpha0_hat = -lv[1] - xi_inv;
#pragma unroll
        for (int i = QMAX; i >= 1; --i) if (i <= q) lv[i] += lv[i - 1] * xistar_inv;
    }
#pragma unroll
    for (int i = 0; i <= QMAX; ++i) C->l[i] = lv[i];
    const double A1 = 1.0 - alpha0_hat + alpha0;
    const double A2 = 1.0 + q * A1;
    const double lq = pick(lv, 1, QMAX, q);
    const double tq2 = fabs(A1 / (alpha0 * A2));
    C->tq[2] = tq2;
    C->tq[5] = fabs(A2 * xistar_inv / (lq * xi_inv));
    if (qwait == 1) {
        if (q > 1) {
            const double Cc = xistar_inv / lq;
            const double A3 = alpha0 + inv_int(q);
            const double A4 = alpha0_hat + xi_inv;
            const double Cpinv = (1.0 - A4 + A3) / A3;
            C->tq[1] = fabs(Cc * Cpinv);
        } else C->tq[1] = 1.0;
        xi_inv = xinv_at(q + 1);   // h / (h + tau[1] + ... + tau[q])
        const double A5 = alpha0 - inv_int(q + 1);
        const double A6 = alpha0_hat - xi_inv;
        const double Cppinv = (1.0 - A6 + A5) / A2;
        C->tq[3] = fabs(Cppinv / (xi_inv * (q + 2) * A5));
    }
    tq4_out = CORTES / tq2;
    C->tq[4] = tq4_out;
    const double rl1 = 1.0 / lv[1];
    C->rl1 = rl1;
    const double gamma = h * rl1;
    C->gamma = gamma;
    if (nst == 0) C->gammap = gamma;
    gamrat_out = (nst > 0) ? gamma / in.gammap : 1.0;
    C->gamrat = gamrat_out;
}

// cvSet in every engine (cv_set_lp): cv_set's operations, with the independent divisions spread over
// the lanes of each 16-lane DPP row -- lane t computes one quotient and a row broadcast
// (row_newbcast) hands it to the row (a 16-lane group is one row; in 32- and 64-lane groups every
// row computes the same quotients), 3 division sequences instead of 14 -- and the order masks of the
// l recurrences folded into zero coefficients (exact: every l_i is >= 0 and finite, so
// l_i + l_{i-1} * 0 = l_i). cv_set was 19 % of C2's VALU instructions and 7.1 % of GRI's
// (profiles/r06_quad_valu_split.json). On the same inputs it returns cv_set's bits
// (scripts/micro/cvset_check.hip, 8192 random states), and the wavefront engine's trajectories are
// bit-identical to the cv_set build (GRI, surface-only, gas + surface); inside k_group the compiler
// fuses multiplies and adds of the surrounding code differently, so C2 trajectories move by
// rounding (< 0.5 band against the cv_set build, parity windows unchanged).
template <int K>
__device__ __forceinline__ double row_lane(double v) { return dppd<0x150 + K>(v); }
__device__ __forceinline__ double sel6(int t, double v0, double v1, double v2, double v3, double v4, double v5) {
    // lane t's operand (opaque copies: a select chain, not a private array in scratch memory)
    double v = v0;
    const double c[5] = {v1, v2, v3, v4, v5};
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        double x = c[i];
        asm volatile("" : "+v"(x));
        v = (t == i + 1) ? x : v;
    }
    return v;
}
__device__ __forceinline__ void cv_set_lp(LCtl* C, const AttemptIn& in, double& tq4_out, double& gamrat_out) {
    const int t = (int)(threadIdx.x & 15);
    const int q = in.q, qwait = in.qwait, nst = in.nst;
    const double h = in.h;
    // h / hsum_m, hsum_m = h + tau[1] + ... + tau[m-1] in CVODE's order, m = 2 .. QMAX + 1: lane m - 2
    double hsum[QMAX + 2];
    {
        double hs = h;
#pragma unroll
        for (int m = 2; m <= QMAX + 1; ++m) {
            hs += in.tau[m - 1];
            hsum[m] = hs;
        }
    }
    const double xq = h / sel6(t, hsum[2], hsum[3], hsum[4], hsum[5], hsum[6], hsum[6]);
    double xinv[QMAX + 2];
    xinv[0] = xinv[1] = 0.0;
    xinv[2] = row_lane<0>(xq); xinv[3] = row_lane<1>(xq); xinv[4] = row_lane<2>(xq);
    xinv[5] = row_lane<3>(xq); xinv[6] = row_lane<4>(xq);
    auto pick = [&](const double* arr, int lo, int hi, int m) {
        double v = arr[lo];
#pragma unroll
        for (int i = lo + 1; i <= QMAX + 1; ++i) {
            if (i <= hi) {
                double x = arr[i];
                asm volatile("" : "+v"(x));
                v = (m == i) ? x : v;
            }
        }
        return v;
    };
    double lv[QMAX + 1] = {1.0, 1.0, 0.0, 0.0, 0.0, 0.0};
    double xi_inv = 1.0, xistar_inv = 1.0, alpha0 = -1.0, alpha0_hat = -1.0;
    if (q > 1) {
#pragma unroll
        for (int j = 2; j < QMAX; ++j) {
            const bool on = j < q;
            const double c = on ? xinv[j] : 0.0;
            alpha0 -= on ? inv_int(j) : 0.0;
#pragma unroll
            for (int i = QMAX; i >= 1; --i) if (i <= j) lv[i] += lv[i - 1] * c;
        }
        alpha0 -= inv_int(q);
        xistar_inv = -lv[1] - alpha0;
        xi_inv = pick(xinv, 2, QMAX + 1, q);
        alpha0_hat = -lv[1] - xi_inv;
        // no order mask: l_i = 0 for i >= q here, and the descending sweep reads each l_{i-1} before
        // updating it, so every l_i with i > q stays 0 (0 + 0 * xistar_inv)
#pragma unroll
        for (int i = QMAX; i >= 1; --i) lv[i] += lv[i - 1] * xistar_inv;
    }
#pragma unroll
    for (int i = 0; i <= QMAX; ++i) C->l[i] = lv[i];
    const double A1 = 1.0 - alpha0_hat + alpha0;
    const double A2 = 1.0 + q * A1;
    const double lq = pick(lv, 1, QMAX, q);
    // round 1, lane t: 0 tq2, 1 tq5, 2 1/l_1, 3 Cc, 4 Cpinv, 5 Cppinv (3..5 used when qwait == 1)
    const double A3 = alpha0 + inv_int(q);
    const double A4 = alpha0_hat + xi_inv;
    const double xi1 = pick(xinv, 2, QMAX + 1, q + 1);   // h / (h + tau[1] + ... + tau[q])
    const double A5 = alpha0 - inv_int(q + 1);
    const double A6 = alpha0_hat - xi1;
    const double num = sel6(t, A1, A2 * xistar_inv, 1.0, xistar_inv, 1.0 - A4 + A3, 1.0 - A6 + A5);
    const double den = sel6(t, alpha0 * A2, lq * xi_inv, lv[1], lq, A3, A2);
    const double r1 = num / den;
    const double tq2 = fabs(row_lane<0>(r1));
    const double rl1 = row_lane<2>(r1);
    const double Cc = row_lane<3>(r1), Cpinv = row_lane<4>(r1), Cppinv = row_lane<5>(r1);
    C->tq[2] = tq2;
    C->tq[5] = fabs(row_lane<1>(r1));
    C->rl1 = rl1;
    const double gamma = h * rl1;
    C->gamma = gamma;
    if (nst == 0) C->gammap = gamma;
    // round 2, lane t: 0 tq4, 1 tq3's quotient, 2 gamrat
    const double r2 = sel6(t, CORTES, Cppinv, gamma, 1.0, 1.0, 1.0) /
                      sel6(t, tq2, xi1 * (q + 2) * A5, in.gammap, 1.0, 1.0, 1.0);
    tq4_out = row_lane<0>(r2);
    C->tq[4] = tq4_out;
    if (qwait == 1) {
        C->tq[1] = (q > 1) ? fabs(Cc * Cpinv) : 1.0;
        C->tq[3] = fabs(row_lane<1>(r2));
    }
    gamrat_out = (nst > 0) ? row_lane<2>(r2) : 1.0;
    C->gamrat = gamrat_out;
}

// Nordsieck rescale of z[1..q] by eta^j; h = hscale*eta
template <int CPL, int GW = 64, int VS = GW>
__device__ __forceinline__ void cv_rescale(LCtl* C, VA<CPL, GW, VS>& V, int lane) {
    const int q = gui<GW>(C->q);
    const double eta = ud(C->eta), hscale = ud(C->hscale);
    double f = eta;
#pragma unroll
    for (int j = 1; j <= QMAX; ++j) {
        if (j <= q) {
#pragma unroll
            FOR_S V.at(j, s) *= f;
            f *= eta;
        }
    }
    const double h = hscale * eta;
    C->h = h; C->hscale = h;
}
// prediction (tn += h, Pascal triangle on z) and its inverse
template <int CPL, int GW = 64, int VS = GW>
__device__ __forceinline__ void cv_predict(LCtl* C, VA<CPL, GW, VS>& V, int lane, const AttemptIn& in) {
    const int q = in.q;
    double tn = in.tn + in.h;
    const double tstop = in.tstop;
    if ((tn - tstop) * in.h > 0) tn = tstop;
    C->tn = tn;
#pragma unroll
    FOR_S {
        double z[QMAX + 1];
#pragma unroll
        for (int j = 0; j <= QMAX; ++j) z[j] = V.at(j, s);
#pragma unroll
        for (int k = 1; k <= QMAX; ++k)
#pragma unroll
            for (int j = QMAX; j >= k; --j)
                if (j <= q && k <= q) z[j - 1] += z[j];
#pragma unroll
        for (int j = 0; j < QMAX; ++j) V.at(j, s) = z[j];
    }
}
template <int CPL, int GW = 64, int VS = GW>
__device__ __forceinline__ void cv_restore(LCtl* C, VA<CPL, GW, VS>& V, int lane) {
    const int q = gui<GW>(C->q);
    C->tn = ud(C->saved_t);
#pragma unroll
    FOR_S {
        double z[QMAX + 1];
#pragma unroll
        for (int j = 0; j <= QMAX; ++j) z[j] = V.at(j, s);
#pragma unroll
        for (int k = 1; k <= QMAX; ++k)
#pragma unroll
            for (int j = QMAX; j >= k; --j)
                if (j <= q && k <= q) z[j - 1] -= z[j];
#pragma unroll
        for (int j = 0; j < QMAX; ++j) V.at(j, s) = z[j];
    }
}
// cvAdjustOrder for BDF (zn[L] from zn[qmax] = indx_acor on increase)
template <int CPL, int GW = 64, int VS = GW>
__device__ __forceinline__ void cv_adjust_order(LCtl* C, VA<CPL, GW, VS>& V, int lane, int dq) {
    const int q = gui<GW>(C->q);
    if (q == 2 && dq != 1) return;
    double lv[QMAX + 1] = {0.0, 0.0, 1.0, 0.0, 0.0, 0.0};
    const double hscale = ud(C->hscale);
    if (dq == 1) {
        double alpha1 = 1.0, prod = 1.0, xiold = 1.0, alpha0 = -1.0, hsum = hscale;
        for (int j = 1; j < q; ++j) {
            hsum += ud(C->tau[j + 1]);
            const double xi = hsum / hscale;
            prod *= xi;
            alpha0 -= inv_int(j + 1);
            alpha1 += 1.0 / xi;
#pragma unroll
            for (int i = QMAX; i >= 2; --i) if (i <= j + 2) lv[i] = lv[i] * xiold + lv[i - 1];
            xiold = xi;
        }
        const double A1 = (-alpha0 - alpha1) / prod;
#pragma unroll
        FOR_S {
            const double zL = A1 * V.at(QMAX, s);
#pragma unroll
            for (int j = 2; j <= QMAX; ++j) if (j <= q) V.at(j, s) += lv[j] * zL;
            vset<CPL>(V, q + 1, s, zL);
        }
    } else {
        double hsum = 0.0;
        for (int j = 1; j <= q - 2; ++j) {
            hsum += ud(C->tau[j]);
            const double xi = hsum / hscale;
#pragma unroll
            for (int i = QMAX; i >= 2; --i) if (i <= j + 2) lv[i] = lv[i] * xi + lv[i - 1];
        }
#pragma unroll
        FOR_S {
            const double zq = vget<CPL>(V, q, s);
#pragma unroll
            for (int j = 2; j < QMAX; ++j) if (j < q) V.at(j, s) -= lv[j] * zq;
        }
    }
}
// trace row of an accepted step (save_data, src/BatchReactor.jl:383-402): t, h, q, the pressure
// of the last RHS evaluation, the accepted state u_n, the state y of the last RHS evaluation
template <int CPL, int GW = 64>
__device__ __forceinline__ void trace_row(LCtl* C, const CtlArgs& a, int lane, int step, double t,
                                          const double (&v)[CPL], const double (&y)[CPL]) {
    if (a.trace && step <= a.trace_cap) {
        auto row = a.trace + ((size_t)a.rid * (a.trace_cap + 1) + step) * (2 * a.n + 4);
        if (lane == 0) { row[0] = t; row[1] = ud(C->h); row[2] = (double)gui<GW>(C->q); row[3] = ud(C->p_last); }
#pragma unroll
        FOR_S if (CS < a.n) { row[4 + CS] = v[s]; row[4 + a.n + CS] = y[s]; }
    }
}
// one attempt of cvStep: predict, coefficients, and the Newton iteration's setup decision
template <int CPL, int GW = 64, int VS = GW>
__device__ __forceinline__ void begin_attempt(LCtl* C, VA<CPL, GW, VS>& V, int lane, int nflag) {
    const AttemptIn in = load_attempt<GW>(C);
    cv_predict<CPL, GW>(C, V, lane, in);
    double tq4, gamrat;
    cv_set_lp(C, in, tq4, gamrat);   // (cv_set: the plain form it is checked against)
    BR_XC_AFTER_CVSET();
    const int nst = in.nst;
    C->convfail = ((nflag == FIRST_CALL) || (nflag == PREV_ERR_FAIL)) ? NO_FAILURES : FAIL_OTHER;
    C->callSetup = (nflag == PREV_CONV_FAIL) || (nflag == PREV_ERR_FAIL) || (nst == 0) ||
                   (nst >= in.nstlp + MSBP) || (fabs(gamrat - 1.0) > DGMAX);
#pragma unroll
    FOR_S V.at(V_ACOR, s) = 0.0;
    C->tol = tq4;
    C->jbad = 0;
    C->jcur_nls = 0;
    C->m_it = 0;
#pragma unroll
    FOR_S V.at(V_Y, s) = V.at(0, s);   // y = z0
}
template <int CPL, int GW = 64, int VS = GW>
__device__ __forceinline__ void begin_step(LCtl* C, VA<CPL, GW, VS>& V, int lane, const CtlArgs& a) {
    BR_SUB_T(bt0);
    BR_QMARK(begin_step);
    const double tn = ud(C->tn), hprime = ud(C->hprime), h = ud(C->h);   // read before the V stores
    const int nst = gui<GW>(C->nst), qp = gui<GW>(C->qprime), q = gui<GW>(C->q);
#pragma unroll
    FOR_S {
        const double z0 = V.at(0, s);
        V.at(V_EWT, s) = (CS < a.n) ? 1.0 / (a.rtol * fabs(z0) + a.atol) : 1.0;
    }
    C->saved_t = tn;
    C->ncf = 0; C->nef = 0;
    if ((nst > 0) && (hprime != h)) {
        if (qp != q) {
            cv_adjust_order<CPL, GW>(C, V, lane, qp - q);
            C->q = qp; C->L = qp + 1; C->qwait = qp + 1;
        }
        cv_rescale<CPL, GW>(C, V, lane);
    }
    BR_QMARK(begin_step_attempt);
    begin_attempt<CPL, GW>(C, V, lane, FIRST_CALL);
    BR_QMARK(begin_step_end);
    BR_SUB_ADD(7, bt0);
}

// The time CVODE hands to f for the RHS evaluation the controller has just asked for (A_RHS), read
// from the controller's own state, where ctl_post_rhs / ctl_post_solve left it:
//   PH_F0      tn = t0: the first evaluation;
//   PH_HIN     tn + hg: cvYddNorm's f(tn + hg, y) of the initial-step estimate, hg as ctl_post_rhs set it
//              with the y of that evaluation (tn is still t0);
//   PH_NEWTON  tn: cv_predict advanced it (clamped to tstop) for the predictor and every Newton
//              evaluation of the attempt, cv_restore took it back to saved_t after a failed one; the DQ
//              columns and the analytic Jacobian of a setup are at the same tn;
//   PH_EF1     tn: the restored time (cvDoErrorTest's f(tn, zn[0]) before the order-1 restart).
// Only a temperature-programme run evaluates f at a time (k_integrate<NMAX, true>); a field for it in
// Ctl would move every engine's LDS block.
template <int GW = 64>
__device__ __forceinline__ double ctl_rhs_time(LCtl* C) {
    const double tn = ud(C->tn);
    return gui<GW>(C->phase) == PH_HIN ? tn + ud(C->hg) : tn;
}

// Controller, part 1: after the RHS value f = F(y) of this lane is known.
// Returns A_RHS (next y in V[V_Y]), A_SOLVE (delta for the solve returned in *rhs_out),
// A_SETUP (Jacobian decision in C->newj, then LU and solve), A_DONE.
template <int CPL, int GW = 64, int VS = GW, bool EN = false>
__device__ BR_CTL_INLINE int ctl_post_rhs(LCtl* C, VA<CPL, GW, VS>& V, int lane, const double (&f)[CPL], double (&rhs_out)[CPL]) {
    const CtlArgs a = load_args<GW>(C);
    const int n = a.n;
    C->nfe = gui<GW>(C->nfe) + 1;
    const int phase = gui<GW>(C->phase);
    double z0[CPL];
#pragma unroll
    FOR_S z0[s] = V.at(0, s);
    if (phase == PH_NEWTON) {
        const double rl1 = ud(C->rl1), gamma = ud(C->gamma);
#pragma unroll
        FOR_S {
            const double acor = V.at(V_ACOR, s);
            const double delta = (rl1 * V.at(1, s) + acor) - gamma * f[s];   // cvNlsResidual
            rhs_out[s] = -delta;
        }
        if (gui<GW>(C->m_it) == 0 && gui<GW>(C->callSetup)) {          // cvLsSetup decision
            const int nst = gui<GW>(C->nst);
            const double dgamma = fabs(ud(C->gamma) / ud(C->gammap) - 1.0);
            const int cf = gui<GW>(C->jbad) ? FAIL_BAD_J : gui<GW>(C->convfail);
            const int newj = (nst == 0) || (nst > gui<GW>(C->nstlj) + LS_MSBJ) || ((cf == FAIL_BAD_J) && (dgamma < LS_DGMAX)) ||
                             (cf == FAIL_OTHER);
            C->newj = newj;
            if (newj) { C->nje = gui<GW>(C->nje) + 1; C->nstlj = nst; }
            C->nsetups = gui<GW>(C->nsetups) + 1;
            C->jcur_nls = newj;
            C->gamrat = 1.0; C->gammap = ud(C->gamma); C->crate = 1.0; C->nstlp = nst;
            return A_SETUP;
        }
        return A_SOLVE;
    }
    double h = 0.0;
    if (phase == PH_EF1) {   // restart at order 1 after repeated error-test failures
        const double hh = ud(C->h);
#pragma unroll
        FOR_S V.at(1, s) = hh * f[s];
        begin_attempt<CPL, GW>(C, V, lane, PREV_ERR_FAIL);
        C->phase = PH_NEWTON;
        return A_RHS;
    }
    double z1in[CPL], ewt[CPL];
#pragma unroll
    FOR_S {
        z1in[s] = (phase == PH_F0) ? f[s] : V.at(1, s);
        ewt[s] = V.at(V_EWT, s);
    }
    if (phase == PH_F0) {
        const double tn = ud(C->tn), tstop = ud(C->tstop);
        const double tdist = fabs(tstop - tn);
        const double tround = UROUND * fmax(fabs(tn), fabs(tstop));
        const double hlb = HLB_FACTOR * tround;
        double ratio = 0.0;
#pragma unroll
        FOR_S {
            V.at(1, s) = f[s];
            if (CS < n) ratio = fmax(ratio, fabs(f[s]) / (HUB_FACTOR * fabs(z0[s]) + 1.0 / ewt[s]));
        }
        const double hub_inv = guni<GW>(gmax<GW>(ratio));
        double hub = HUB_FACTOR * tdist;
        if (hub * hub_inv > 1.0) hub = 1.0 / hub_inv;
        const double hg = sqrt(hlb * hub);
        C->hlb = hlb; C->hub = hub; C->hg = hg;
        if (hub < hlb) {
            h = hg;
        } else {
            C->count1 = 1; C->hnewOK = 0; C->hnew = hg;
#pragma unroll
            FOR_S V.at(V_Y, s) = hg * f[s] + z0[s];
            C->phase = PH_HIN;
            return A_RHS;
        }
    } else {                 // PH_HIN (cvYddNorm + the cvHin iteration)
        double hg = ud(C->hg);
        const double hub = ud(C->hub), hlb = ud(C->hlb);
        double tempv[CPL];
#pragma unroll
        FOR_S tempv[s] = (f[s] - z1in[s]) * (1.0 / hg);
        const double yddnrm = wrms_l<CPL, GW>(tempv, ewt, lane, n);
        const int count1 = gui<GW>(C->count1);
        double hnew;
        if (gui<GW>(C->hnewOK) || count1 == MAX_ITERS) {
            hnew = hg;
        } else {
            hnew = (yddnrm * hub * hub > 2.0) ? sqrt(2.0 / yddnrm) : sqrt(hg * hub);
            const double hrat = hnew / hg;
            int ok = 0;
            if ((hrat > 0.5) && (hrat < 2.0)) ok = 1;
            if ((count1 > 1) && (hrat > 2.0)) { hnew = hg; ok = 1; }
            C->hnewOK = ok;
            hg = hnew;
            C->hg = hg;
            C->count1 = count1 + 1;
#pragma unroll
            FOR_S V.at(V_Y, s) = hg * z1in[s] + z0[s];
            return A_RHS;
        }
        double h0 = H_BIAS * hnew;
        if (h0 < hlb) h0 = hlb;
        if (h0 > hub) h0 = hub;
        h = h0;
    }
    // ---- first step size known
    if (a.hmax_inv > 0) { const double rh = fabs(h) * a.hmax_inv; if (rh > 1.0) h /= rh; }
    const double tn = ud(C->tn), tstop = ud(C->tstop);
    if ((tn + h - tstop) * h > 0.0) h = (tstop - tn) * (1.0 - 4.0 * UROUND);
    C->h = h; C->hscale = h; C->hprime = h;
    if constexpr (!EN) trace_row<CPL, GW>(C, a, lane, 0, 0.0, z0, z0);   // (EN: a.trace is T_out, dense_output)
#pragma unroll
    FOR_S V.at(1, s) *= h;
    if (a.max_steps <= 0) { C->status = BR_ERR_MAXSTEPS; return A_DONE; }
    begin_step<CPL, GW>(C, V, lane, a);
    C->phase = PH_NEWTON;
    return A_RHS;
}

// x^(1/L) for the step-size ratios (L = order + 1 <= 6): hardware fp32 log2/exp2 estimate and
// two fp64 Newton steps (within a few ulp of pow(x, 1.0/L), which CVODE uses; ~40 instructions
// instead of ~280 for the generic pow); outside [1e-30, 1e30] the generic pow
__device__ __forceinline__ double root_int(double x, int L) {
    if (L == 1) return x;
    if (L == 2) return sqrt(x);
    if (!(x >= 1e-30 && x <= 1e30)) return pow(x, 1.0 / L);
    double y = (double)__builtin_amdgcn_exp2f(__builtin_amdgcn_logf((float)x) / (float)L);
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        double p = y;                                  // y^(L-1)
        for (int k = 2; k < L; ++k) p *= y;
        y -= (p * y - x) / (L * p);
    }
    return y;
}
// x^L for the small integer L of cvPrepareNextStep (repeated products; pow in CVODE)
__device__ __forceinline__ double pow_int(double x, int L) {
    double p = x;
    for (int k = 1; k < L; ++k) p *= x;
    return p;
}

// Controller, part 2: after the linear solve (delta = this lane's Newton correction) or after
// an LU failure (lu_fail != 0). Runs the convergence test, the error test, cvCompleteStep,
// cvPrepareNextStep and the tstop logic; returns A_RHS (next y in V[V_Y]) or A_DONE.
// (EN, the energy instances: component n - 1 is T. The NaN check covers it, the runaway test against ulimit
// does not; no trace rows; the dense output writes T_out)
template <int CPL, int GW = 64, int VS = GW, bool EN = false>
__device__ BR_CTL_INLINE int ctl_post_solve(LCtl* C, VA<CPL, GW, VS>& V, int lane, double (&delta)[CPL], int lu_fail) {
    BR_SUB_T(ps0);
    BR_QMARK(ps_start);
    const CtlArgs a = load_args<GW>(C);
    const int n = a.n;
    double ewt[CPL], acor[CPL];
#pragma unroll
    FOR_S ewt[s] = V.at(V_EWT, s);
    int nls;                                                   // 0 converged, else failure
    double acnrm = 0.0;
    const double tq2_e = ud(C->tq[2]);
    if (lu_fail) {
        nls = 2;
    } else {
        C->nni = gui<GW>(C->nni) + 1;
        const double gamrat = ud(C->gamrat);
        const int m = gui<GW>(C->m_it);                            // read before the V stores
        double crate = ud(C->crate);
        const double delp = ud(C->delp), tol = ud(C->tol);
#pragma unroll
        FOR_S {
            if (gamrat != 1.0) delta[s] *= 2.0 / (1.0 + gamrat);
            acor[s] = V.at(V_ACOR, s) + delta[s];
            V.at(V_ACOR, s) = acor[s];
        }
        const double del = wrms_l<CPL, GW>(delta, ewt, lane, n);     // cvNlsConvTest
        if (m > 0) { crate = fmax(CRDOWN * crate, del / delp); C->crate = crate; }
        const double dcon = del * fmin(1.0, crate) / tol;
        if (dcon <= 1.0) {
            acnrm = (m == 0) ? del : wrms_l<CPL, GW>(acor, ewt, lane, n);
            C->acnrm = acnrm;
            nls = 0;
        } else {
            bool fail = (m >= 1) && (del > RDIV * delp);
            if (!fail) {
                C->delp = del;
                C->m_it = m + 1;
                if (m + 1 >= NLS_MAXCOR) fail = true;
            }
            if (!fail) {
#pragma unroll
                FOR_S V.at(V_Y, s) = V.at(0, s) + acor[s];
                return A_RHS;
            }
            if (!gui<GW>(C->jcur_nls)) {                          // retry with a fresh Jacobian
                C->callSetup = 1; C->jbad = 1; C->m_it = 0;
#pragma unroll
                FOR_S {
                    V.at(V_ACOR, s) = 0.0;
                    V.at(V_Y, s) = V.at(0, s);
                }
                return A_RHS;
            }
            nls = 1;
        }
    }
    BR_QMARK(ps_nflag);
    if (nls != 0) {                                          // cvHandleNFlag
        C->ncfn = gui<GW>(C->ncfn) + 1;
        cv_restore<CPL, GW>(C, V, lane);
        const int ncf = gui<GW>(C->ncf) + 1;
        C->ncf = ncf;
        C->etamax = 1.0;
        if (ncf == MXNCF) { C->status = BR_ERR_CONV; return A_DONE; }
        C->eta = ETACF;
        cv_rescale<CPL, GW>(C, V, lane);
        begin_attempt<CPL, GW>(C, V, lane, PREV_CONV_FAIL);
        return A_RHS;
    }
    // ---- cvDoErrorTest
    BR_QMARK(ps_errtest);
    const double dsm = acnrm * tq2_e;
    const int q = gui<GW>(C->q);
    if (dsm > 1.0) {
        const int nef = gui<GW>(C->nef) + 1;
        C->nef = nef; C->netf = gui<GW>(C->netf) + 1;
        cv_restore<CPL, GW>(C, V, lane);
        if (nef == MXNEF) { C->status = BR_ERR_ERRTEST; return A_DONE; }
        C->etamax = 1.0;
        if (nef <= MXNEF1) {
            double eta = 1.0 / (root_int(BIAS2 * dsm, gui<GW>(C->L)) + ADDON);
            eta = fmax(ETAMIN, eta);
            if (nef >= SMALL_NEF) eta = fmin(eta, ETAMXF);
            C->eta = eta;
            cv_rescale<CPL, GW>(C, V, lane);
            begin_attempt<CPL, GW>(C, V, lane, PREV_ERR_FAIL);
            return A_RHS;
        }
        if (q > 1) {
            C->eta = ETAMIN;
            cv_adjust_order<CPL, GW>(C, V, lane, -1);
            C->L = q; C->q = q - 1; C->qwait = q;
            cv_rescale<CPL, GW>(C, V, lane);
            begin_attempt<CPL, GW>(C, V, lane, PREV_ERR_FAIL);
            return A_RHS;
        }
        C->eta = ETAMIN;
        const double h = ud(C->h) * ETAMIN;
        C->h = h; C->hscale = h; C->qwait = LONG_WAIT;
#pragma unroll
        FOR_S V.at(V_Y, s) = V.at(0, s);
        C->phase = PH_EF1;
        return A_RHS;
    }
    // ---- cvCompleteStep
    BR_SUB_ADD(8, ps0);
    BR_QMARK(ps_complete);
    BR_SUB_T(ps1);
    // every controller scalar this part reads, loaded in one batch before the first Nordsieck store
    // (V shares LDS with the controller, so a load placed after a V store cannot be hoisted above
    // it: read in place, each one was its own LDS round trip)
    const int nst = gui<GW>(C->nst) + 1;
    const double h = ud(C->h);
    double tauv[QMAX + 1], lv[QMAX + 1];
#pragma unroll
    for (int i = 1; i <= QMAX; ++i) tauv[i] = ud(C->tau[i]);
#pragma unroll
    for (int j = 0; j <= QMAX; ++j) lv[j] = ud(C->l[j]);
    int qwait = gui<GW>(C->qwait) - 1;
    const double etamax = ud(C->etamax), tq1 = ud(C->tq[1]), tq2 = ud(C->tq[2]), tq3 = ud(C->tq[3]);
    const double tq5 = ud(C->tq[5]);
    double saved_tq5 = ud(C->saved_tq5);
    const int L = gui<GW>(C->L);
    const int nstloc = gui<GW>(C->nstloc) + 1;
    const double tn = ud(C->tn), tstop = ud(C->tstop), ulimit = ud(C->ulimit);
    C->nst = nst;
    double tau2 = tauv[2];   // tau[2] after the shift
#pragma unroll
    for (int i = QMAX; i >= 2; --i) if (i <= q) C->tau[i] = tauv[i - 1];
    if (q >= 2 || nst > 1) tau2 = tauv[1];
    if ((q == 1) && (nst > 1)) C->tau[2] = tauv[1];
    C->tau[1] = h;
#pragma unroll
    FOR_S acor[s] = V.at(V_ACOR, s);
#pragma unroll
    for (int j = 0; j <= QMAX; ++j) {
        if (j <= q) {
#pragma unroll
            FOR_S V.at(j, s) += lv[j] * acor[s];
        }
    }
    if ((qwait == 1) && (q != QMAX)) {
#pragma unroll
        FOR_S V.at(QMAX, s) = acor[s];
        saved_tq5 = tq5;
        C->saved_tq5 = tq5;
    }
    // ---- cvPrepareNextStep
    BR_QMARK(ps_prepare);
    double eta = 1.0, hprime = h;
    int qprime = q;
    if (etamax == 1.0) {
        qwait = qwait > 2 ? qwait : 2;
    } else {
        // the three step-size ratios (etaq, and at an order decision etaqm1 / etaqp1) in ONE root and
        // division sequence: lane 0 of each DPP row takes etaq's argument, lane 1 etaqm1's, lane 2
        // etaqp1's (root_int and the division per lane; a row broadcast returns each); C2: etaq's
        // root + division alone was 4.6 % of the kernel's VALU (profiles/r06_quad_valu_split.json)
        const int t = lane & 15;
        double xm = 1.0, xp = 1.0;     // benign arguments for lanes whose ratio is not needed
        bool hm = false, hp = false;
        if (qwait == 0) {
            if (q > 1) {
                double zq[CPL];
#pragma unroll
                FOR_S zq[s] = vget<CPL>(V, q, s);
                const double ddn = wrms_l<CPL, GW>(zq, ewt, lane, n) * tq1;
                xm = BIAS1 * ddn;
                hm = true;
            }
            if (q != QMAX && saved_tq5 != 0.0) {
                const double cquot = (tq5 / saved_tq5) * pow_int(h / tau2, L);
                double tempv[CPL];
#pragma unroll
                FOR_S tempv[s] = acor[s] - cquot * V.at(QMAX, s);
                const double dup = wrms_l<CPL, GW>(tempv, ewt, lane, n) * tq3;
                xp = BIAS3 * dup;
                hp = true;
            }
        }
        const double xa = t == 1 ? xm : (t == 2 ? xp : BIAS2 * dsm);
        const int La = t == 1 ? (hm ? q : L) : (t == 2 ? (hp ? L + 1 : L) : L);
        const double er = 1.0 / (root_int(xa, La) + ADDON);
        const double etaq = row_lane<0>(er);
        BR_XC_AFTER_ETAQ();
        if (qwait != 0) { eta = etaq; }
        else {
            qwait = 2;
            const double etaqm1 = hm ? row_lane<1>(er) : 0.0;
            const double etaqp1 = hp ? row_lane<2>(er) : 0.0;
            const double etam = fmax(etaqm1, fmax(etaq, etaqp1));
            if (etam < THRESH) { eta = 1.0; }
            else if (etam == etaq) { eta = etaq; }
            else if (etam == etaqm1) { eta = etaqm1; qprime = q - 1; }
            else {
                eta = etaqp1; qprime = q + 1;
#pragma unroll
                FOR_S V.at(QMAX, s) = acor[s];
            }
        }
        if (eta < THRESH) { eta = 1.0; hprime = h; }                // cvSetEta
        else {
            eta = fmin(eta, etamax);
            if (a.hmax_inv > 0) eta /= fmax(1.0, fabs(h) * a.hmax_inv * eta);   // (/ 1.0 otherwise)
            hprime = h * eta;
        }
    }
    C->qwait = qwait;
    C->etamax = (nst <= SMALL_NST) ? ETAMX2 : ETAMX3;
#pragma unroll
    FOR_S V.at(V_ACOR, s) = acor[s] * tq2;
    C->nstloc = nstloc;
    double z0[CPL];
#pragma unroll
    FOR_S z0[s] = V.at(0, s);
    C->eta = eta; C->hprime = hprime; C->qprime = qprime;
    BR_SUB_ADD(9, ps1);
    BR_QMARK(ps_unstable);
    BR_SUB_T(ps2);
    {   // SciML unstable_check: NaN state (ulimit = inf), or opt-in runaway (br_opts.unstable_factor);
        // first, as in the oracle: an unstable step writes no trace row and no dense output
        double zm = 0.0;
#pragma unroll
        FOR_S if (CS < n) {
            const double a = fabs(z0[s]);
            if constexpr (EN) zm = fmax(zm, a == a ? (CS == n - 1 && a < INFINITY ? 0.0 : a) : INFINITY);
            else zm = fmax(zm, a == a ? a : INFINITY);
        }
        const double mx = guni<GW>(gmax<GW>(zm));
        if (!(mx < INFINITY) || mx > ulimit) { C->status = BR_ERR_UNSTABLE; return A_DONE; }
    }
    if (!EN && a.trace) {
        double yl[CPL];
#pragma unroll
        FOR_S yl[s] = V.at(V_Y, s);                     // the last RHS was evaluated at y
        trace_row<CPL, GW>(C, a, lane, nst, tn, z0, yl);
    }
    BR_QMARK(ps_ignition);
    if (a.ign >= 0) track_ignition<CPL, GW>(C, a, lane, tn, z0);
    BR_QMARK(ps_dense);
    if (a.nout) dense_output<CPL, GW, VS, EN>(C, V, a, lane, tn, h, q, tn);
    // CVode ONE_STEP + tstop handling
    BR_QMARK(ps_tstop);
    const double troundoff = FUZZ * UROUND * (fabs(tn) + fabs(h));
    if (fabs(tn - tstop) <= troundoff) {                     // CVodeGetDky(tstop, 0)
        if (a.nout) dense_output<CPL, GW, VS, EN>(C, V, a, lane, tn, h, q, tstop);
        const double sk = (tstop - tn) / h;
#pragma unroll
        FOR_S {
            double yv = vget<CPL>(V, q, s);
#pragma unroll
            for (int j = QMAX - 1; j >= 0; --j) if (j < q) yv = V.at(j, s) + sk * yv;
            V.at(V_Y, s) = yv;
            if (!EN && a.trace && nst <= a.trace_cap) {
                auto row = a.trace + ((size_t)a.rid * (a.trace_cap + 1) + nst) * (2 * n + 4);
                if (lane == 0 && s == 0) row[0] = tstop;
                if (CS < n) row[4 + CS] = yv;
            }
        }
        return A_DONE;
    }
    if ((tn + hprime - tstop) * h > 0.0) {
        hprime = (tstop - tn) * (1.0 - 4.0 * UROUND);
        C->hprime = hprime;
        C->eta = hprime / h;
    }
    if (nstloc >= a.max_steps) { C->status = BR_ERR_MAXSTEPS; return A_DONE; }
    BR_SUB_ADD(10, ps2);
    BR_QMARK(ps_to_begin);
    begin_step<CPL, GW>(C, V, lane, a);
    BR_QMARK(ps_end);
    return A_RHS;
}

// ---- CVODE's dense difference-quotient Jacobian (cvLsDenseDQJac; CVODE_BDF()'s default, no `jac`
// is passed to ODEProblem at src/BatchReactor.jl:140,:204): at the setup point (y = z0, fy = F(y)),
// column j = (F(y + inc_j e_j) - fy) / inc_j with inc_j = max(sqrt(uround) |y_j|, minInc / ewt_j),
// minInc = 1000 |h| uround n ||fy||_WRMS (1 if that norm is 0). One RHS per column, run through the
// kernel's single RHS call site (k_integrate: the column index `dqj` routes the result here).
constexpr double DQ_SRUR = 1.4901161193847656e-08;   // sqrt(UROUND) = 2^-26
constexpr double DQ_MIN_INC_MULT = 1000.0;
template <int CPL, int GW = 64, int VS = GW>
__device__ __forceinline__ void dq_begin(LCtl* C, VA<CPL, GW, VS>& V, int lane, const double (&f)[CPL]) {
    const int n = gui<GW>(C->a_n);
    double ewt[CPL];
#pragma unroll
    FOR_S {
        ewt[s] = V.at(V_EWT, s);
        V.at(V_TEMP, s) = f[s];                      // fy, kept for the n columns
    }
    const double fnorm = wrms_l<CPL, GW>(f, ewt, lane, n);
    C->dq_mininc = (fnorm != 0.0) ? (DQ_MIN_INC_MULT * fabs(ud(C->h)) * UROUND * n * fnorm) : 1.0;
}
// increment of this lane's components (the one for component j is used by column j)
template <int CPL, int GW = 64, int VS = GW>
__device__ __forceinline__ void dq_incs(LCtl* C, VA<CPL, GW, VS>& V, int lane, double (&inc)[CPL]) {
    const double mininc = ud(C->dq_mininc);
#pragma unroll
    FOR_S inc[s] = fmax(DQ_SRUR * fabs(V.at(V_Z0, s)), mininc / V.at(V_EWT, s));
}
// column j of the saved J from F(y + inc_j e_j) = f (rows as jacobian(): JW per column)
template <int CPL, int GW = 64, int VS = GW>
__device__ __forceinline__ void dq_column(LCtl* C, VA<CPL, GW, VS>& V, int lane, int j, const double (&f)[CPL], double* Jsave) {
    constexpr int JW = CPL == 2 ? 80 : 64;
    double inc[CPL];
    dq_incs<CPL, GW>(C, V, lane, inc);
    const double ij = (j < 64) ? gbcast<GW>(inc[0], j) : gbcast<GW>(inc[CPL - 1], j - 64);
    const double ii = 1.0 / ij;
    BR_GLOBAL double* col = launder(Jsave) + (size_t)j * JW;
    const int n = gui<GW>(C->a_n);
    // rows >= n stored as 0 (with 32-wide vectors lanes 32..63 read lane - 32's V_TEMP, and f is 0
    // there: no consumer of Jsave has to mask them)
#pragma unroll
    FOR_S {
        const double v = CS < n ? ii * f[s] - ii * V.at(V_TEMP, s) : 0.0;
        if (s == 0) col[lane] = v;
        else if (lane < 16) col[64 + lane] = v;
    }
    C->nfe_dq = gui<GW>(C->nfe_dq) + 1;
}
// the Newton right-hand side at the setup point again (cvNlsResidual with f = fy, as ctl_post_rhs)
template <int CPL, int GW = 64, int VS = GW>
__device__ __forceinline__ void dq_newton_rhs(LCtl* C, VA<CPL, GW, VS>& V, int lane, double (&b)[CPL]) {
    const double rl1 = ud(C->rl1), gamma = ud(C->gamma);
#pragma unroll
    FOR_S b[s] = -((rl1 * V.at(1, s) + V.at(V_ACOR, s)) - gamma * V.at(V_TEMP, s));
}

}  // namespace
