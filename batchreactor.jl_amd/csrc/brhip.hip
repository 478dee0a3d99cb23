// brhip.hip -- libbrhip.so: C-ABI (include/brhip.h) + the batched CVODE-style BDF kernel.
//
// The integrator restates SUNDIALS CVODE 5.x (the solver behind CVODE_BDF() in
// src/BatchReactor.jl:138-141,:210): Nordsieck BDF orders 1..5, modified Newton with
// maxcor 3, Jacobian reuse (msbp 20 / msbj 51 / dgmax 0.3/0.2), WRMS error test, cvHin
// initial step, tstop clamping and dense output at tstop. The Jacobian is analytic
// (brhip_device.hpp) instead of CVODE's difference quotients.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/brhip.h"
#include "brhip_ctl.hpp"   // CVODE constants, KOpts, the controller on the LDS block
#include "mech_pack.hpp"   // br_mech_desc -> DevMech + tables (host)

namespace {

#include "brhip_lane.hpp"   // one reactor per lane (small gas mechanisms)
#include "brhip_energy.hpp"  // adiabatic constant-volume reactors: T as component ng of the energy instances
#include "brhip_group.hpp"   // group engines: 4 / 2 reactors per wave (16- / 32-lane groups, n <= 32)
#include "brhip_sens.hpp"    // rate-multiplier block, br_sensitivity's expansion and reduction kernels
#include "brhip_tprog.hpp"   // temperature programmes T(t): the launch's block and the evaluator

// ------------------------------------------------------------------------------------
// the integrator kernel: one reactor per 64-lane wavefront, `rpb` reactors per workgroup
// ------------------------------------------------------------------------------------
#ifndef BR_WPE
#define BR_WPE 2
#endif
// (Measured and not adopted, round 4-5; DESIGN.md section 3: the blocked LU with fp64 MFMA trailing
// updates -- GRI 88.8k / 92.0k vs 110.5k reactors/s, now in the variant library
// csrc/variants/brhip_lumf.hip -- and the 4 x 16 lane-grid LU with DPP-broadcast FMAs -- GRI -3.1 %,
// removed in round 6; it stays in the git history before that round.)
// upper bound of reactors (waves) per workgroup for the occupancy search: gas+surface (n > 64)
// needs 21 KB of LDS per reactor (+18 KB of tables), so only one workgroup of up to 6 reactors
// (tables staged once) fits a CU's 160 KB: 6 waves/CU instead of 4 with 1-reactor workgroups;
// n <= 64 keeps 256-thread workgroups (2 x 4 or 4 x 2 reactors, 8 waves/CU, VGPR-limited)
#ifndef BR_MAXRPB56
#define BR_MAXRPB56 16   // n in 33..64: one workgroup of up to 16 reactors per CU (tables staged once)
#endif
#ifndef BR_MAXRPB72
#define BR_MAXRPB72 12   // n > 64 (gas + surface): one workgroup of up to 12 reactors per CU (tables staged once)
#endif
__host__ __device__ constexpr int br_maxrpb(int nmax) {
    return nmax > 64 ? BR_MAXRPB72 : (nmax == 56 || nmax == 64) ? BR_MAXRPB56 : 4;
}
constexpr size_t LDS_PER_CU = 160 * 1024, LDS_GRANULE = 1280;   // gfx950 (granule: conservative)
#ifndef BR_WPE32
#define BR_WPE32 5   // n <= 32 (surface-only): 5 waves/SIMD (96 VGPRs, 80 B/lane spilled) -- with the 32-wide
                     // vectors (BR_VS32) five 4-reactor workgroups fit the LDS: 20 waves/CU, C4 232.8k vs
                     // 219.7k reactors/s at 16 (round 5); round 2: 3 waves/SIMD, 12 waves/CU, 130k -> 156k/s
#endif
// minimum waves per SIMD the register allocator must allow, per instance
#ifndef BR_WPE72
#define BR_WPE72 3   // n > 64: 3 waves/SIMD (168 VGPRs, 26 spilled; 11 reactors per CU by LDS: +3 % over 2 waves)
#endif
#ifndef BR_WPE56
#define BR_WPE56 4   // n in 33..64 (GRI): 4 waves/SIMD (<= 128 VGPRs; 16 x 8.8 KB + tables fit the LDS)
#endif
__host__ __device__ constexpr int br_wpe(int nmax) {
    return nmax == 32 ? BR_WPE32 : (nmax == 56 || nmax == 64) ? BR_WPE56 : nmax == 72 ? BR_WPE72 : BR_WPE;
}
// TPROG: the instances of a temperature-programme run (br_opts.ntprog; brhip_tprog.hpp). They take KOptsProg,
// do not read Tv, and refresh the T-only constants inside the step loop; everything under
// `if constexpr (TPROG)` is theirs alone, the isothermal instances compile the source they always had.
// ENERGY: the instances of an adiabatic run (br_opts.energy; brhip_energy.hpp), NMAX from ng + 1. They take
// KOptsEnergy, carry T as component ng (lane ng) of a system of nsys = ng + 1 equations, refresh the constants
// before any RHS whose T differs from the cached one, and always build CVODE's DQ Jacobian; everything under
// `if constexpr (ENERGY)` is theirs alone.
// The instances that keep a lane's first two {kf, kr} pairs and its molar mass in registers between setups
// (KReg): n in 33..56, isothermal or with a programme (a programme's refresh reloads them). Not the energy
// instance, which refreshes the constants twice per DQ Jacobian, and not NMAX = 64: with two pairs held (the form
// with the first pass unrolled) their scratch grew, 120 -> 160 B and 68 -> 84 B. NMAX = 16 / 32 / 72 spill already.
__host__ __device__ constexpr bool kreg_on(int nmax, bool energy) { return nmax == 56 && !energy; }
template <int NMAX, bool TPROG = false, bool ENERGY = false>
__global__ __launch_bounds__(64 * br_maxrpb(NMAX)) __attribute__((amdgpu_waves_per_eu(br_wpe(NMAX), 8))) void k_integrate(
    DevMech M, int N, int rpb, const double* __restrict__ Tv, const double* __restrict__ Asvv, double* __restrict__ U,
    const double* __restrict__ tfv, std::conditional_t<TPROG, KOptsProg, std::conditional_t<ENERGY, KOptsEnergy, KOpts>> o,
    br_stats* __restrict__ stats, double* __restrict__ Jws, double* __restrict__ trace) {
    static_assert(!(TPROG && ENERGY) && (!ENERGY || NMAX <= 56), "energy instances: no programme, one component per lane");
    constexpr int CPL = NMAX > 64 ? 2 : 1;   // components per lane
    constexpr bool KR = kreg_on(NMAX, ENERGY);
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const WaveCtx W = [&] {
        if constexpr (ENERGY) return energy_wave_ctx<NMAX>(M, smem_raw, rpb, Jws);
        else return wave_ctx<CPL, NMAX>(M, smem_raw, rpb, Jws);
    }();
    // Reactor indices: with o.work every wave of the (resident-sized) grid keeps taking the next
    // index from the counter until the list is drained, so a wave whose reactor finishes early
    // starts another instead of idling until the slowest reactor of its workgroup is done; the
    // wave's workspace slot and LDS block are reused. Index -> reactor through rid_list when set
    // (the deferred reactors of a k_lane pass).
    const int widx = W.rid;               // workspace slot of this wave
    const int nidx = o.rid_list ? min(*o.rid_count, N) : N;
    auto next_index = [&]() -> int {
        int v = 0;
        if (W.lane == 0) v = atomicAdd(o.work, 1);
        return __builtin_amdgcn_readlane(v, 0);
    };
    for (int idx = o.work ? next_index() : widx; idx < nidx; idx = o.work ? next_index() : nidx) {
    int rid = o.rid_list ? uni(o.rid_list[idx]) : idx;
    wave_sync();
    const int lane = W.lane;
    const Tab& tb = W.tb;
    const size_t roff = (size_t)(W.rbase - smem_raw);
    LCtl* C = (LCtl*)(smem_raw + roff);
    const VA<CPL, 64, vec_stride(NMAX)> Vm{(LDbl*)(smem_raw + roff + CTL_BYTES), lane};
    VA<CPL, 64, vec_stride(NMAX)> V = Vm;
    const RView& S = W.R;
    const int n = M.n;
    const int nsys = ENERGY ? n + 1 : n;   // equations of the controller, the DQ Jacobian, the LU and the solve
    // T: the temperature the T-only constants in the reactor's slots were built for. Isothermal: the
    // reactor's constant. Programme run: T(t) of the last refresh, wave-uniform, with the reactor's row
    // and cached segment in tp. Energy run: the clamped T of the last refresh, wave-uniform, with the
    // lane's e_k and cv_k at it in ek, cvk
    double T;
    [[maybe_unused]] std::conditional_t<TPROG, TProgRow, NoTProgRow> tp;
    [[maybe_unused]] double ek = 0.0, cvk = 0.0;
    if constexpr (TPROG) {
        tp = tprog_row(o.prog, rid);
        T = uni(tp.eval(o.rid_t0 ? uni(o.rid_t0[idx]) : 0.0));
    } else if constexpr (ENERGY) {
        T = energy_tclamp(uni(Tv[rid]));
    } else {
        T = Tv[rid];
    }
    const double Asv = Asvv ? Asvv[rid] : 1.0;
    const double Asv_th = (M.conv & 4) ? 1.0 : Asv;
    double* Jsave = Jws + (size_t)widx * ws_doubles(NMAX, M.nrg);   // J, LU factors, Jacobian scratch
    double* LUsave = Jsave + NMAX * col_rows(NMAX);
    double* jscr = LUsave;   // (aliases the factors: see rxd_ws_off)
    C->a_rtol = o.rtol; C->a_atol = o.atol; C->a_hmax_inv = o.hmax_inv; C->a_ufac = o.ufac;
    C->a_max_steps = o.max_steps; C->a_trace_cap = o.trace_cap; C->a_rid = rid; C->a_n = nsys;
    if constexpr (ENERGY) C->a_trace = o.T_out;   // (no trace in an energy run: the slot carries T_out)
    else C->a_trace = trace;
    C->a_ign = o.ign; C->a_nout = o.nout; C->a_tout = o.tout; C->a_yout = o.yout;

    init_tconst<CPL, true>(M, tb, S, T, lane, rid);
    KReg<KR> kq;   // the lane's first two {kf, kr} pairs and its molar mass (brhip_device.hpp, KReg: lifetime)
    kreg_load(kq, tb, S, lane);
    if constexpr (ENERGY) energy_thermo(lane, n, T, ek, cvk);

    // ---- CVodeInit
    double u0[CPL], su = 0.0;
#pragma unroll
    FOR_S {
        const bool act = CS < nsys;
        if constexpr (ENERGY) u0[s] = CS < n ? U[(size_t)rid * n + CS] : (CS == n ? uni(Tv[rid]) : 0.0);   // lane ng: T(0)
        else u0[s] = act ? U[(size_t)rid * n + CS] : 0.0;
#pragma unroll
        for (int j = 0; j < NVEC; ++j) V.at(j, s) = 0.0;
        V.at(0, s) = u0[s];
        V.at(V_Y, s) = u0[s];
        V.at(V_EWT, s) = act ? 1.0 / (o.rtol * fabs(u0[s]) + o.atol) : 1.0;
        su += (ENERGY ? CS < n : act) ? fabs(u0[s]) : 0.0;   // (the runaway limit is on the species)
    }
#pragma unroll
    for (int i = 0; i < QMAX + 2; ++i) C->tau[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) C->tq[i] = 0.0;
#pragma unroll
    for (int i = 0; i <= QMAX; ++i) C->l[i] = 0.0;
    C->tn = 0.0; C->h = 0.0; C->rl1 = 0.0; C->gamma = 0.0; C->gamrat = 1.0; C->gammap = 0.0; C->crate = 1.0;
    C->delp = 0.0; C->hprime = 0.0; C->hscale = 0.0; C->eta = 1.0; C->etamax = ETAMX1; C->acnrm = 0.0;
    C->saved_tq5 = 0.0; C->saved_t = 0.0; C->tol = 0.0; C->hg = 0.0; C->hub = 0.0; C->hlb = 0.0; C->hnew = 0.0;
    C->tstop = tfv[rid];
    const double t0 = o.rid_t0 ? uni(o.rid_t0[idx]) : 0.0;   // > 0: continue a deferred lane reactor
    C->tn = t0;
    C->ulimit = o.ufac > 0.0 ? o.ufac * uni(wave_sum(su)) : INFINITY;
    C->q = 1; C->qprime = 1; C->L = 2; C->qwait = 2;
    C->nst = 0; C->nfe = 0; C->nsetups = 0; C->nje = 0; C->nni = 0; C->ncfn = 0; C->netf = 0; C->nstlp = 0;
    C->nstlj = 0; C->ncf = 0; C->nef = 0; C->nstloc = 0; C->status = 0; C->m_it = 0; C->convfail = 0;
    C->count1 = 0; C->phase = PH_F0; C->callSetup = 0; C->jbad = 0; C->jcur_nls = 0; C->hnewOK = 0; C->newj = 0;
    C->p_last = 0.0;
    C->iout = 0; C->ign_t = t0; C->ign_rate = -INFINITY; C->t_ign = NAN; C->ign_x = 0.0; C->ign_dt = NAN;
    C->dq_mininc = 1.0; C->nfe_dq = 0;
    if (o.ign >= 0) C->ign_x = uni(mole_frac_of<CPL>(u0, lane, o.ign));
    // counters and ignition marker of the lane pass (deferred reactors) to continue from
    enum { P_NSTEPS, P_NFE, P_NJE, P_NSETUPS, P_NNI, P_NCFN, P_NETF, P_NFE_DQ, P_COUNT };
    double prev[P_COUNT] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (o.rid_t0 && stats) {
        // (read as columns of the [N][BR_NSTAT] array, index rid * BR_NSTAT + column, the seven leading
        // counters in one loop: as member reads the same loads left k_integrate<32> and <72> with another
        // register allocation)
        static_assert(BR_STAT_COL(nsteps) == P_NSTEPS && BR_STAT_COL(netf) == P_NETF, "the carried counters lead br_stats");
        const double* last = reinterpret_cast<const double*>(stats);
#pragma unroll
        for (size_t k = BR_STAT_COL(nsteps); k <= BR_STAT_COL(netf); ++k) prev[k] = uni(last[(size_t)rid * BR_NSTAT + k]);
        prev[P_NFE_DQ] = uni(last[(size_t)rid * BR_NSTAT + BR_STAT_COL(nfe_dq)]);
        // the step limit is on the whole run (SciML maxiters): the lane pass's steps count against it
        C->a_max_steps = max(o.max_steps - (int)prev[P_NSTEPS], 0);
        if (o.ign >= 0) {
            C->ign_rate = uni(last[(size_t)rid * BR_NSTAT + BR_STAT_COL(ign_rate)]);
            C->t_ign = uni(last[(size_t)rid * BR_NSTAT + BR_STAT_COL(t_ign)]);
            C->ign_dt = uni(last[(size_t)rid * BR_NSTAT + BR_STAT_COL(ign_dt)]);
        }
    }
    if (o.nout) {                                           // outputs at t <= t0: the initial state
        int io = 0;
        while (io < o.nout && tout_pre(o.tout, (size_t)rid * o.nout + io, io, t0)) {
            if (!o.rid_t0)                                  // (a continued reactor wrote them already)
#pragma unroll
                FOR_S if (CS < n) o.yout[((size_t)rid * o.nout + io) * n + CS] = u0[s];
            if constexpr (ENERGY) { if (o.T_out && lane == n) o.T_out[(size_t)rid * o.nout + io] = u0[0]; }
            ++io;
        }
        C->iout = io;
    }

    BR_CLK_BEGIN;
    const unsigned long long cyc0 = wall_clock64();
    int perm[CPL];
#pragma unroll
    FOR_S perm[s] = CS;
    LDSd* scr = (LDSd*)(S.sp + Lay<CPL>::ACCW);   // solve / LU scratch: the production sums are idle then
    double* p_last = reinterpret_cast<double*>(W.rbase);
    int dqj = -1;   // >= 0: building DQ Jacobian column dqj (this RHS is at y + inc_dqj e_dqj)
    // Programme run, before an RHS or Jacobian evaluation: T at the time the controller means
    // (ctl_rhs_time). Bitwise the cached T: the constants stand (the DQ columns and Newton iterations of
    // an attempt share its tn, a constant programme never changes). Else the isothermal prologue's
    // init_tconst for the new T, fences included: {kf, kr} live in the global slot. Its g/RT scratch is
    // the production sums' block, idle between evaluations (the RHS zeroes it, the solve is done with it).
    auto tprog_refresh = [&]() {
        if constexpr (TPROG) {
            const double Tt = uni(tp.eval(uni(ctl_rhs_time(C))));
            if (__double_as_longlong(Tt) != __double_as_longlong(T)) {
                T = Tt;
                wave_sync();
                init_tconst<CPL, true>(M, tb, S, T, lane, rid);
                kreg_load(kq, tb, S, lane);
            }
        }
    };
    // Energy run, before an RHS: T is component ng of the y it is evaluated at, clamped. Bitwise the cached T
    // (the species columns of a DQ Jacobian, a Newton iterate that left T alone): the constants stand. Else
    // tprog_refresh's sequence, and lane k recomputes its e_k and cv_k. The T column of a DQ Jacobian
    // refreshes once, the RHS after it refreshes back.
    auto energy_refresh = [&](double yl) {
        if constexpr (ENERGY) {
            const double Tc = energy_tclamp(uni(bcast(yl, n)));
            if (__double_as_longlong(Tc) != __double_as_longlong(T)) {
                T = Tc;
                wave_sync();
                init_tconst<CPL, true>(M, tb, S, T, lane, rid);
                energy_thermo(lane, n, T, ek, cvk);
            }
        }
    };
    for (;;) {
        double y[CPL], f[CPL];
#pragma unroll
        FOR_S y[s] = V.at(V_Y, s);
        if (dqj >= 0) {
            double inc[CPL];
            dq_incs<CPL>(C, V, lane, inc);
#pragma unroll
            FOR_S if (CS == dqj) y[s] += inc[s];
        }
        {
            BR_CLK(c0);
            tprog_refresh();
            energy_refresh(y[0]);
            rhs<CPL, KR>(M, tb, S, T, Asv, Asv_th, y, lane, p_last, f, kq);
            if constexpr (ENERGY) {   // f[ng] = dT/dt from the du just computed (lane ng's f was 0)
                const double Td = energy_tdot(tb, lane, n, y[0], f[0], ek, cvk);
                if (lane == n) f[0] = Td;
            }
            BR_X_AFTER_RHS();
            BR_ACC(cyc_rhs, c0);
        }
        double b[CPL];
        int act_code;
        bool jac_ready = false;
        if (dqj >= 0) {   // a DQ column (its RHS counts in nfe_dq, not nfe)
            BR_CLK(c0);
            dq_column<CPL>(C, V, lane, dqj, f, Jsave);
            BR_ACC(cyc_jac, c0);
            if (++dqj < nsys) continue;
            dqj = -1;
            dq_newton_rhs<CPL>(C, V, lane, b);
            act_code = A_SETUP;
            jac_ready = true;
        } else {
            BR_CLK(c2);
            BR_SUB_T(pr0);
            if constexpr (ENERGY) act_code = ctl_post_rhs<CPL, 64, vec_stride(NMAX), true>(C, V, lane, f, b);
            else act_code = ctl_post_rhs<CPL>(C, V, lane, f, b);
            BR_SUB_ADD(3, pr0);
            BR_ACC(cyc_ctl, c2);
            if (act_code == A_RHS) continue;
            if (act_code == A_DONE) break;
            if (act_code == A_SETUP && o.dq_jac && ui(C->newj)) {
                dq_begin<CPL>(C, V, lane, f);
                dqj = 0;
                continue;
            }
        }
        int lu_fail = 0;
        if (act_code == A_SETUP) {
            if constexpr (!ENERGY) {   // (an energy run's o.dq_jac is always set: every new J came from the DQ columns)
            if (!jac_ready && ui(C->newj)) {
                BR_CLK(c0);
                tprog_refresh();   // (the tn of the RHS just before: no refresh in practice)
                jacobian<CPL>(M, tb, S, T, Asv, Asv_th, y, lane, Jsave, jscr);
                BR_X_AFTER_JAC();
                BR_ACC(cyc_jac, c0);
            }
            }
            BR_CLK(c1);
            if constexpr (CPL == 1) lu_fail = lu_factor<NMAX>(Jsave, LUsave, ud(C->gamma), nsys, lane, perm[0]);
            else lu_fail = lu_factor2<NMAX>(Jsave, LUsave, scr, ud(C->gamma), nsys, lane, perm);
            // the registers were dead across the setup: the pairs again from the slot (lu_solve's entry
            // drains the memory counter, so their latency runs under it)
            kreg_load(kq, tb, S, lane);
            BR_ACC(cyc_lu, c1);
        }
        double delta[CPL];
#pragma unroll
        FOR_S delta[s] = 0.0;
        if (!lu_fail) {
            BR_CLK(c0);
            if constexpr (CPL == 1) {
                delta[0] = lu_solve<NMAX>(LUsave, nsys, lane, perm[0], b[0], scr);
                BR_X_AFTER_SOLVE();
            } else {
                lu_solve2<NMAX>(LUsave, scr, nsys, lane, perm, b);
                delta[0] = b[0];
                delta[1] = b[1];
            }
            BR_ACC(cyc_sol, c0);
        }
        BR_X_AFTER_ITER();
        BR_CLK(c3);
        if constexpr (ENERGY) act_code = ctl_post_solve<CPL, 64, vec_stride(NMAX), true>(C, V, lane, delta, lu_fail);
        else act_code = ctl_post_solve<CPL>(C, V, lane, delta, lu_fail);
        BR_ACC(cyc_ctl, c3);
        if (act_code == A_DONE) break;
    }
    const int status = ui(C->status);
#pragma unroll
    FOR_S {
        const double u_out = status ? V.at(0, s) : V.at(V_Y, s);
        if (CS < n) U[(size_t)rid * n + CS] = u_out;
        if constexpr (ENERGY) { if (o.T_end && CS == n) o.T_end[rid] = u_out; }
    }
    if (stats && lane == 0) {
        br_stats& s = stats[rid];
        s.nsteps = prev[P_NSTEPS] + ui(C->nst); s.nfe = prev[P_NFE] + ui(C->nfe); s.nje = prev[P_NJE] + ui(C->nje);
        s.nsetups = prev[P_NSETUPS] + ui(C->nsetups); s.nni = prev[P_NNI] + ui(C->nni); s.ncfn = prev[P_NCFN] + ui(C->ncfn);
        s.netf = prev[P_NETF] + ui(C->netf); s.status = (double)status;
        s.cyc_total = (double)(wall_clock64() - cyc0);
        BR_CLK_STORE(s);
        s.t_end = ud(C->tn);
        s.t_ign = o.ign >= 0 ? ud(C->t_ign) : NAN; s.ign_rate = o.ign >= 0 ? ud(C->ign_rate) : NAN;
        s.ign_dt = o.ign >= 0 ? ud(C->ign_dt) : NAN; s.nfe_dq = prev[P_NFE_DQ] + ui(C->nfe_dq);
    }
    }   // next reactor
}

// ------------------------------------------------------------------------------------
// parity kernels: rates, rhs, jacobian (one reactor per wave)
// ------------------------------------------------------------------------------------
template <int CPL>
__global__ __launch_bounds__(256) void k_rates(DevMech M, int N, int rpb, const double* Tv, const double* pv,
                                               const double* X, const double* TH, double* W_, double* SD, double* Jws) {
    typedef Lay<CPL> L;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const WaveCtx W = wave_ctx<CPL, CPL == 2 ? 72 : 64>(M, smem_raw, rpb, Jws);
    const int rid = W.rid;
    if (rid >= N) return;
    const int lane = W.lane;
    const RView& S = W.R;
    const double T = Tv[rid], p = pv[rid];
    init_tconst<CPL>(M, W.tb, S, T, lane);
    double cg = 0.0;
#pragma unroll
    FOR_S {
        const int k = CS;
        double c = 0.0;
        if (k < M.ng) c = p * X[(size_t)rid * M.ng + k] / (R_GAS * T);
        else if (k < M.n) c = TH ? TH[(size_t)rid * M.ns + (k - M.ng)] : 0.0;
        if (k < M.n) { S.sp[L::CONC + k] = c; S.sp[L::ACCW + k] = 0.0; S.sp[L::ACCS + k] = 0.0; }
        cg += k < M.ng ? c : 0.0;
    }
    const double Ctot = wave_sum(cg);
    wave_sync();
    third_body_sets<CPL>(M, W.tb, S.sp, Ctot, lane);
    wave_sync();
    production<CPL>(M, W.tb, S, R_GAS * T, lane, rx_prefetch(S, lane));
    wave_sync();
#pragma unroll
    FOR_S {
        const int k = CS;
        const double w = k < M.n ? S.sp[L::ACCW + k] : 0.0;
        const double sd = k < M.n ? S.sp[L::ACCS + k] : 0.0;
        if (k < M.ng) W_[(size_t)rid * M.ng + k] = w;
        if (SD && k < M.n) SD[(size_t)rid * M.n + k] = sd;
    }
}

template <int CPL>
__global__ __launch_bounds__(256) void k_rhs(DevMech M, int N, int rpb, const double* Tv, const double* Asvv,
                                             const double* U, double* DU, double* Jws) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const WaveCtx W = wave_ctx<CPL, CPL == 2 ? 72 : 64>(M, smem_raw, rpb, Jws);
    const int rid = W.rid;
    if (rid >= N) return;
    const int lane = W.lane;
    const RView& S = W.R;
    const double T = Tv[rid];
    const double Asv = Asvv ? Asvv[rid] : 1.0;
    const double Asv_th = (M.conv & 4) ? 1.0 : Asv;
    init_tconst<CPL>(M, W.tb, S, T, lane);
    double u[CPL], du[CPL];
#pragma unroll
    FOR_S u[s] = CS < M.n ? U[(size_t)rid * M.n + CS] : 0.0;
    rhs<CPL>(M, W.tb, S, T, Asv, Asv_th, u, lane, reinterpret_cast<double*>(W.rbase), du);
#pragma unroll
    FOR_S if (CS < M.n) DU[(size_t)rid * M.n + CS] = du[s];
}

template <int NMAX>
__global__ __launch_bounds__(256) void k_jac(DevMech M, int N, int rpb, const double* Tv, const double* Asvv,
                                             const double* U, double* J, double* Jws) {
    constexpr int CPL = NMAX > 64 ? 2 : 1;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const WaveCtx W = wave_ctx<CPL, NMAX>(M, smem_raw, rpb, Jws);
    const int rid = W.rid;
    if (rid >= N) return;
    const int lane = W.lane;
    const RView& S = W.R;
    const double T = Tv[rid];
    const double Asv = Asvv ? Asvv[rid] : 1.0;
    const double Asv_th = (M.conv & 4) ? 1.0 : Asv;
    init_tconst<CPL>(M, W.tb, S, T, lane);
    double u[CPL];
#pragma unroll
    FOR_S u[s] = CS < M.n ? U[(size_t)rid * M.n + CS] : 0.0;
    double* Jsave = Jws + (size_t)rid * ws_doubles(NMAX, M.nrg);
    jacobian<CPL>(M, W.tb, S, T, Asv, Asv_th, u, lane, Jsave, Jsave + NMAX * col_rows(NMAX));
#pragma unroll
    FOR_S {
        if (CS < M.n) {
            double* row = J + ((size_t)rid * M.n + CS) * M.n;
            for (int j = 0; j < M.n; ++j) row[j] = Jsave[j * col_rows(NMAX) + CS];
        }
    }
}

// br_phase_tout_dev: tout[i][j] = tau[j] * t_ign[i], NaN (no output) where t_ign is NaN or the product
// is past tf[i]. One thread per entry; one rounded product, so the host mirror (phase_grid of the
// Python package) gives the same bits.
__global__ __launch_bounds__(256) void k_phase_tout(int N, const br_stats* __restrict__ stats, int ntau,
                                                    const double* __restrict__ tau, const double* __restrict__ tfv,
                                                    double* __restrict__ tout) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)N * ntau) return;
    const size_t i = e / ntau;
    const int j = (int)(e - i * ntau);
    const double p = tau[j] * stats[i].t_ign;
    tout[e] = (p <= tfv[i]) ? p : NAN;
}

}  // namespace

// ------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------
// the kernel instances, one lookup per family (the kernels are emitted in the order of these functions)
// the group-engine instances (brhip_group.hpp; also of the test kernels of brhip_debug.hpp): f(GL, NM)
// as integral constants for the built pair (gl, nm), nullptr for any other
template <class F>
static const void* grp_instance(int gl, int nm, F f) {
    using std::integral_constant;
    if (gl == 16 && nm == 9) return f(integral_constant<int, 16>{}, integral_constant<int, 9>{});
    if (gl == 16 && nm == 16) return f(integral_constant<int, 16>{}, integral_constant<int, 16>{});
    if (gl == 32 && nm == 24) return f(integral_constant<int, 32>{}, integral_constant<int, 24>{});
    if (gl == 32 && nm == 32) return f(integral_constant<int, 32>{}, integral_constant<int, 32>{});
    return nullptr;
}
static const void* grp_kernel(int gl, int nm) {
    return grp_instance(gl, nm, [](auto g, auto w) { return (const void*)k_group<g(), w()>; });
}
static const void* grp_energy_kernel(int gl, int nm) {   // ... of an adiabatic run, (gl, nm) from ng + 1
    return grp_instance(gl, nm, [](auto g, auto w) { return (const void*)k_group<g(), w(), true>; });
}
static const void* wave_kernel(int nmax) {   // one reactor per wavefront
    return nmax == 16 ? (const void*)k_integrate<16> : nmax == 32 ? (const void*)k_integrate<32>
         : nmax == 56 ? (const void*)k_integrate<56> : nmax == 64 ? (const void*)k_integrate<64>
                                                                  : (const void*)k_integrate<72>;
}
static const void* wave_tprog_kernel(int nmax) {   // ... of a temperature-programme run
    return nmax == 16 ? (const void*)k_integrate<16, true> : nmax == 32 ? (const void*)k_integrate<32, true>
         : nmax == 56 ? (const void*)k_integrate<56, true> : nmax == 64 ? (const void*)k_integrate<64, true>
                                                                        : (const void*)k_integrate<72, true>;
}
static const void* wave_energy_kernel(int nmax) {   // ... of an adiabatic run, nmax from ng + 1 <= 56
    return nmax == 16 ? (const void*)k_integrate<16, false, true> : nmax == 32 ? (const void*)k_integrate<32, false, true>
         : nmax == 56 ? (const void*)k_integrate<56, false, true> : nullptr;
}
static const void* lane_kernel(int nm) { return nm == 9 ? (const void*)k_lane<9> : (const void*)k_lane<12>; }
// the parity kernels, by components per lane
static const void* rates_kernel(int cpl) { return cpl == 2 ? (const void*)k_rates<2> : (const void*)k_rates<1>; }
static const void* rhs_kernel(int cpl) { return cpl == 2 ? (const void*)k_rhs<2> : (const void*)k_rhs<1>; }
static const void* jac_kernel(int cpl) { return cpl == 2 ? (const void*)k_jac<72> : (const void*)k_jac<64>; }

// grow-only device buffer, freed with its owner
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { if (p) hipFree(p); }
    hipError_t ensure(size_t need) {
        if (bytes >= need) return hipSuccess;
        if (p) hipFree(p);
        p = nullptr; bytes = 0;
        const hipError_t e = hipMalloc(&p, need);
        if (e == hipSuccess) bytes = need;
        return e;
    }
    template <class T>
    T* as() const { return (T*)p; }
};

// The launch geometry of one integrator instance for one mechanism. A shape the mechanism does not have (state < 0)
// keeps every other field 0, so gl and nm also answer "eligible?".
struct Shape {
    int state = 0;       // 0: not looked for yet, 1: has one, -1: has none
    int gl = 0, nm = 0;  // instance widths: NMAX of k_integrate | GL (16: quad, 32: pair) and NM of k_group | NM of k_lane
    int threads = 0;     // per workgroup
    int rpb = 0;         // reactors per workgroup
    size_t shmem = 0;    // dynamic LDS bytes per workgroup
    int wg_per_cu = 0;   // resident workgroups per CU
};

struct br_mech {
    int device = 0;
    int ng = 0, ns = 0, nrg = 0, nrs = 0, n = 0, nmax = 64;
    DevMech dm{};
    size_t shmem1 = 0;
    std::vector<void*> allocs;   // the uploaded tables
    DevBuf ws;                   // staging of the host-buffer entry points (Stage)
    DevBuf jws;                  // wavefront engine: per-wave workspace slots (jws_bytes)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool ev_recorded = false;
    // the launch shapes, found in br_mech_create: the wavefront engine (always has one; the programme instances
    // run in it too), the one-reactor-per-lane engine (brhip_lane.hpp) and the group engine (brhip_group.hpp)
    Shape wave, lane, grp;
    // ... and those of the energy instances (brhip_energy.hpp), widths from ng + 1, each found at the first look
    // (energy_shape, group_energy_shape): wavefront (none: too large for the LDS) and group (none: surface species,
    // ng + 1 > 32, too many efficiency sets, or the LDS)
    Shape wave_e, grp_e;
    DevBuf lws;                  // lane engine: saved Jacobians, slot-major [NM*NM][slots]
    DevBuf queue;                // int[2 + DEFER_CAP]: work counter, deferred count, deferred reactors
    DevBuf qws;                  // group engines: saved Jacobians, 16 x 16 per group slot
    DevBuf wq;                   // int: k_integrate work counter
    DevBuf defer_t0;             // double[DEFER_CAP]: start time of each deferred lane reactor
    int ncu = 0;
    MultBlock* mult_hdr = nullptr;   // the 32 bytes in front of the g_par table (br_opts.rate_mult; brhip_device.hpp)
};

static thread_local std::string g_err;
// error message from the host mechanism compiler (mech_host.cpp, same library)
extern "C" __attribute__((visibility("hidden"))) void br_set_last_error(const char* msg) { g_err = msg; }
static int fail(int code, const std::string& msg) { g_err = msg; return code; }
static int fail_code_input() { return fail(BR_ERR_INPUT, "bad argument"); }
#define HIPCHK(x)                                                                         \
    do {                                                                                  \
        hipError_t e_ = (x);                                                              \
        if (e_ != hipSuccess) return fail(BR_ERR_HIP, std::string(#x ": ") + hipGetErrorString(e_)); \
    } while (0)

template <class T>
static int upload(br_mech* m, const std::vector<T>& v, const T** out) {
    void* p = nullptr;
    size_t b = std::max<size_t>(v.size(), 1) * sizeof(T);
    HIPCHK(hipMalloc(&p, b));
    m->allocs.push_back(p);
    if (!v.empty()) HIPCHK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    *out = (const T*)p;
    return 0;
}

// Host arrays of the host-buffer entry points, staged back to back in m->ws: reserve the total, then
// take the pieces in order. push copies a host array into the next piece (nullptr: the piece alone);
// the first failed copy is kept in err.
struct Stage {
    double* next = nullptr;
    hipError_t err = hipSuccess;
    hipError_t reserve(br_mech* m, size_t doubles) {
        const hipError_t e = m->ws.ensure(doubles * sizeof(double));
        next = m->ws.as<double>();
        return e;
    }
    double* take(size_t count) { double* d = next; next += count; return d; }
    void put(double* dev, const double* host, size_t count) {
        if (!host || !count) return;
        const hipError_t e = hipMemcpy(dev, host, count * sizeof(double), hipMemcpyHostToDevice);
        if (err == hipSuccess) err = e;
    }
    double* push(const double* host, size_t count) { double* d = take(count); put(d, host, count); return d; }
};

// Workgroups of `threads` threads and `shmem` bytes of dynamic LDS of kernel `fn` that are resident per CU, from the
// occupancy calculator (VGPRs, LDS); -1 when shmem is over lds_limit or a call fails. Leaves shmem as the
// kernel's dynamic-LDS attribute.
static int resident_per_cu(const void* fn, int threads, size_t shmem, size_t lds_limit = LDS_PER_CU, bool whole_granules = true) {
    if (shmem > lds_limit) return -1;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem) != hipSuccess) return -1;
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, threads, shmem) != hipSuccess) return -1;
    // the calculator ignores the LDS allocation granule: 3 x 54.5 KB workgroups were reported
    // resident but only 2 were (measured: 6 of 9 waves/CU); count whole granules per CU
    if (whole_granules) nb = std::min(nb, (int)(LDS_PER_CU / ((shmem + LDS_GRANULE - 1) / LDS_GRANULE * LDS_GRANULE)));
    return std::max(nb, 0);
}
// The shape of a wavefront-engine instance k_integrate<nmax, ...>: the reactors (waves) per workgroup that maximise
// the resident waves per CU, with lds_bytes(rpb) of LDS (tables once per workgroup + one block per reactor); ties
// go to the smaller workgroup. None when not even one reactor fits.
template <class F>
static Shape wave_shape(const void* kfn, int nmax, F lds_bytes) {
    Shape best{-1};
    for (int rpb = 1; rpb <= br_maxrpb(nmax); ++rpb) {
        const size_t b = lds_bytes(rpb);
        const int nb = resident_per_cu(kfn, 64 * rpb, b);
        if (nb < 0) break;
        if (nb * rpb > best.wg_per_cu * best.rpb) best = Shape{1, 0, nmax, 64 * rpb, rpb, b, nb};
    }
    return best;
}
// The shape of the group instance (brhip_group.hpp) of a system of nsys equations with nrs surface reactions:
// 4 reactors per wave for nsys <= 16, 2 for nsys <= 32, BR_QWPB waves per workgroup, k_group<GL, NM, ...> from
// `kernel` (grp_kernel, grp_energy_kernel). None when nsys or the efficiency sets are too many, or by the LDS.
static Shape group_shape(const br_mech* m, int nsys, int nrs, const void* (*kernel)(int gl, int nm)) {
    if (nsys > 32 || m->dm.nset > grp::MAX_SETS) return Shape{-1};
    const int gl = nsys <= 16 ? 16 : 32, nm = nsys <= 9 ? 9 : (nsys <= 16 ? 16 : (nsys <= 24 ? 24 : 32));
    const int rpb = BR_QWPB * (64 / gl);
    const size_t shmem = (size_t)m->dm.img_bytes + (size_t)rpb * grp::block_bytes(gl, nm, m->nrg, m->dm.nfo, nrs);
    const int nb = resident_per_cu(kernel(gl, nm), 64 * BR_QWPB, shmem);
    return nb > 0 ? Shape{1, gl, nm, 64 * BR_QWPB, rpb, shmem, nb} : Shape{-1};
}

extern "C" {

int br_version(void) { return 232; }   // 232: br_debug_wave_lu; 231: br_mech_energy_launch_info, br_debug_group_energy_eval (br_opts as in 230)
const char* br_last_error(void) { return g_err.c_str(); }
int br_device_count(void) {
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) return 0;
    return c;
}

int br_mech_info(const br_mech* m, int* ng, int* ns, int* nrg, int* nrs) {
    if (!m) return fail(BR_ERR_INPUT, "null mech");
    if (ng) *ng = m->ng;
    if (ns) *ns = m->ns;
    if (nrg) *nrg = m->nrg;
    if (nrs) *nrs = m->nrs;
    return 0;
}

// engine selection for br_integrate* (untraced): BRHIP_ENGINE = wave | lane | quad | pair forces one
// (when the mechanism is eligible); default: the group engine for eligible mechanisms (quad, n <= 16:
// C2 H2/O2 882k reactors/s against 477k for the lane engine and 470k for the wavefront engine, round
// 4; pair, 16 < n <= 32, when BR_PAIR_DEFAULT: off, surface-only Ni/CH4 194.8k vs 217.7k for the
// wavefront engine), else the lane engine, else the wavefront engine.
// Codes: 0 wavefront, NM > 0 lane, -(100 gl + NM) group.
#ifndef BR_QUAD_DEFAULT
#define BR_QUAD_DEFAULT 1
#endif
#ifndef BR_PAIR_DEFAULT
#define BR_PAIR_DEFAULT 0
#endif
static int pick_engine(const br_mech* m) {
    const char* eng = getenv("BRHIP_ENGINE");
    if (eng && strcmp(eng, "wave") == 0) return 0;
    if (eng && strcmp(eng, "lane") == 0) return m->lane.nm;
    const int gcode = -(100 * m->grp.gl + m->grp.nm);
    if (m->grp.gl == 16 && ((eng && strcmp(eng, "quad") == 0) || (!eng && BR_QUAD_DEFAULT))) return gcode;
    if (m->grp.gl == 32 && ((eng && strcmp(eng, "pair") == 0) || (!eng && BR_PAIR_DEFAULT))) return gcode;
    return m->lane.nm;
}
int br_mech_engine(const br_mech* m) {
    if (!m) return fail(BR_ERR_INPUT, "null mechanism");
    return pick_engine(m);
}

// what the launch-info entry points report of a shape (each through its pointer, when given): reactors per
// workgroup, resident waves per CU, LDS bytes per workgroup, reactors resident on the device
static void report_shape(const Shape& sh, int ncu, int* rpb, int* waves_per_cu, long long* lds_bytes, int* resident) {
    if (rpb) *rpb = sh.rpb;
    if (waves_per_cu) *waves_per_cu = sh.wg_per_cu * (sh.threads / 64);
    if (lds_bytes) *lds_bytes = (long long)sh.shmem;
    if (resident) *resident = std::max(ncu, 1) * sh.wg_per_cu * sh.rpb;
}

int br_mech_launch_info(const br_mech* m, int* rpb, int* waves_per_cu, long long* lds_bytes) {
    if (!m) return fail(BR_ERR_INPUT, "null mechanism");
    // the geometry of the engine br_integrate launches (pick_engine), not always the wavefront one
    const int e = pick_engine(m);
    report_shape(e < 0 ? m->grp : e > 0 ? m->lane : m->wave, m->ncu, rpb, waves_per_cu, lds_bytes, nullptr);
    return 0;
}

int br_mech_create(const br_mech_desc* d, int device, br_mech** out) {
    if (!d || !out) return fail(BR_ERR_INPUT, "null argument");
    const int ng = d->ng, ns = d->ns, nrg = d->nrg, nrs = d->nrs, n = ng + ns;
    if (ng <= 0 || ns < 0 || nrg < 0 || nrs < 0) return fail(BR_ERR_INPUT, "bad sizes");
    if (n > 72) return fail(BR_ERR_UNSUPPORTED, "n > 72 components is not supported by this build");
    // ---- the DevMech block and the tables (mech_pack.cpp: host arithmetic only)
    const char* ss = getenv("BRHIP_SPREAD");   // "0": scatter lists in first-appearance order (A/B)
    const char* jf = getenv("BRHIP_JFAST");    // "0": the general column-list Jacobian (A/B)
    PackOpts po;
    po.spread = !(ss && atoi(ss) == 0);
    po.allow_jfast = !(jf && atoi(jf) == 0);
    PackedMech pk;
    std::string perr;
    if (const int prc = mech_pack(d, po, &pk, &perr)) return fail(prc, perr);
    HIPCHK(hipSetDevice(device));
    std::unique_ptr<br_mech, int (*)(br_mech*)> owner(new br_mech(), br_mech_destroy);   // frees on every early return
    br_mech* m = owner.get();
    m->device = device; m->ng = ng; m->ns = ns; m->nrg = nrg; m->nrs = nrs; m->n = n;
    m->nmax = nmax_of(n);
    m->dm = pk.dm;
    DevMech& M = m->dm;
    int rc = 0;
    rc |= upload(m, pk.img, &M.img);
    rc |= upload(m, pk.nasa, &M.nasa); rc |= upload(m, pk.g_dnu, &M.g_dnu);
    {   // g_par behind its MultBlock header: the permutation and the row length now, the table per launch
        const int* dperm = nullptr;
        rc |= upload(m, pk.g_perm, &dperm);
        const MultBlock hdr{nullptr, nullptr, dperm, nrg + nrs, 0};
        std::vector<double> gp(MULT_HDR_DOUBLES + pk.g_par.size());
        memcpy(gp.data(), &hdr, sizeof hdr);
        std::copy(pk.g_par.begin(), pk.g_par.end(), gp.begin() + MULT_HDR_DOUBLES);
        const double* dgp = nullptr;
        rc |= upload(m, gp, &dgp);
        if (!rc) { m->mult_hdr = (MultBlock*)dgp; M.g_par = dgp + MULT_HDR_DOUBLES; }
    }
    rc |= upload(m, pk.fo_par, &M.fo_par); rc |= upload(m, pk.s_par, &M.s_par);
    rc |= upload(m, pk.tb_eff, &M.tb_eff); rc |= upload(m, pk.col_ptr, &M.col_ptr); rc |= upload(m, pk.col_rx, &M.col_rx);
    if (rc) return rc;
    HIPCHK(hipDeviceGetAttribute(&m->ncu, hipDeviceAttributeMultiprocessorCount, device));
    // ---- the launch shapes (the energy instances': at the first look)
    m->wave = wave_shape(wave_kernel(m->nmax), m->nmax, [&](int rpb) { return wg_lds_bytes(M, rpb); });
    if (m->wave.state < 0) return fail(BR_ERR_UNSUPPORTED, "mechanism too large for LDS");
    m->shmem1 = wg_lds_bytes(M, 1);
    // one-reactor-per-lane engine for small gas-only mechanisms (brhip_lane.hpp): one wave of 64 reactors per
    // workgroup, at most 64 KB of LDS, residency as the calculator gives it (no granule count)
    m->lane.state = -1;
    if (ns == 0 && n <= 12) {
        const int nm = n <= 9 ? 9 : 12;
        const size_t shmem = lane_lds_bytes(nm, n, M.nset, nrg, M.nfo);
        const int nb = resident_per_cu(lane_kernel(nm), 64, shmem, 64 * 1024, false);
        if (nb > 0) m->lane = Shape{1, 0, nm, 64, 64, shmem, nb};   // (else it does not fit: the wave engine integrates it)
    }
    m->grp = group_shape(m, n, nrs, grp_kernel);
    HIPCHK(hipEventCreate(&m->ev0));
    HIPCHK(hipEventCreate(&m->ev1));
    *out = owner.release();
    return 0;
}

int br_mech_destroy(br_mech* m) {
    if (!m) return 0;
    hipSetDevice(m->device);
    for (void* p : m->allocs) hipFree(p);
    if (m->ev0) hipEventDestroy(m->ev0);
    if (m->ev1) hipEventDestroy(m->ev1);
    delete m;   // (the DevBuf members free theirs)
    return 0;
}

constexpr int DEFER_CAP = 4096;   // reactors one k_lane pass may hand to the wavefront engine
// wavefront-engine and parity-kernel workspace (m->jws): one slot per reactor in flight
static size_t jws_bytes(const br_mech* m, int N) {
    return (size_t)N * ws_doubles(std::max(m->nmax, 64), m->nrg) * sizeof(double);
}

int br_rates(br_mech* m, int N, const double* T, const double* p, const double* x, const double* theta, double* wdot,
             double* sdot) {
    if (!m || N < 0 || !T || !p || !x || !wdot) return fail(BR_ERR_INPUT, "bad argument");
    if (N == 0) return 0;
    HIPCHK(hipSetDevice(m->device));
    const int ng = m->ng, ns = m->ns, n = m->n;
    Stage st;
    HIPCHK(st.reserve(m, (size_t)N * (2 + ng + ns) + (size_t)N * (ng + n)));
    HIPCHK(m->jws.ensure(jws_bytes(m, N)));   // per-reactor slots: {kf, kr} per gas reaction
    const double* dT = st.push(T, N);
    const double* dp = st.push(p, N);
    const double* dx = st.push(x, (size_t)N * ng);
    double* dth = st.push(theta, (size_t)N * ns);
    double* dw = st.take((size_t)N * ng);
    double* ds = st.take((size_t)N * n);
    HIPCHK(st.err);
    if (ns && !theta) HIPCHK(hipMemset(dth, 0, (size_t)N * ns * sizeof(double)));
    const void* fn = rates_kernel(m->dm.cpl);
    HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)m->shmem1));
    const DevMech dm = m->dm;
    const int rpb = 1;
    const double* pth = ns ? dth : nullptr;
    double* jws = m->jws.as<double>();
    void* args[] = {(void*)&dm, (void*)&N, (void*)&rpb, (void*)&dT, (void*)&dp, (void*)&dx, (void*)&pth, (void*)&dw, (void*)&ds, (void*)&jws};
    HIPCHK(hipLaunchKernel(fn, dim3(N), dim3(64), args, m->shmem1, 0));
    HIPCHK(hipMemcpy(wdot, dw, (size_t)N * ng * sizeof(double), hipMemcpyDeviceToHost));
    if (sdot) HIPCHK(hipMemcpy(sdot, ds, (size_t)N * n * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

// br_rhs and br_jacobian: k_rhs / k_jac on N staged reactors, `nres` doubles of result per reactor
static int eval_staged(br_mech* m, const void* fn, int N, const double* T, const double* Asv, const double* u, size_t nres,
                       double* res) {
    HIPCHK(hipSetDevice(m->device));
    const int n = m->n;
    Stage st;
    HIPCHK(st.reserve(m, (size_t)N * (2 + n + nres)));
    const double* dT = st.push(T, N);
    const double* dA = st.push(Asv, N);
    const double* du = st.push(u, (size_t)N * n);
    double* dres = st.take((size_t)N * nres);
    HIPCHK(st.err);
    HIPCHK(m->jws.ensure(jws_bytes(m, N)));   // per-reactor slots: {kf, kr} per gas reaction, Jacobian columns
    HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)m->shmem1));
    const DevMech dm = m->dm;
    const int rpb = 1;
    const double* pA = Asv ? dA : nullptr;
    double* jws = m->jws.as<double>();
    void* args[] = {(void*)&dm, (void*)&N, (void*)&rpb, (void*)&dT, (void*)&pA, (void*)&du, (void*)&dres, (void*)&jws};
    HIPCHK(hipLaunchKernel(fn, dim3(N), dim3(64), args, m->shmem1, 0));
    HIPCHK(hipMemcpy(res, dres, (size_t)N * nres * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

int br_rhs(br_mech* m, int N, const double* T, const double* Asv, const double* u, double* du) {
    if (!m || N < 0 || !T || !u || !du) return fail(BR_ERR_INPUT, "bad argument");
    if (N == 0) return 0;
    return eval_staged(m, rhs_kernel(m->dm.cpl), N, T, Asv, u, m->n, du);
}

int br_jacobian(br_mech* m, int N, const double* T, const double* Asv, const double* u, double* J) {
    if (!m || N < 0 || !T || !u || !J) return fail(BR_ERR_INPUT, "bad argument");
    if (N == 0) return 0;
    return eval_staged(m, jac_kernel(m->dm.cpl), N, T, Asv, u, (size_t)m->n * m->n, J);
}

// does this br_opts ask for outputs (nout > 0 and both arrays), and on one grid per reactor?
struct OutReq {
    int nout;
    bool per;
};
static OutReq out_request(const br_opts* opts) {
    const int nout = (opts && opts->nout > 0 && opts->tout && opts->yout) ? opts->nout : 0;
    return {nout, nout && opts->tout_per_reactor};
}

// rate multipliers of a br_opts (nmult > 0): the shape checks every entry point shares
static int mult_request(int N, const br_opts* opts) {
    if (!opts || opts->nmult == 0) return 0;
    if (opts->nmult < 0 || !opts->rate_mult) return fail(BR_ERR_INPUT, "nmult > 0 needs rate_mult[nmult][nrg+nrs]");
    if (!opts->rate_mult_row && opts->nmult != N)
        return fail(BR_ERR_INPUT, "rate_mult_row is NULL: nmult must be N = " + std::to_string(N) + ", got " +
                                      std::to_string(opts->nmult));
    return 0;
}
// ... and the contents, for host arrays: every multiplier finite and >= 0, every row index in range
static int check_mult_host(const br_mech* m, int N, const br_opts* opts) {
    if (const int rc = mult_request(N, opts)) return rc;
    if (!opts || opts->nmult == 0) return 0;
    const int nr = m->nrg + m->nrs;
    for (int q = 0; q < opts->nmult; ++q)
        for (int r = 0; r < nr; ++r) {
            const double v = opts->rate_mult[(size_t)q * nr + r];
            if (!(v >= 0.0) || !(v < INFINITY))
                return fail(BR_ERR_INPUT, "rate_mult[" + std::to_string(q) + "][" + std::to_string(r) + "] = " +
                                              std::to_string(v) + ": multipliers must be finite and >= 0");
        }
    for (int i = 0; i < N && opts->rate_mult_row; ++i)
        if (opts->rate_mult_row[i] < 0 || opts->rate_mult_row[i] >= opts->nmult)
            return fail(BR_ERR_INPUT, "rate_mult_row[" + std::to_string(i) + "] = " + std::to_string(opts->rate_mult_row[i]) +
                                          " is outside [0, nmult = " + std::to_string(opts->nmult) + ")");
    return 0;
}
// doubles of staging the host multiplier arrays take (table, then the row indices as ints), and the copy:
// od's pointers become the device ones
static size_t mult_stage_doubles(const br_mech* m, int N, const br_opts* opts) {
    if (!opts || opts->nmult <= 0) return 0;
    return (size_t)opts->nmult * (m->nrg + m->nrs) + (opts->rate_mult_row ? ((size_t)N + 1) / 2 : 0);
}
static void stage_mult(Stage& st, const br_mech* m, int N, const br_opts* opts, br_opts* od) {
    if (!opts || opts->nmult <= 0) return;
    od->rate_mult = st.push(opts->rate_mult, (size_t)opts->nmult * (m->nrg + m->nrs));
    if (opts->rate_mult_row) {
        int* drow = (int*)st.take(((size_t)N + 1) / 2);
        const hipError_t e = hipMemcpy(drow, opts->rate_mult_row, (size_t)N * sizeof(int), hipMemcpyHostToDevice);
        if (st.err == hipSuccess) st.err = e;
        od->rate_mult_row = drow;
    }
}

// temperature programmes of a br_opts (ntprog > 0): the shape checks every entry point shares
static int tprog_shape(int N, int ntprog, const double* t, const double* T, int nrows, const int* row) {
    if (ntprog < 0 || !t || !T || nrows < 1)
        return fail(BR_ERR_INPUT, "ntprog > 0 needs tprog_t and tprog_T [ntprog_rows][ntprog], ntprog_rows >= 1");
    if (!row && nrows != N)
        return fail(BR_ERR_INPUT, "tprog_row is NULL: ntprog_rows must be N = " + std::to_string(N) + ", got " +
                                      std::to_string(nrows));
    return 0;
}
static int tprog_request(int N, const br_opts* opts) {
    if (!opts || opts->ntprog == 0) return 0;
    return tprog_shape(N, opts->ntprog, opts->tprog_t, opts->tprog_T, opts->ntprog_rows, opts->tprog_row);
}
// ... and the contents, for host arrays. A row: first time 0, times ascending, NaN only as trailing padding,
// temperatures at the knots finite and > 0. The message names the first reactor that has a bad row index
// or uses a bad row, and the row (i0: the index of reactor 0 in the caller's ensemble)
static std::string tprog_row_defect(int nk, const double* t, const double* T) {
    if (!(t[0] == 0.0)) return "its first knot time is " + std::to_string(t[0]) + ", not 0";
    bool pad = false;
    for (int j = 0; j < nk; ++j) {
        if (t[j] != t[j]) { pad = true; continue; }
        if (pad) return "knot time " + std::to_string(j) + " follows a NaN (NaN is trailing padding only)";
        if (j && !(t[j] >= t[j - 1])) return "knot times must be ascending (knot " + std::to_string(j) + ")";
        if (!(t[j] < INFINITY)) return "knot time " + std::to_string(j) + " is not finite";
        if (!(T[j] > 0.0) || !(T[j] < INFINITY))
            return "T = " + std::to_string(T[j]) + " at knot " + std::to_string(j) + ": temperatures must be finite and > 0";
    }
    return "";
}
static int check_tprog_arrays(int N, int nk, const double* t, const double* T, int nrows, const int* row) {
    if (const int rc = tprog_shape(N, nk, t, T, nrows, row)) return rc;
    std::vector<std::string> defect(nrows);
    for (int r = 0; r < nrows; ++r) defect[r] = tprog_row_defect(nk, t + (size_t)r * nk, T + (size_t)r * nk);
    for (int i = 0; i < N; ++i) {
        const int r = row ? row[i] : i;
        if (r < 0 || r >= nrows)
            return fail(BR_ERR_INPUT, "tprog_row[" + std::to_string(i) + "] = " + std::to_string(r) +
                                          " is outside [0, ntprog_rows = " + std::to_string(nrows) + "): reactor " + std::to_string(i));
        if (!defect[r].empty())
            return fail(BR_ERR_INPUT, "temperature programme of reactor " + std::to_string(i) + " (row " + std::to_string(r) +
                                          "): " + defect[r]);
    }
    for (int r = 0; r < nrows; ++r)   // (a row no reactor uses is checked all the same)
        if (!defect[r].empty())
            return fail(BR_ERR_INPUT, "temperature programme row " + std::to_string(r) + " (used by no reactor): " + defect[r]);
    return 0;
}
static int check_tprog_host(int N, const br_opts* opts) {
    if (!opts || opts->ntprog == 0) return 0;
    return check_tprog_arrays(N, opts->ntprog, opts->tprog_t, opts->tprog_T, opts->ntprog_rows, opts->tprog_row);
}
// doubles of staging the host programme arrays take (times, temperatures, then the row indices as ints), and the
// copy: od's pointers become the device ones
static size_t tprog_stage_doubles(int N, const br_opts* opts) {
    if (!opts || opts->ntprog <= 0) return 0;
    return 2 * (size_t)opts->ntprog_rows * opts->ntprog + (opts->tprog_row ? ((size_t)N + 1) / 2 : 0);
}
static void stage_tprog(Stage& st, int N, const br_opts* opts, br_opts* od) {
    if (!opts || opts->ntprog <= 0) return;
    const size_t ne = (size_t)opts->ntprog_rows * opts->ntprog;
    od->tprog_t = st.push(opts->tprog_t, ne);
    od->tprog_T = st.push(opts->tprog_T, ne);
    if (opts->tprog_row) {
        int* drow = (int*)st.take(((size_t)N + 1) / 2);
        const hipError_t e = hipMemcpy(drow, opts->tprog_row, (size_t)N * sizeof(int), hipMemcpyHostToDevice);
        if (st.err == hipSuccess) st.err = e;
        od->tprog_row = drow;
    }
}

// an energy run of a br_opts: the checks that need no handle (a bad value, together with a programme) ...
static int energy_request(const br_opts* opts) {
    if (!opts || opts->energy == 0) return 0;
    if (opts->energy != BR_ENERGY_ADIABATIC_V)
        return fail(BR_ERR_INPUT, "br_opts.energy = " + std::to_string(opts->energy) + ": 0 or BR_ENERGY_ADIABATIC_V (1)");
    if (opts->ntprog != 0)
        return fail(BR_ERR_INPUT, "br_opts.energy together with a temperature programme (br_opts.ntprog): T is either "
                                  "integrated or prescribed");
    return 0;
}
// ... and those on the mechanism, with the launch shape of its energy instance (the occupancy search of
// br_mech_create on that kernel and its LDS block), kept in the handle
static int energy_shape(br_mech* m) {
    if (m->ns > 0)
        return fail(BR_ERR_UNSUPPORTED, "br_opts.energy: mechanisms with surface species are not supported (gas-only)");
    if (m->ng + 1 > 56)
        return fail(BR_ERR_UNSUPPORTED, "br_opts.energy: ng + 1 = " + std::to_string(m->ng + 1) +
                                            " components exceed the 56 of the widest energy instance");
    if (!m->wave_e.state) {
        const int nmax = nmax_of(m->ng + 1);
        m->wave_e = wave_shape(wave_energy_kernel(nmax), nmax, [&](int rpb) { return energy_wg_lds_bytes(m->dm, nmax, rpb); });
    }
    if (m->wave_e.state < 0) return fail(BR_ERR_UNSUPPORTED, "br_opts.energy: mechanism too large for LDS");
    return 0;
}

// the group energy instance of a mechanism (brhip_group.hpp, k_group<GL, NM, true>): (GL, NM) from nsys = ng + 1,
// one shape up from the isothermal instance where ng = 9, 16 or 24; its own LDS block and residency, kept in
// the handle. Returns whether the mechanism has one.
static bool group_energy_shape(br_mech* m) {
    if (!m->grp_e.state) m->grp_e = m->ns > 0 ? Shape{-1} : group_shape(m, m->ng + 1, 0, grp_energy_kernel);
    return m->grp_e.state > 0;
}
// engine of an energy run (codes of br_mech_engine): the group energy instance when BRHIP_ENGINE asks for the
// group width ng + 1 selects (quad: ng + 1 <= 16, pair: 16 < ng + 1 <= 32) and the mechanism has one; in every
// other case -- BRHIP_ENGINE unset, wave, lane, the other width, an ineligible mechanism -- 0, the wavefront
// energy instance
static int pick_energy_engine(br_mech* m) {
    const char* eng = getenv("BRHIP_ENGINE");
    if (!eng) return 0;
    const int nsys = m->ng + 1;
    const bool quad = strcmp(eng, "quad") == 0 && nsys <= 16, pair = strcmp(eng, "pair") == 0 && nsys > 16 && nsys <= 32;
    if (!(quad || pair) || !group_energy_shape(m)) return 0;
    return -(100 * m->grp_e.gl + m->grp_e.nm);
}

// the kernel options of a run: br_opts with its defaults filled in (no work list, no deferral)
static KOpts make_kopts(const br_mech* m, const br_opts* opts, bool traced) {
    KOpts o;
    o.rtol = (opts && opts->rtol > 0) ? opts->rtol : 1e-6;
    o.atol = (opts && opts->atol > 0) ? opts->atol : 1e-10;
    o.max_steps = (opts && opts->max_steps > 0) ? opts->max_steps : 100000;
    o.hmax_inv = (opts && opts->hmax > 0) ? 1.0 / opts->hmax : 0.0;
    o.trace_cap = (opts && traced) ? opts->trace_cap : 0;
    o.ufac = opts ? opts->unstable_factor : 0.0;          // <= 0: NaN check only (SciML default)
    o.ign = (opts && opts->ignition_species > 0 && opts->ignition_species <= m->ng) ? opts->ignition_species - 1 : -1;
    const OutReq rq = out_request(opts);
    o.nout = rq.nout;
    o.tout = rq.nout ? tout_tag(opts->tout, rq.per) : nullptr;
    o.yout = rq.nout ? opts->yout : nullptr;
    o.dq_jac = (opts && opts->dq_jacobian) ? 1 : 0;
    o.defer_steps = o.max_steps;
    o.rid_list = nullptr;
    o.rid_count = nullptr;
    o.rid_t0 = nullptr;
    o.work = nullptr;
    return o;
}

// The instance families of a run. The kernel options of each begin with the run's KOpts: ISOTHERMAL takes KOpts
// itself, PROGRAMME KOptsProg (+ the programme block), ENERGY KOptsEnergy (+ the T outputs).
enum Flavour { ISOTHERMAL, PROGRAMME, ENERGY };
static KOptsEnergy energy_kopts(const KOpts& o, const br_opts* opts) {
    KOptsEnergy oe;
    static_cast<KOpts&>(oe) = o;
    oe.T_end = opts->T_end;
    oe.T_out = o.nout ? opts->T_out : nullptr;
    return oe;
}

// k_integrate of flavour `fl` and shape `sh` on `nwg` workgroups of sh.rpb reactors (waves) each
// (opts: read for a programme's block and an energy run's T outputs only)
static int launch_wave(br_mech* m, Flavour fl, const Shape& sh, const DevMech& dm, int N, int nwg, const double* dT,
                       const double* dAsv, double* du, const double* dtf, const KOpts& o, const br_opts* opts,
                       br_stats* dstats, double* trace, hipStream_t s) {
    const void* fn = fl == PROGRAMME ? wave_tprog_kernel(sh.nm) : fl == ENERGY ? wave_energy_kernel(sh.nm) : wave_kernel(sh.nm);
    HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh.shmem));
    const int rpb = sh.rpb;
    double* jws = m->jws.as<double>();
    KOptsProg op;
    KOptsEnergy oe;
    const void* ko = &o;
    if (fl == PROGRAMME) {
        static_cast<KOpts&>(op) = o;
        op.prog = TProg{opts->tprog_t, opts->tprog_T, opts->tprog_row, opts->ntprog, 0};
        ko = &op;
    } else if (fl == ENERGY) {
        oe = energy_kopts(o, opts);
        ko = &oe;
    }
    void* args[] = {(void*)&dm, (void*)&N, (void*)&rpb, (void*)&dT, (void*)&dAsv, (void*)&du, (void*)&dtf,
                    (void*)ko, (void*)&dstats, (void*)&jws, (void*)&trace};
    HIPCHK(hipLaunchKernel(fn, dim3(nwg), dim3(64 * rpb), args, sh.shmem, s));
    return 0;
}

// The wavefront engine's run. Persistent grid: as many workgroups as are resident at once, reactors from a work
// counter (BRHIP_STATIC=1: one reactor per wave over ceil(N / rpb) workgroups).
static int launch_wave_grid(br_mech* m, Flavour fl, const Shape& sh, const DevMech& dm, int N, const double* dT,
                            const double* dAsv, double* du, const double* dtf, KOpts o, const br_opts* opts,
                            br_stats* dstats, double* trace, hipStream_t s) {
    const int rpb = sh.rpb;
    const char* st_env = getenv("BRHIP_STATIC");
    const bool dyn = !(st_env && atoi(st_env) == 1) && m->ncu > 0;
    const int nwg_all = (N + rpb - 1) / rpb;
    const int nwg = dyn ? std::min(nwg_all, m->ncu * sh.wg_per_cu) : nwg_all;
    HIPCHK(m->jws.ensure(jws_bytes(m, nwg * rpb)));   // (slots of the 64-wide layout: no narrower than an energy instance's)
    if (dyn) {
        HIPCHK(m->wq.ensure(sizeof(int)));
        HIPCHK(hipMemsetAsync(m->wq.p, 0, sizeof(int), s));
        o.work = m->wq.as<int>();
    }
    HIPCHK(hipEventRecord(m->ev0, s));
    if (const int rc = launch_wave(m, fl, sh, dm, N, nwg, dT, dAsv, du, dtf, o, opts, dstats, trace, s)) return rc;
    HIPCHK(hipEventRecord(m->ev1, s));
    m->ev_recorded = true;
    return 0;
}

// A group engine's run on instance `gfn` of shape `sh`: 2 or 4 reactors per wave (one per 32- / 16-lane group),
// persistent grid over the resident workgroups, reactors from a work counter, m->qws sized by the instance's slot.
// `o`: the instance's options, KOpts or the KOptsEnergy that begins with it (the kernel reads the whole struct).
static int launch_group(br_mech* m, const Shape& sh, const void* gfn, const DevMech& dm, int N, const double* dT,
                        const double* dAsv, double* du, const double* dtf, KOpts* o, br_stats* dstats, hipStream_t s) {
    const int blocks = std::max(1, std::min((N + sh.rpb - 1) / sh.rpb, sh.wg_per_cu * std::max(m->ncu, 1)));
    HIPCHK(m->qws.ensure((size_t)blocks * sh.rpb * grp::slot_doubles(sh.gl, m->nrg) * sizeof(double)));
    HIPCHK(m->queue.ensure((2 + DEFER_CAP) * sizeof(int)));
    HIPCHK(hipMemsetAsync(m->queue.p, 0, 2 * sizeof(int), s));
    o->work = m->queue.as<int>();
    HIPCHK(hipFuncSetAttribute(gfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh.shmem));
    HIPCHK(hipEventRecord(m->ev0, s));
    double* qws = m->qws.as<double>();
    void* args[] = {(void*)&dm, (void*)&N, (void*)&dT, (void*)&dAsv, (void*)&du, (void*)&dtf, (void*)o, (void*)&dstats, (void*)&qws};
    HIPCHK(hipLaunchKernel(gfn, dim3(blocks), dim3(sh.threads), args, sh.shmem, s));
    HIPCHK(hipEventRecord(m->ev1, s));
    m->ev_recorded = true;
    return 0;
}

int br_mech_energy_launch_info(br_mech* m, int* engine, int* rpb, int* waves_per_cu, long long* lds_bytes, int* resident) {
    if (!m) return fail(BR_ERR_INPUT, "null mechanism");
    HIPCHK(hipSetDevice(m->device));
    if (const int rc = energy_shape(m)) return rc;
    const int e = pick_energy_engine(m);
    if (engine) *engine = e;
    report_shape(e < 0 ? m->grp_e : m->wave_e, m->ncu, rpb, waves_per_cu, lds_bytes, resident);
    return 0;
}

static int integrate_dev(br_mech* m, int N, const double* dT, const double* dAsv, double* du, const double* dtf,
                         const br_opts* opts, br_stats* dstats, void* stream, double* trace) {
    if (const int rc = energy_request(opts)) return rc;   // (before the handle is looked at, as the programme checks)
    const bool prog = opts && opts->ntprog != 0;   // a temperature programme: dT is not read
    const bool energy = opts && opts->energy != 0;
    if (!m || N < 0 || (!dT && !prog) || !du || !dtf) return fail(BR_ERR_INPUT, "bad argument");
    if (const int rc = tprog_request(N, opts)) return rc;
    if (energy && trace)
        return fail(BR_ERR_UNSUPPORTED, "br_integrate_traced does not take br_opts.energy: the trace row has no T column");
    if (N == 0) return 0;
    HIPCHK(hipSetDevice(m->device));
    if (energy) { if (const int rc = energy_shape(m)) return rc; }
    KOpts o = make_kopts(m, opts, trace != nullptr);
    hipStream_t s = (hipStream_t)stream;
    DevMech dm = m->dm;
    if (const int rc = mult_request(N, opts)) return rc;
    if (opts && opts->nmult > 0) {
        // rate multipliers: the launch's table and row indices into the block in front of g_par (on this
        // stream), and the tag on the launch's copy of the pointer that makes the init functions read it
        hipLaunchKernelGGL(k_mult_block, dim3(1), dim3(64), 0, s, m->mult_hdr, opts->rate_mult, opts->rate_mult_row);
        HIPCHK(hipGetLastError());
        dm.g_par = reinterpret_cast<const double*>(reinterpret_cast<size_t>(dm.g_par) | 1u);
    }
    if (energy) o.dq_jac = 1;   // CVODE's DQ Jacobian, in either engine
    // the engine (traced and programme runs: the wavefront engine) and the instance family
    const int engine = energy ? pick_energy_engine(m) : (trace || prog) ? 0 : pick_engine(m);
    const Flavour fl = energy ? ENERGY : prog ? PROGRAMME : ISOTHERMAL;
    if (engine < 0 && energy) {
        KOptsEnergy oe = energy_kopts(o, opts);
        return launch_group(m, m->grp_e, grp_energy_kernel(m->grp_e.gl, m->grp_e.nm), dm, N, dT, dAsv, du, dtf, &oe, dstats, s);
    }
    if (engine < 0) return launch_group(m, m->grp, grp_kernel(m->grp.gl, m->grp.nm), dm, N, dT, dAsv, du, dtf, &o, dstats, s);
    if (engine > 0) {
        // one reactor per lane; reactors still running after defer_steps steps (a few per 1e4 on
        // H2/O2, some of them up to max_steps) are handed to a follow-up wavefront pass, whose
        // per-step latency for a lone reactor is far lower than a wave's with one live lane
        const int NM = m->lane.nm;
        const int blocks = std::max(1, std::min((N + 63) / 64, m->lane.wg_per_cu * m->ncu));
        const size_t need = (size_t)lane_lay(NM, m->n, m->dm.nset, m->nrg, m->dm.nfo).g_rows * blocks * 64 * sizeof(double);
        if (need >= 0x7fffffffull) return fail(BR_ERR_UNSUPPORTED, "lane workspace exceeds the 2 GB buffer range");
        HIPCHK(m->lws.ensure(need));
        const char* ds = getenv("BRHIP_DEFER_STEPS");
        o.defer_steps = ds ? atoi(ds) : 5000;
        if (o.defer_steps <= 0 || o.defer_steps >= o.max_steps) o.defer_steps = o.max_steps;
        const int cap = std::min(N, DEFER_CAP);
        HIPCHK(m->jws.ensure(jws_bytes(m, cap)));
        HIPCHK(m->queue.ensure((2 + DEFER_CAP) * sizeof(int)));
        HIPCHK(m->defer_t0.ensure(DEFER_CAP * sizeof(double)));
        HIPCHK(hipMemsetAsync(m->queue.p, 0, 2 * sizeof(int), s));
        HIPCHK(hipEventRecord(m->ev0, s));
        const void* lfn = lane_kernel(NM);
        HIPCHK(hipFuncSetAttribute(lfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)m->lane.shmem));
        double* lws = m->lws.as<double>();
        int* queue = m->queue.as<int>();
        double* defer_t0 = m->defer_t0.as<double>();
        void* args[] = {(void*)&dm, (void*)&N, (void*)&dT, (void*)&du, (void*)&dtf, (void*)&o, (void*)&dstats, (void*)&lws,
                        (void*)&queue, (void*)&defer_t0, (void*)&cap};
        HIPCHK(hipLaunchKernel(lfn, dim3(blocks), dim3(64), args, m->lane.shmem, s));
        if (o.defer_steps < o.max_steps) {   // the deferred reactors continue on the wavefront engine
            KOpts o2 = o;
            o2.defer_steps = o.max_steps;
            o2.rid_list = queue + 2;
            o2.rid_count = queue + 1;
            o2.rid_t0 = defer_t0;
            const int nwg = (cap + m->wave.rpb - 1) / m->wave.rpb;
            if (const int rc = launch_wave(m, ISOTHERMAL, m->wave, dm, cap, nwg, dT, dAsv, du, dtf, o2, nullptr, dstats, nullptr, s))
                return rc;
        }
        HIPCHK(hipEventRecord(m->ev1, s));
        m->ev_recorded = true;
        return 0;
    }
    return launch_wave_grid(m, fl, energy ? m->wave_e : m->wave, dm, N, dT, dAsv, du, dtf, o, opts, dstats, trace, s);
}

int br_integrate_dev(br_mech* m, int N, const double* dT, const double* dAsv, double* du, const double* dtf,
                     const br_opts* opts, br_stats* dstats, void* stream) {
    return integrate_dev(m, N, dT, dAsv, du, dtf, opts, dstats, stream, nullptr);
}

int br_last_kernel_ms(br_mech* m, double* ms) {
    if (!m || !ms || !m->ev_recorded) return fail(BR_ERR_INPUT, "no kernel recorded");
    HIPCHK(hipEventSynchronize(m->ev1));
    float f = 0.f;
    HIPCHK(hipEventElapsedTime(&f, m->ev0, m->ev1));
    *ms = (double)f;
    return 0;
}

// per-reactor output grids (br_opts.tout_per_reactor, host array tout[N][nout]): every row ascending,
// NaN (no output) only as trailing padding; the message names the first bad reactor
static int check_tout_rows(int N, int nout, const double* tout) {
    for (int i = 0; i < N; ++i) {
        const double* r = tout + (size_t)i * nout;
        for (int j = 1; j < nout; ++j) {
            if (r[j] != r[j]) continue;                     // padding, if nothing but NaN follows
            if (r[j - 1] != r[j - 1])
                return fail(BR_ERR_INPUT, "tout of reactor " + std::to_string(i) + ": NaN before a time (entry " +
                                              std::to_string(j - 1) + "); NaN is trailing padding only");
            if (!(r[j] >= r[j - 1]))
                return fail(BR_ERR_INPUT, "tout of reactor " + std::to_string(i) + " must be ascending (entry " +
                                              std::to_string(j) + ")");
        }
    }
    return 0;
}

static int integrate_host(br_mech* m, int N, const double* T, const double* Asv, double* u, const double* tf,
                          const br_opts* opts, br_stats* stats, double* trace) {
    // (the programme first: its checks need no handle, and with one the T argument may be NULL)
    if (const int rc = energy_request(opts)) return rc;
    if (N >= 0) { if (const int rc = check_tprog_host(N, opts)) return rc; }
    const bool prog = opts && opts->ntprog != 0;
    const bool energy = opts && opts->energy != 0;
    if (!m || N < 0 || (!T && !prog) || !u || !tf) return fail(BR_ERR_INPUT, "bad argument");
    if (energy && trace)
        return fail(BR_ERR_UNSUPPORTED, "br_integrate_traced does not take br_opts.energy: the trace row has no T column");
    if (N == 0) return 0;
    HIPCHK(hipSetDevice(m->device));
    const int n = m->n;
    const int cap = (trace && opts) ? opts->trace_cap : 0;
    if (trace && cap <= 0) return fail(BR_ERR_INPUT, "trace_cap must be > 0");
    const size_t ntr = trace ? (size_t)N * (cap + 1) * (2 * n + 4) : 0;
    const OutReq rq = out_request(opts);
    const int nout = rq.nout;
    const bool per = rq.per;                                // tout[N][nout], one row per reactor
    const size_t nyo = (size_t)N * nout * n;
    const size_t nto = per ? (size_t)N * nout : (size_t)nout;
    if (per) {
        int rc = check_tout_rows(N, nout, opts->tout);
        if (rc) return rc;
    }
    for (int i = 1; i < nout && !per; ++i)
        if (!(opts->tout[i] >= opts->tout[i - 1])) return fail(BR_ERR_INPUT, "tout must be ascending");
    if (const int rc = check_mult_host(m, N, opts)) return rc;
    Stage st;
    // an energy run's T outputs: T_end[N], T_out[N][nout] (staged with the caller's values: entries without an
    // output keep them, as the rows of yout)
    const size_t nTe = (energy && opts->T_end) ? (size_t)N : 0, nTo = (energy && opts->T_out) ? (size_t)N * nout : 0;
    HIPCHK(st.reserve(m, (size_t)N * (3 + n + BR_NSTAT) + ntr + nto + nyo + mult_stage_doubles(m, N, opts) +
                             tprog_stage_doubles(N, opts) + nTe + nTo));
    double* dT = st.take(N);
    double* dA = st.take(N);
    double* dtf = st.take(N);
    double* du_ = st.take((size_t)N * n);
    double* dst = st.take((size_t)N * BR_NSTAT);
    double* dtr = st.take(ntr);
    br_opts od;
    if (opts) od = *opts;
    double* dyo = nullptr;
    if (nout) {
        od.tout = st.push(opts->tout, nto);
        od.yout = dyo = st.push(opts->yout, nyo);
    }
    stage_mult(st, m, N, opts, &od);
    stage_tprog(st, N, opts, &od);
    if (energy) {
        od.T_end = nTe ? st.take(nTe) : nullptr;
        od.T_out = nTo ? st.push(opts->T_out, nTo) : nullptr;
    }
    st.put(dT, T, N);
    st.put(dA, Asv, N);
    st.put(dtf, tf, N);
    st.put(du_, u, (size_t)N * n);
    HIPCHK(st.err);
    if (trace) HIPCHK(hipMemset(dtr, 0, ntr * sizeof(double)));
    const int rc = integrate_dev(m, N, dT, Asv ? dA : nullptr, du_, dtf, opts ? &od : nullptr, (br_stats*)dst, nullptr,
                                 trace ? dtr : nullptr);
    if (rc) return rc;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(u, du_, (size_t)N * n * sizeof(double), hipMemcpyDeviceToHost));
    if (stats) HIPCHK(hipMemcpy(stats, dst, (size_t)N * BR_NSTAT * sizeof(double), hipMemcpyDeviceToHost));
    if (trace) HIPCHK(hipMemcpy(trace, dtr, ntr * sizeof(double), hipMemcpyDeviceToHost));
    if (nout) HIPCHK(hipMemcpy(opts->yout, dyo, nyo * sizeof(double), hipMemcpyDeviceToHost));
    if (nTe) HIPCHK(hipMemcpy(opts->T_end, od.T_end, nTe * sizeof(double), hipMemcpyDeviceToHost));
    if (nTo) HIPCHK(hipMemcpy(opts->T_out, od.T_out, nTo * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

int br_integrate(br_mech* m, int N, const double* T, const double* Asv, double* u, const double* tf,
                 const br_opts* opts, br_stats* stats) {
    return integrate_host(m, N, T, Asv, u, tf, opts, stats, nullptr);
}

int br_integrate_traced(br_mech* m, int N, const double* T, const double* Asv, double* u, const double* tf,
                        const br_opts* opts, br_stats* stats, double* trace) {
    return integrate_host(m, N, T, Asv, u, tf, opts, stats, trace);
}

int br_integrate_multi(br_mech* const* mechs, int ndev, int N, const double* T, const double* Asv, double* u,
                       const double* tf, const br_opts* opts, br_stats* stats) {
    if (const int rc0 = energy_request(opts)) return rc0;
    if (N >= 0) { if (const int rc0 = check_tprog_host(N, opts)) return rc0; }   // (indices of the ensemble in the message)
    const bool prog = opts && opts->ntprog != 0;
    if (!mechs || ndev < 1 || N < 0 || (!T && !prog) || !u || !tf) return fail(BR_ERR_INPUT, "bad argument");
    for (int d = 0; d < ndev; ++d) {
        if (!mechs[d] || mechs[d]->n != mechs[0]->n) return fail(BR_ERR_INPUT, "handles differ in size");
        for (int e = 0; e < d; ++e)
            if (mechs[e] == mechs[d]) return fail(BR_ERR_INPUT, "one handle per shard (handles hold workspaces)");
    }
    const int n = mechs[0]->n;
    const int nout = out_request(opts).nout;
    const bool per = out_request(opts).per;
    if (per) {   // (here, so that the message names the reactor's index in the ensemble, not in its slice)
        int rc0 = check_tout_rows(N, nout, opts->tout);
        if (rc0) return rc0;
    }
    // (the multipliers too: indices of the ensemble in the message; the slices are checked again, cheaply)
    if (const int rc0 = check_mult_host(mechs[0], N, opts)) return rc0;
    const int nr = mechs[0]->nrg + mechs[0]->nrs;
    std::vector<int> rc(ndev, 0);
    std::vector<std::string> msg(ndev);
    std::vector<std::thread> th;
    const int base = N / ndev, extra = N % ndev;
    for (int d = 0; d < ndev; ++d) {
        const int start = d * base + std::min(d, extra), cnt = base + (d < extra ? 1 : 0);
        th.emplace_back([&, d, start, cnt]() {
            br_opts od{};
            if (opts) od = *opts;
            if (nout) od.yout = opts->yout + (size_t)start * nout * n;
            if (per) od.tout = opts->tout + (size_t)start * nout;
            if (opts && opts->energy) {   // the slice's T outputs
                if (opts->T_end) od.T_end = opts->T_end + start;
                if (opts->T_out) od.T_out = opts->T_out + (size_t)start * nout;
            }
            if (opts && opts->nmult > 0) {   // the slice's row indices, or its rows of the dense table
                if (opts->rate_mult_row) od.rate_mult_row = opts->rate_mult_row + start;
                else { od.rate_mult = opts->rate_mult + (size_t)start * nr; od.nmult = cnt; }
            }
            if (prog) {   // likewise the programmes: the slice's row indices, or its rows
                if (opts->tprog_row) od.tprog_row = opts->tprog_row + start;
                else {
                    od.tprog_t = opts->tprog_t + (size_t)start * opts->ntprog;
                    od.tprog_T = opts->tprog_T + (size_t)start * opts->ntprog;
                    od.ntprog_rows = cnt;
                }
            }
            rc[d] = integrate_host(mechs[d], cnt, T ? T + start : nullptr, Asv ? Asv + start : nullptr, u + (size_t)start * n,
                                   tf + start, opts ? &od : nullptr, stats ? stats + start : nullptr, nullptr);
            if (rc[d]) msg[d] = g_err;
        });
    }
    for (auto& t : th) t.join();
    for (int d = 0; d < ndev; ++d)
        if (rc[d]) return fail(rc[d], "shard " + std::to_string(d) + ": " + msg[d]);
    return 0;
}

int br_phase_tout_dev(int N, br_stats* dstats, int ntau, const double* dtau, const double* dtf, double* dtout,
                      void* stream) {
    if (N < 0 || ntau < 1 || !dstats || !dtau || !dtf || !dtout) return fail(BR_ERR_INPUT, "bad argument");
    if (N == 0) return 0;
    const size_t ne = (size_t)N * ntau;
    hipLaunchKernelGGL(k_phase_tout, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, (hipStream_t)stream, N,
                       (const br_stats*)dstats, ntau, dtau, dtf, dtout);
    HIPCHK(hipGetLastError());
    return 0;
}

int br_integrate_phase(br_mech* m, int N, const double* T, const double* Asv, double* u, const double* tf,
                       const br_opts* opts, br_stats* stats, int ntau, const double* tau, double* tout, double* yout) {
    if (const int rce = energy_request(opts)) return rce;
    if (N >= 0) { if (const int rcp = check_tprog_host(N, opts)) return rcp; }
    const bool prog = opts && opts->ntprog != 0;
    if (!m || N < 0 || (!T && !prog) || !u || !tf || !tau || !tout || !yout || ntau < 1) return fail(BR_ERR_INPUT, "bad argument");
    if (!opts || opts->ignition_species < 1 || opts->ignition_species > m->ng)
        return fail(BR_ERR_INPUT, "br_integrate_phase needs br_opts.ignition_species (the phases are multiples of t_ign)");
    for (int j = 0; j < ntau; ++j)
        if (!(tau[j] > 0.0) || !(tau[j] < INFINITY) || (j && !(tau[j] >= tau[j - 1])))
            return fail(BR_ERR_INPUT, "tau must be positive, finite and ascending");
    if (N == 0) return 0;
    HIPCHK(hipSetDevice(m->device));
    const int n = m->n;
    const size_t nu = (size_t)N * n, nto = (size_t)N * ntau, nyo = nto * n;
    if (const int rcm = check_mult_host(m, N, opts)) return rcm;
    Stage st;
    // an energy run: both passes run with it; opts->T_end [N] and opts->T_out [N][ntau] (T at the phases; entries
    // of NaN times are left untouched) are pass 2's
    const size_t nTe = (opts->energy && opts->T_end) ? (size_t)N : 0, nTo = (opts->energy && opts->T_out) ? nto : 0;
    HIPCHK(st.reserve(m, (size_t)N * (3 + BR_NSTAT) + 2 * nu + ntau + nto + nyo + mult_stage_doubles(m, N, opts) +
                             tprog_stage_doubles(N, opts) + nTe + nTo));
    double* dT = st.push(T, N);
    double* dA = st.push(Asv, N);
    double* dtf = st.push(tf, N);
    double* du_ = st.take(nu);
    double* du0 = st.push(u, nu);
    double* dst = st.take((size_t)N * BR_NSTAT);
    double* dtau = st.push(tau, ntau);
    double* dto = st.take(nto);
    double* dyo = st.push(yout, nyo);   // (rows without an output keep their values)
    br_opts od = *opts;
    stage_mult(st, m, N, opts, &od);   // (both passes run with the same multipliers)
    stage_tprog(st, N, opts, &od);     // (... and the same programmes)
    double* dTe = nTe ? st.take(nTe) : nullptr;
    double* dTo = nTo ? st.push(opts->T_out, nTo) : nullptr;
    HIPCHK(st.err);
    od.trace_cap = 0;
    // pass 1: no outputs, for t_ign
    od.nout = 0; od.tout = nullptr; od.yout = nullptr; od.tout_per_reactor = 0;
    od.T_end = nullptr; od.T_out = nullptr;
    HIPCHK(hipMemcpyAsync(du_, du0, nu * sizeof(double), hipMemcpyDeviceToDevice, nullptr));
    int rc = integrate_dev(m, N, dT, Asv ? dA : nullptr, du_, dtf, &od, (br_stats*)dst, nullptr, nullptr);
    if (rc) return rc;
    rc = br_phase_tout_dev(N, (br_stats*)dst, ntau, dtau, dtf, dto, nullptr);
    if (rc) return rc;
    // pass 2: the same u0 and options (the same steps) with the per-reactor grid
    od.nout = ntau; od.tout = dto; od.yout = dyo; od.tout_per_reactor = 1;
    od.T_end = dTe; od.T_out = dTo;
    HIPCHK(hipMemcpyAsync(du_, du0, nu * sizeof(double), hipMemcpyDeviceToDevice, nullptr));
    rc = integrate_dev(m, N, dT, Asv ? dA : nullptr, du_, dtf, &od, (br_stats*)dst, nullptr, nullptr);
    if (rc) return rc;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(u, du_, nu * sizeof(double), hipMemcpyDeviceToHost));
    if (stats) HIPCHK(hipMemcpy(stats, dst, (size_t)N * BR_NSTAT * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(tout, dto, nto * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(yout, dyo, nyo * sizeof(double), hipMemcpyDeviceToHost));
    if (nTe) HIPCHK(hipMemcpy(opts->T_end, dTe, nTe * sizeof(double), hipMemcpyDeviceToHost));
    if (nTo) HIPCHK(hipMemcpy(opts->T_out, dTo, nTo * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

// br_sensitivity: one multiplier table of 2 nsel + 1 rows (built here once; 1.7 MB for every reaction of
// GRI-Mech, so it stays L2-resident), and per chunk of base reactors: k_sens_expand, one br_integrate_dev over the
// expanded reactors, k_sens_reduce / k_sens_base, and the copy of S and the base results to the host.
constexpr size_t SENS_BUDGET_BYTES = (size_t)1 << 30;   // expanded inputs, states and stats of one chunk
int br_sensitivity(br_mech* m, int N, const double* T, const double* Asv, const double* u0, const double* tf,
                   const br_opts* opts, double factor, int nsel, const int* rxn, double* S_tign, double* S_u, double* u,
                   br_stats* stats, long long* nbad) {
    if (opts && opts->ntprog != 0)   // (before anything else: no handle, no device needed to learn it)
        return fail(BR_ERR_UNSUPPORTED, "br_sensitivity does not take a temperature programme (br_opts.ntprog)");
    if (const int rce = energy_request(opts)) return rce;
    if (!m || N < 0 || !T || !u0 || !tf) return fail(BR_ERR_INPUT, "bad argument");
    if (!(factor > 1.0) || !(factor < INFINITY)) return fail(BR_ERR_INPUT, "factor must be finite and > 1");
    if (opts && (opts->nmult != 0 || opts->rate_mult))
        return fail(BR_ERR_INPUT, "br_sensitivity builds its own multiplier table: opts->rate_mult must be unset");
    if (S_tign && (!opts || opts->ignition_species < 1 || opts->ignition_species > m->ng))
        return fail(BR_ERR_INPUT, "S_tign needs br_opts.ignition_species");
    const int n = m->n, nr = m->nrg + m->nrs;
    if (!rxn) nsel = nr;
    if (nsel < 1) return fail(BR_ERR_INPUT, "no reactions selected");
    for (int j = 0; j < nsel && rxn; ++j)
        if (rxn[j] < 0 || rxn[j] >= nr)
            return fail(BR_ERR_INPUT, "rxn[" + std::to_string(j) + "] = " + std::to_string(rxn[j]) + " is outside [0, " +
                                          std::to_string(nr) + ")");
    if (nbad) *nbad = 0;
    if (N == 0) return 0;
    HIPCHK(hipSetDevice(m->device));
    const int rows = 2 * nsel + 1;
    std::vector<double> table((size_t)rows * nr, 1.0);
    for (int j = 0; j < nsel; ++j) {
        const int r = rxn ? rxn[j] : j;
        table[(size_t)(1 + 2 * j) * nr + r] = factor;
        table[(size_t)(2 + 2 * j) * nr + r] = 1.0 / factor;
    }
    // doubles per base reactor: its inputs, its expanded reactors (T, Asv, tf, row index, state, stats), S,
    // base state and stats
    const size_t per_base = (size_t)(3 + n) + (size_t)rows * (4 + n + BR_NSTAT) + (size_t)nsel * (1 + n) + n + BR_NSTAT;
    long long chunk = (long long)std::max<size_t>(1, SENS_BUDGET_BYTES / (per_base * sizeof(double)));
    if (const char* ce = getenv("BRHIP_SENS_CHUNK")) { if (atoll(ce) > 0) chunk = atoll(ce); }
    chunk = std::min<long long>(std::min<long long>(chunk, N), 0x7fffffffLL / rows);
    const int B0 = (int)chunk;
    const size_t NE0 = (size_t)B0 * rows;
    Stage st;
    HIPCHK(st.reserve(m, table.size() + 1 + B0 * per_base));
    const double* dtab = st.push(table.data(), table.size());
    unsigned long long* dbad = (unsigned long long*)st.take(1);
    double* dT = st.take(B0); double* dA = st.take(B0); double* dtf = st.take(B0); double* du0 = st.take((size_t)B0 * n);
    double* eT = st.take(NE0); double* eA = st.take(NE0); double* etf = st.take(NE0);
    int* erow = (int*)st.take(NE0);
    double* eU = st.take(NE0 * n);
    br_stats* est = (br_stats*)st.take(NE0 * BR_NSTAT);
    double* dSt = st.take((size_t)B0 * nsel); double* dSu = st.take((size_t)B0 * nsel * n);
    double* dbu = st.take((size_t)B0 * n);
    br_stats* dbst = (br_stats*)st.take((size_t)B0 * BR_NSTAT);
    HIPCHK(st.err);
    HIPCHK(hipMemset(dbad, 0, sizeof(unsigned long long)));
    br_opts od{};
    if (opts) od = *opts;
    od.trace_cap = 0; od.nout = 0; od.tout = nullptr; od.yout = nullptr; od.tout_per_reactor = 0;
    od.nmult = rows; od.rate_mult = dtab; od.rate_mult_row = erow;
    od.T_end = nullptr; od.T_out = nullptr;   // (an energy run's expanded reactors: no T outputs)
    const double den = 2.0 * std::log(factor);
    auto blocks = [](size_t ne) { return dim3((unsigned)((ne + 255) / 256)); };
    for (int i0 = 0; i0 < N; i0 += B0) {
        const int B = std::min(B0, N - i0);
        const size_t NE = (size_t)B * rows;
        st.put(dT, T + i0, B); st.put(dA, Asv ? Asv + i0 : nullptr, B); st.put(dtf, tf + i0, B);
        st.put(du0, u0 + (size_t)i0 * n, (size_t)B * n);
        HIPCHK(st.err);
        hipLaunchKernelGGL(k_sens_expand, blocks(NE * n), dim3(256), 0, nullptr, B, rows, n, (const double*)dT,
                           (const double*)(Asv ? dA : nullptr), (const double*)du0, (const double*)dtf, eT, eA, eU, etf, erow);
        HIPCHK(hipGetLastError());
        const int rc = integrate_dev(m, (int)NE, eT, Asv ? eA : nullptr, eU, etf, &od, est, nullptr, nullptr);
        if (rc) return rc;
        const int nk = S_u ? n : 1;
        if (S_tign || S_u) {
            hipLaunchKernelGGL(k_sens_reduce, blocks((size_t)B * nsel * nk), dim3(256), 0, nullptr, B, nsel, rows, n, nk, den,
                               (const double*)eU, (const br_stats*)est, S_tign ? dSt : nullptr, S_u ? dSu : nullptr, dbad);
            HIPCHK(hipGetLastError());
        }
        hipLaunchKernelGGL(k_sens_base, blocks((size_t)B * (n + BR_NSTAT)), dim3(256), 0, nullptr, B, rows, n,
                           (const double*)eU, (const br_stats*)est, dbu, dbst);
        HIPCHK(hipGetLastError());
        HIPCHK(hipDeviceSynchronize());
        if (S_tign) HIPCHK(hipMemcpy(S_tign + (size_t)i0 * nsel, dSt, (size_t)B * nsel * sizeof(double), hipMemcpyDeviceToHost));
        if (S_u) HIPCHK(hipMemcpy(S_u + (size_t)i0 * nsel * n, dSu, (size_t)B * nsel * n * sizeof(double), hipMemcpyDeviceToHost));
        if (u) HIPCHK(hipMemcpy(u + (size_t)i0 * n, dbu, (size_t)B * n * sizeof(double), hipMemcpyDeviceToHost));
        if (stats) HIPCHK(hipMemcpy(stats + i0, dbst, (size_t)B * BR_NSTAT * sizeof(double), hipMemcpyDeviceToHost));
    }
    if (nbad) {
        unsigned long long nb = 0;
        HIPCHK(hipMemcpy(&nb, dbad, sizeof nb, hipMemcpyDeviceToHost));
        *nbad = (long long)nb;
    }
    return 0;
}

}  // extern "C"

#include "brhip_debug.hpp"   // test and diagnostic kernels and entry points
