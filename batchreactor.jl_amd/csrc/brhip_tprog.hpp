// brhip_tprog.hpp -- prescribed per-reactor temperature programmes T(t) (br_opts.ntprog): the launch's
// programme block, the kernel options of the programme instances of k_integrate, and the evaluator the
// integrator and br_debug_tprog_eval share. Included by brhip.hip inside its anonymous namespace, after
// brhip_ctl.hpp. Only the programme instances (k_integrate<NMAX, true>) and k_tprog_eval read any of it:
// the isothermal kernels take the KOpts they always took.
#pragma once

// a launch's programmes: knot times and temperatures [nrows][nk] (NaN time = trailing padding of a row),
// the row of each reactor (nullptr: row = reactor index)
struct TProg {
    const double* t;
    const double* T;
    const int* row;
    int nk, pad;
};
// kernel options of a programme run: KOpts, then the block (the isothermal instances' argument is KOpts)
struct KOptsProg : KOpts {
    TProg prog;
};

// One reactor's programme with the segment of the last evaluation. Everything here is wave-uniform in
// k_integrate (rid is scalar): the knot loads are scalar loads, the scan's branches scalar branches.
// T(t) = T_j + (t - t_j) * ((T_{j+1} - T_j) / (t_{j+1} - t_j)) on the segment t_j <= t < t_{j+1} (the
// formula of include/brhip.h, operation for operation), T of the last knot at and beyond it. The scan is
// linear from the cached segment: forwards while the next knot is at or before t, backwards after a
// rejected step took the time back. Equal knot times (a jump) are stepped over and never divided by.
struct TProgRow {
    const BR_GLOBAL double* kt;   // (global address space: global_load / scalar loads, not flat)
    const BR_GLOBAL double* kT;
    int nk, seg;
    __device__ __forceinline__ double eval(double t) {
        int j = seg;
        while (j > 0 && t < kt[j]) --j;
        while (j + 1 < nk && t >= kt[j + 1]) ++j;   // (a NaN time -- padding -- fails the comparison)
        seg = j;
        const double tj = kt[j], Tj = kT[j];
        if (j + 1 >= nk) return Tj;
        const double t1 = kt[j + 1];
        if (!(t1 == t1)) return Tj;                 // the last knot of a ragged row: held
        return Tj + (t - tj) * ((kT[j + 1] - Tj) / (t1 - tj));
    }
};
__device__ __forceinline__ TProgRow tprog_row(const TProg& p, int rid) {
    const size_t row = p.row ? (size_t)p.row[rid] : (size_t)rid;
    return TProgRow{(const BR_GLOBAL double*)p.t + row * (size_t)p.nk, (const BR_GLOBAL double*)p.T + row * (size_t)p.nk,
                    p.nk, 0};
}
// the isothermal instances' stand-in: no members, no code
struct NoTProgRow {};

// br_debug_tprog_eval: Tout[i][k] = T(t[i][k]) of reactor i, one thread per reactor, its times in order
// (each evaluation starts from the segment the one before ended in, as in the integrator)
__global__ __launch_bounds__(64) void k_tprog_eval(int N, TProg p, int nt, const double* __restrict__ t,
                                                   double* __restrict__ Tout) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= N) return;
    TProgRow r = tprog_row(p, i);
    for (int k = 0; k < nt; ++k) Tout[(size_t)i * nt + k] = r.eval(t[(size_t)i * nt + k]);
}
