// brhip_energy.hpp -- adiabatic constant-volume reactors (br_opts.energy = BR_ENERGY_ADIABATIC_V): what only the
// energy instances of k_integrate (k_integrate<NMAX, false, true>) and k_energy_eval read. Included by brhip.hip
// inside its anonymous namespace, after brhip_ctl.hpp. The isothermal and programme instances take the KOpts /
// KOptsProg they always took and see none of this.
//
// The system has ng + 1 components: u_0 .. u_{ng-1} on lanes 0 .. ng-1 of the Nordsieck and work vectors, T on
// lane ng. The chemistry keeps M.n = ng (rhs<1> masks lane ng out by itself); the controller, the DQ Jacobian,
// the LU and the solve get ng + 1 through Ctl::a_n. The instance width follows ng + 1, so its LDS block and
// launch shape are its own (energy_reactor_bytes), not those of the mechanism's isothermal instance.
// The group engines' energy instances (k_group<GL, NM, true>, brhip_group.hpp, included after this file) use
// KOptsEnergy, energy_tclamp, energy_thermo and energy_tdot<GL> with the lane within the group in place of `lane`.
#pragma once

// kernel options of an energy run: KOpts, then the two T outputs (device arrays, either may be nullptr)
struct KOptsEnergy : KOpts {
    double* T_end;   // [N]
    double* T_out;   // [N][nout]
};

// Tc of include/brhip.h: everything that depends on temperature is evaluated at the clamped value; NaN passes
__device__ __forceinline__ double energy_tclamp(double T) { return T < 200.0 ? 200.0 : (T > 6000.0 ? 6000.0 : T); }

// e_k = (h_k/RT - 1) R Tc and cv_k = (cp_k/R - 1) R of the lane's species (0 on the other lanes, so that the
// two wave sums of energy_tdot need no mask)
__device__ __forceinline__ void energy_thermo(int lane, int ng, double Tc, double& ek, double& cvk) {
    const int k = lane < ng ? lane : 0;
    const double e = (nasa_hrt(k, Tc) - 1.0) * (R_GAS * Tc), cv = (nasa_cpr(k, Tc) - 1.0) * R_GAS;
    ek = lane < ng ? e : 0.0;
    cvk = lane < ng ? cv : 0.0;
}
// dT/dt = - sum_k e_k w_k / sum_k c_k cv_k with w_k = du_k / M_k from the RHS's own du (every lane returns it)
__device__ __forceinline__ double energy_tdot(const Tab& tb, int lane, int ng, double uk, double duk, double ek, double cvk) {
    const double Mk = tb.molwt[lane];
    const bool sp = lane < ng;
    const double w = sp ? duk / Mk : 0.0, c = sp ? uk / Mk : 0.0;
    const double num = wave_sum(ek * w), den = wave_sum(c * cvk);
    return -(num / den);
}
// ... of a GW-lane group's reactor (the energy instances of k_group, brhip_group.hpp: `gl` the lane within the
// group, T on lane ng): the same quotient with group sums in place of the wave sums
template <int GW>
__device__ __forceinline__ double energy_tdot(const Tab& tb, int gl, int ng, double uk, double duk, double ek, double cvk) {
    const double Mk = tb.molwt[gl];
    const bool sp = gl < ng;
    const double w = sp ? duk / Mk : 0.0, c = sp ? uk / Mk : 0.0;
    const double num = gsum<GW>(ek * w), den = gsum<GW>(c * cvk);
    return -(num / den);
}

// LDS block of a reactor of the NMAX-wide energy instance, and of a workgroup of rpb of them
__host__ __device__ inline size_t energy_reactor_bytes(const DevMech& M, int nmax) {
    return CTL_BYTES + vec_bytes(1, vec_stride(nmax)) + (size_t)M.rblock_bytes;
}
__host__ __device__ inline size_t energy_wg_lds_bytes(const DevMech& M, int nmax, int rpb) {
    return M.img_bytes + rpb * energy_reactor_bytes(M, nmax);
}
// wave_ctx of an energy instance: the same block order, the vector width of NMAX (not of M.n)
template <int NMAX>
__device__ __forceinline__ WaveCtx energy_wave_ctx(const DevMech& M, char* smem, int rpb, double* ws) {
    WaveCtx w;
    w.wave = uni((int)(threadIdx.x >> 6));
    w.lane = threadIdx.x & 63;
    w.rid = blockIdx.x * rpb + w.wave;
    stage_tables(M, smem);
    w.tb = tab_view<1>(smem, M);
    w.rbase = smem + M.img_bytes + (size_t)w.wave * energy_reactor_bytes(M, NMAX);
    w.R = rview<1>(w.rbase + CTL_BYTES + vec_bytes(1, vec_stride(NMAX)), M,
                   launder(ws + (size_t)w.rid * ws_doubles(NMAX, M.nrg) + rxd_ws_off(NMAX, M.nrg)));
    return w;
}
