// brhip_chem.hpp -- the chemistry, stated once for the wavefront engine (brhip_device.hpp) and the group
// engines (brhip_group.hpp): what a species, a reaction or an efficiency set contributes, as a function of
// its index and plain pointers (concentrations, third-body sums, the {kf, kr} pairs, falloff constants,
// g/RT). The functions know the RX / SX record formats, MF(...) and the arithmetic. They know nothing of
// lanes, strides, LDS layouts, barriers or prefetching: the loops over reactions, the scatter targets, the
// fences and wave_sync() are the engines'. Included by brhip_device.hpp (inside namespace brhip, after
// MF, rx_rec, Tab, BR_GLOBAL and MultRow).
#pragma once

// g/RT of species k (NASA-7, lT = log T)
__device__ __forceinline__ double nasa_grt(int k, double T, double lT) {
    const double* c = MF(nasa) + 15 * k;
    const double* a = (T < c[0]) ? c + 8 : c + 1;
    const double h = a[0] + a[1] * T / 2 + a[2] * T * T / 3 + a[3] * T * T * T / 4 + a[4] * T * T * T * T / 5 + a[5] / T;
    const double s = a[0] * lT + a[1] * T + a[2] * T * T / 2 + a[3] * T * T * T / 3 + a[4] * T * T * T * T / 4 + a[6];
    return h - s;
}

// h/RT and cp/R of species k (NASA-7, the branch rule of nasa_grt); the energy instances of k_integrate
// (brhip_energy.hpp) are their only callers
__device__ __forceinline__ double nasa_hrt(int k, double T) {
    const double* c = MF(nasa) + 15 * k;
    const double* a = (T < c[0]) ? c + 8 : c + 1;
    return a[0] + a[1] * T / 2 + a[2] * T * T / 3 + a[3] * T * T * T / 4 + a[4] * T * T * T * T / 5 + a[5] / T;
}
__device__ __forceinline__ double nasa_cpr(int k, double T) {
    const double* c = MF(nasa) + 15 * k;
    const double* a = (T < c[0]) ? c + 8 : c + 1;
    return a[0] + a[1] * T + a[2] * T * T + a[3] * T * T * T + a[4] * T * T * T * T;
}

// T-only constants of gas reaction r: kd[2r] = kf, kd[2r+1] = kr = kf / Kc (grt: g/RT per species), and
// for a falloff reaction its {k0/k_inf, log10 Fcent, c, n} in fod. mr: the reactor's rate multipliers
// (MULT = false: a kernel that never sees a tagged g_par, see MultBlock)
template <bool MULT>
__device__ __forceinline__ void gas_tconst(const Tab& tb, int r, const double* grt, double T, double lT, double RT,
                                           const MultRow& mr, BR_GLOBAL double* kd, double* fod) {
    const auto rec = rx_rec(tb.rx, r);
    const uint32_t info = rec[2];
    const double* gp = (MULT ? gpar_table() : MF(g_par)) + 4 * r;
    const double kf1 = gp[0] * exp(gp[1] * lT - gp[2] / T);
    const double kf = (MULT && mr.on()) ? kf1 * mr.gas(r) : kf1;   // (kr = kf / Kc: both directions scale)
    double kr = 0.0;
    if (gi_rev(info)) {
        double dg = 0.0;
        const int nf = gi_nf(info), nr = gi_nr(info);
        for (int e = 0; e < 4; ++e) if (e < nr) dg += grt[sp8(rec[1], e)];
        for (int e = 0; e < 4; ++e) if (e < nf) dg -= grt[sp8(rec[0], e)];
        double Kc = exp(-dg) * pow(MF(p_std) / RT, (double)MF(g_dnu)[r]);
        Kc *= gp[3];
        kr = kf / Kc;
    }
    kd[2 * r] = kf;
    kd[2 * r + 1] = kr;
    if (gi_tb(info) == 2) {
        const int fi = gi_foidx(info);
        const double* fp = MF(fo_par) + 8 * fi;
        double* fo = fod + 4 * fi;
        fo[0] = fp[0] * exp(fp[1] * lT - fp[2] / T) / kf1;   // k0 / k_inf (of the unscaled pair)
        double fcv = 1.0;
        if (gi_troe(info)) {
            fcv = (1 - fp[3]) * exp(-T / fp[4]) + fp[3] * exp(-T / fp[5]);
            if (gi_troe(info) == 4) fcv += exp(-fp[6] / T);
        }
        const double lfc = log10(fcv);
        fo[1] = lfc;
        fo[2] = ((MF(conv) & BR_CONV_TROE_C4) ? -4.0 : -0.4) - 0.67 * lfc;
        fo[3] = 0.75 - 1.27 * lfc;
    }
}

// k(T) of surface reaction r (sticking or Arrhenius), times the reactor's rate multiplier
template <bool MULT>
__device__ __forceinline__ double surf_tconst(const Tab& tb, int r, double T, double RT, const MultRow& mr) {
    const uint32_t info = tb.sx[SX_WORDS * r + 4];
    const double* sp = MF(s_par) + 4 * r;
    double k;
    if (si_stick(info)) k = sp[0] * sqrt(RT / (2 * M_PI * sp[3]));
    else k = sp[0] * pow(T, sp[1]) * exp(-sp[2] / RT);
    if (MULT && mr.on()) k *= mr.surf(r);
    return k;
}

// falloff: fac = Pr/(1+Pr)*F and d fac / d[M] (CHEMKIN Lindemann / Troe); fo[0] = k0/k_inf
// (T-only, so Pr = fo[0] [M] needs no division). Troe: log10 F = log10 Fcent / (1 + f1^2) with
// f1 = x / den, evaluated as log10 Fcent den^2 / (den^2 + x^2) (one division), F = exp10(...)
// instead of the generic pow(10, .) (same value to an ulp, about half the instructions).
__device__ __forceinline__ double troe_F(double Pr, const double* fo, double& x_out, double& den_out) {
    const double Prs = Pr > 1e-300 ? Pr : 1e-300;
    const double x = log10(Prs) + fo[2];
    const double den = fo[3] - 0.14 * x;
    const double d2 = den * den;
    x_out = x; den_out = den;
    return exp10(fo[1] * d2 / (d2 + x * x));
}
template <bool WANT_D>
__device__ __forceinline__ void falloff(const double* fo, bool troe, double Mc, double& fac, double& dfac) {
    const double k0r = fo[0];
    const double Pr = k0r * Mc;
    double F = 1.0, g = 0.0;
    if (troe) {
        double x, den;
        F = troe_F(Pr, fo, x, den);
        if (WANT_D) {
            const double lfc = fo[1], nn = fo[3];
            const double f1 = x / den;
            const double df1 = nn / (den * den);
            g = -lfc * 2 * f1 / ((1 + f1 * f1) * (1 + f1 * f1)) * df1;
        }
    }
    fac = Pr / (1 + Pr) * F;
    if (WANT_D) dfac = (F / ((1 + Pr) * (1 + Pr)) + F * g / (1 + Pr)) * k0r;
}

// third-body concentration of efficiency set t: Ctot + sum (eff-1) c over the set's list (the list
// entries are read 2 at a time so the loads overlap: two partial sums, s0 + s1)
__device__ __forceinline__ double third_body_sum(const Tab& tb, int t, const double* conc, double Ctot) {
    const uint32_t w = tb.tbs[t];
    const int b = w & 0xFFFFF, e = b + (int)(w >> 20);
    double s0 = Ctot, s1 = 0.0;
    int i = b;
#pragma unroll 1
    for (; i + 1 < e; i += 2) {
        const double2 e0 = *reinterpret_cast<const double2*>(tb.tbe + 16 * i);
        const double2 e1 = *reinterpret_cast<const double2*>(tb.tbe + 16 * (i + 1));
        const int k0 = __double_as_longlong(e0.x) & 0xFFFF, k1 = __double_as_longlong(e1.x) & 0xFFFF;
        s0 = fma(e0.y, conc[k0], s0);
        s1 = fma(e1.y, conc[k1], s1);
    }
    if (i < e) {
        const double2 e0 = *reinterpret_cast<const double2*>(tb.tbe + 16 * i);
        s0 = fma(e0.y, conc[__double_as_longlong(e0.x) & 0xFFFF], s0);
    }
    return s0 + s1;
}

// mass-action part kf prod(c_f) - kr prod(c_b) of a gas reaction (w0, w1: its reactant / product words,
// k = {kf, kr}). Branch-free products: unused slots point at the pad species, conc = 1; mechanisms with
// at most 3 reactants / products per reaction (MF(nu4) == 0, GRI) skip the 4th slot
__device__ __forceinline__ double gas_mass_action(const double* conc, double2 k, uint32_t w0, uint32_t w1) {
    double Pf = (conc[sp8(w0, 0)] * conc[sp8(w0, 1)]) * conc[sp8(w0, 2)];
    double Pb = (conc[sp8(w1, 0)] * conc[sp8(w1, 1)]) * conc[sp8(w1, 2)];
    if (MF(nu4)) { Pf *= conc[sp8(w0, 3)]; Pb *= conc[sp8(w1, 3)]; }
    return k.x * Pf - k.y * Pb;
}
// net rate of progress of a gas reaction from its mass-action part D: x [M] (mc: the third-body sums) or
// x the falloff factor; tbk = gi_tb(info), the caller's; xm: the falloff form with [M] in mol/cm3
__device__ __forceinline__ double gas_third_body(double D, int tbk, uint32_t info, const double* mc, const double* fod,
                                                 bool xm) {
    if (tbk) {
        const double Mc = mc[gi_tbidx(info)];
        if (tbk == 1) D *= Mc;
        else {
            double fac, dfac;
            falloff<false>(fod + 4 * gi_foidx(info), gi_troe(info) != 0, Mc, fac, dfac);
            D *= fac;
            if (xm) D *= Mc * 1e-6;                                // [M] in mol/cm3
        }
    }
    return D;
}
// ... of gas_mass_action's D
__device__ __forceinline__ double gas_rate(const double* conc, const double* mc, const double* fod, double2 k,
                                           uint32_t w0, uint32_t w1, uint32_t info, bool xm) {
    const int tbk = gi_tb(info);
    return gas_third_body(gas_mass_action(conc, k, w0, w1), tbk, info, mc, fod, xm);
}

// q_r = pre (kf prod c_f - kr prod c_b) of a third-body or falloff reaction: pre ([M] or the falloff
// factor) and coefM = d pre / d[M]; pre = 1, coefM = 0 for an elementary reaction
__device__ __forceinline__ void gas_pre_coef(uint32_t info, const double* mc, const double* fod, bool xm, double& pre,
                                             double& coefM) {
    const int tbk = gi_tb(info);
    pre = 1.0; coefM = 0.0;
    if (tbk) {
        const double Mc = mc[gi_tbidx(info)];
        if (tbk == 1) { pre = Mc; coefM = 1.0; }
        else {
            double fac, dfac;
            falloff<true>(fod + 4 * gi_foidx(info), gi_troe(info) != 0, Mc, fac, dfac);
            pre = fac * (xm ? Mc * 1e-6 : 1.0);
            coefM = dfac * (xm ? Mc * 1e-6 : 1.0) + (xm ? fac * 1e-6 : 0.0);
        }
    }
}

// d q_r / d c_j of gas reaction r at fixed [M]: pre (kf d prod c_f / d c_j - kr d prod c_b / d c_j)
template <class P>
__device__ __forceinline__ double gas_dq_dc(const RxRec<P>& rec, int r, int j, const double* conc,
                                            const BR_GLOBAL double* kd, double pre) {
    const uint32_t info = rec[2];
    const int nf = gi_nf(info), nr = gi_nr(info);
    double d = 0.0;
#pragma unroll
    for (int e = 0; e < 4; ++e) if (e < nf && sp8(rec[0], e) == j) {
        double pr = kd[2 * r];
#pragma unroll
        for (int e2 = 0; e2 < 4; ++e2) if (e2 != e && e2 < nf) pr *= conc[sp8(rec[0], e2)];
        d += pre * pr;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) if (e < nr && sp8(rec[1], e) == j) {
        double pr = kd[2 * r + 1];
#pragma unroll
        for (int e2 = 0; e2 < 4; ++e2) if (e2 != e && e2 < nr) pr *= conc[sp8(rec[1], e2)];
        d -= pre * pr;
    }
    return d;
}

// coverage factor exp(-sum eps theta / RT) of a surface reaction with nc coverage terms (cs: their
// species word, eps: their energies)
__device__ __forceinline__ double surf_cov_factor(uint32_t cs, int nc, const double* eps, const double* conc, double RT) {
    double s = 0.0;
    for (int j = 0; j < 4; ++j) if (j < nc) s += eps[j] * conc[sp8(cs, j)];
    return exp(-s / RT);
}
// branch-free product over the up to 6 reactants of a surface reaction (pad slots: conc = 1)
__device__ __forceinline__ double surf_product(const uint32_t* rec, const double* conc) {
    return ((conc[sp8(rec[0], 0)] * conc[sp8(rec[0], 1)]) * (conc[sp8(rec[0], 2)] * conc[sp8(rec[0], 3)])) *
           (conc[sp8(rec[1], 0)] * conc[sp8(rec[1], 1)]);
}

// d q_r / d u_j of a surface reaction (rec: its SX record, info = rec[4], eps: its coverage energies,
// k = k(T) times its coverage factor): reactant partials with dc/du = 1/M (gas), 1 (sticking) or
// Gamma/sigma, and the coverage-dependent activation term -eps/RT q. ng, G: the caller's MF(ng), MF(G)
__device__ __forceinline__ double surf_dq_du(const Tab& tb, const uint32_t* rec, uint32_t info, const double* eps, int j,
                                             double k, const double* conc, double RT, int ng, double G) {
    const int nf = si_nf(info), nc = si_ncov(info);
    const bool stick = si_stick(info);
    double cv[6], dc[6];
    int sp[6];
#pragma unroll
    for (int e = 0; e < 6; ++e) {
        sp[e] = e < nf ? (e < 4 ? sp8(rec[0], e) : sp8(rec[1], e - 4)) : -1;
        cv[e] = 1.0; dc[e] = 0.0;
        if (e < nf) {
            const int s = sp[e];
            if (s < ng) { cv[e] = conc[s]; dc[e] = 1.0 / tb.molwt[s]; }
            else if (stick) { cv[e] = conc[s]; dc[e] = 1.0; }
            else { cv[e] = conc[s] * G / tb.sigma[s]; dc[e] = G / tb.sigma[s]; }
        }
    }
    double d = 0.0;
#pragma unroll
    for (int e = 0; e < 6; ++e) if (sp[e] == j) {
        double pr = k;
#pragma unroll
        for (int e2 = 0; e2 < 6; ++e2) if (e2 != e && e2 < nf) pr *= cv[e2];
        d += pr * dc[e];
    }
    if (nc) {
        double P = 1.0;
#pragma unroll
        for (int e = 0; e < 6; ++e) if (e < nf) P *= cv[e];
        const double q = k * P;
        for (int jj = 0; jj < 4; ++jj) if (jj < nc && sp8(rec[5], jj) == j) d += q * (-eps[jj] / RT);
    }
    return d;
}

// J[k][j] from the two production sums of column j (w: gas reactions, d/dc_j; sf: surface reactions,
// d/du_j): M_k w / M_j + M_k Asv sf (gas rows; no gas part in a coverage column), Asv_th sigma_k / Gamma sf
// (surface rows). Mk = molwt[k]
__device__ __forceinline__ double jac_entry(const Tab& tb, int k, int j, int ng, double G, double Mk, double w, double sf,
                                            double Asv, double Asv_th) {
    if (k < ng) return (j < ng ? Mk * w / tb.molwt[j] : 0.0) + Mk * Asv * sf;
    return Asv_th * tb.sigma[k] / G * sf;
}
