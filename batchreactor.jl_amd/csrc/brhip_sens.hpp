// brhip_sens.hpp -- the small kernels around the per-reactor rate multipliers (br_opts.rate_mult) and
// br_sensitivity: the per-launch multiplier block, the expansion of N base reactors into N (2 nsel + 1)
// perturbed ones, and the reduction of their results to logarithmic sensitivities. Plain HIP, one thread
// per entry, vector stores only. Included by brhip.hip inside its anonymous namespace.
#pragma once

// the per-launch half of the MultBlock in front of the g_par table (brhip_device.hpp): written on the
// launch's stream, so that launches on one handle with different tables stay ordered
__global__ void k_mult_block(MultBlock* b, const double* mult, const int* row) {
    if (threadIdx.x == 0 && blockIdx.x == 0) { b->mult = mult; b->row = row; }
}

// Expanded reactor r = i * rows + j is base reactor i with row j of the multiplier table: j = 0 the
// unperturbed run, j = 1 + 2 s the run with reaction s of the selection times f, j = 2 + 2 s over f.
// One thread per state entry; the thread of entry 0 also writes the reactor's scalars.
__global__ __launch_bounds__(256) void k_sens_expand(int B, int rows, int n, const double* __restrict__ T,
                                                     const double* __restrict__ Asv, const double* __restrict__ u0,
                                                     const double* __restrict__ tf, double* __restrict__ eT,
                                                     double* __restrict__ eAsv, double* __restrict__ eU,
                                                     double* __restrict__ etf, int* __restrict__ erow) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)B * rows * n) return;
    const size_t r = e / n;
    const int k = (int)(e - r * n);
    const size_t i = r / rows;
    const int j = (int)(r - i * rows);
    eU[e] = u0[i * n + k];
    if (k == 0) {
        eT[r] = T[i];
        if (Asv) eAsv[r] = Asv[i];
        etf[r] = tf[i];
        erow[r] = j;
    }
}

// S_tign[i][s] = (ln t_ign(+) - ln t_ign(-)) / den, S_u[i][s][k] = (u_k(+) - u_k(-)) / den with den = 2 ln f
// from the expanded results. NaN where either perturbed run failed (status != 0), for S_tign also where
// either has no t_ign; every NaN written counts in *nbad. One thread per (i, s, k), nk = n with S_u, else 1.
__global__ __launch_bounds__(256) void k_sens_reduce(int B, int nsel, int rows, int n, int nk, double den,
                                                     const double* __restrict__ eU, const br_stats* __restrict__ est,
                                                     double* __restrict__ S_t, double* __restrict__ S_u,
                                                     unsigned long long* __restrict__ nbad) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)B * nsel * nk) return;
    const size_t p = e / nk;
    const int k = (int)(e - p * nk);
    const size_t i = p / nsel;
    const int s = (int)(p - i * nsel);
    const size_t rp = i * rows + 1 + 2 * (size_t)s, rm = rp + 1;
    const bool ok = est[rp].status == 0.0 && est[rm].status == 0.0;
    if (S_u) {
        S_u[p * n + k] = ok ? (eU[rp * n + k] - eU[rm * n + k]) / den : NAN;
        if (!ok) atomicAdd(nbad, 1ull);
    }
    if (S_t && k == 0) {
        const double tp = est[rp].t_ign, tm = est[rm].t_ign;
        const bool good = ok && tp > 0.0 && tm > 0.0;   // (a NaN fails the comparison)
        S_t[p] = good ? (log(tp) - log(tm)) / den : NAN;
        if (!good) atomicAdd(nbad, 1ull);
    }
}

// the unperturbed runs (row 0 of every base reactor) gathered for the copy back: end states and stats
__global__ __launch_bounds__(256) void k_sens_base(int B, int rows, int n, const double* __restrict__ eU,
                                                   const br_stats* __restrict__ est, double* __restrict__ bu,
                                                   br_stats* __restrict__ bst) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int w = n + BR_NSTAT;
    if (e >= (size_t)B * w) return;
    const size_t i = e / w;
    const int k = (int)(e - i * w);
    if (k < n) bu[i * n + k] = eU[i * rows * n + k];
    else reinterpret_cast<double*>(bst)[i * BR_NSTAT + (k - n)] = reinterpret_cast<const double*>(est)[i * rows * BR_NSTAT + (k - n)];
}
