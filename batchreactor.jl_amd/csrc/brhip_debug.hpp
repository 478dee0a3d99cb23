// brhip_debug.hpp -- test and diagnostic kernels (k_lu_check*, k_group_eval, k_group_lu) and their
// extern "C" entry points (br_debug_*, br_diag_sub). Included at the end of brhip.hip: they use its
// error helpers and br_mech.
// ------------------------------------------------------------------------------------
// dense-solver check: factor (I - gamma*J) with the row-per-lane LU of the integrator and
// solve one right-hand side per matrix. J[N][n][n] row-major, b/x [N][n].
// ------------------------------------------------------------------------------------
namespace {
template <int NMAX>
__global__ __launch_bounds__(64) void k_lu_check(int N, int n, const double* J, const double* g, const double* b,
                                                 double* x, double* ws, int* fail) {
    const int rid = blockIdx.x;
    if (rid >= N) return;
    const int lane = threadIdx.x;
    __shared__ double prow[256];
    double* Jt = ws + (size_t)rid * (NMAX * WAVE + lu_ws_doubles(NMAX));
    double* LU = Jt + NMAX * WAVE;
    for (int j = 0; j < NMAX; ++j) Jt[j * WAVE + lane] = (lane < n && j < n) ? J[((size_t)rid * n + lane) * n + j] : 0.0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    // twice, as in the integrator: the first factorization loads the rows in natural order (pivot
    // search + gather path), the second in the first one's pivot order (every pivot on its own lane:
    // the factors come out in step order, no gather); the solve uses the second one's factors
    int perm = lane;
    auto factor = [&]() __attribute__((always_inline)) { return lu_factor<NMAX>(Jt, LU, g[rid], n, lane, perm); };
    int f = factor();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    f = factor();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    const double r = lu_solve<NMAX>(LU, n, lane, perm, lane < n ? b[(size_t)rid * n + lane] : 0.0, (LDSd*)prow);
    if (lane < n) x[(size_t)rid * n + lane] = r;
    if (lane == 0) fail[rid] = f;
}
template <int NMAX>
__global__ __launch_bounds__(64) void k_lu_check2(int N, int n, const double* J, const double* g, const double* b,
                                                  double* x, double* ws, int* fail) {
    constexpr int JW = CR2;
    __shared__ double scr[256];
    const int rid = blockIdx.x;
    if (rid >= N) return;
    const int lane = threadIdx.x;
    double* Jt = ws + (size_t)rid * (NMAX * JW + lu_ws_doubles(NMAX));
    double* LU = Jt + NMAX * JW;
    for (int j = 0; j < NMAX; ++j)
        for (int s = 0; s < 2; ++s) {
            const int row = lane + 64 * s;
            if (row < JW) Jt[j * JW + row] = (row < n && j < n) ? J[((size_t)rid * n + row) * n + j] : 0.0;
        }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    // twice, as k_lu_check: natural order first (gather path), then the first one's pivot order
    // (the no-gather path when every pivot stays on its position); the solve uses the second
    int perm[2] = {lane, lane + 64};
    int f = lu_factor2<NMAX>(Jt, LU, (LDSd*)scr, g[rid], n, lane, perm);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    f = lu_factor2<NMAX>(Jt, LU, (LDSd*)scr, g[rid], n, lane, perm);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    double r[2];
    for (int s = 0; s < 2; ++s) r[s] = (lane + 64 * s < n) ? b[(size_t)rid * n + lane + 64 * s] : 0.0;
    lu_solve2<NMAX>(LU, (LDSd*)scr, n, lane, perm, r);
    for (int s = 0; s < 2; ++s) if (lane + 64 * s < n) x[(size_t)rid * n + lane + 64 * s] = r[s];
    if (lane == 0) fail[rid] = f;
}
}  // namespace

// device buffers of the diagnostic entry points below, freed on every exit path (HIPCHK returns early)
namespace {
struct DevScratch {
    std::vector<void*> p;
    ~DevScratch() {
        for (void* q : p) hipFree(q);
    }
    template <class T>
    hipError_t alloc(T** out, size_t bytes) {
        void* q = nullptr;
        const hipError_t e = hipMalloc(&q, bytes);
        if (e == hipSuccess) { p.push_back(q); *out = (T*)q; }
        return e;
    }
};
}  // namespace

extern "C" int br_debug_lu_solve(int N, int n, const double* J, const double* gamma, const double* b, double* x,
                                 int* fail_out) {
    if (N <= 0 || n <= 0 || n > 72) return fail_code_input();
    const int nmax = nmax_of(n);
    double *dJ, *dg, *db, *dx, *dws;
    int* df;
    DevScratch S;
    HIPCHK(S.alloc(&dJ, (size_t)N * n * n * 8));
    HIPCHK(S.alloc(&dg, (size_t)N * 8));
    HIPCHK(S.alloc(&db, (size_t)N * n * 8));
    HIPCHK(S.alloc(&dx, (size_t)N * n * 8));
    HIPCHK(S.alloc(&dws, (size_t)N * (nmax * col_rows(nmax) + lu_ws_doubles(nmax)) * 8));
    HIPCHK(S.alloc(&df, (size_t)N * 4));
    HIPCHK(hipMemcpy(dJ, J, (size_t)N * n * n * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dg, gamma, (size_t)N * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(db, b, (size_t)N * n * 8, hipMemcpyHostToDevice));
    const void* fn = nmax == 16 ? (const void*)k_lu_check<16> : nmax == 32 ? (const void*)k_lu_check<32>
                   : nmax == 56 ? (const void*)k_lu_check<56> : nmax == 64 ? (const void*)k_lu_check<64>
                                                                            : (const void*)k_lu_check2<72>;
    void* args[] = {(void*)&N, (void*)&n, (void*)&dJ, (void*)&dg, (void*)&db, (void*)&dx, (void*)&dws, (void*)&df};
    HIPCHK(hipLaunchKernel(fn, dim3(N), dim3(64), args, 0, 0));
    HIPCHK(hipMemcpy(x, dx, (size_t)N * n * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(fail_out, df, (size_t)N * 4, hipMemcpyDeviceToHost));
    return 0;
}

// ------------------------------------------------------------------------------------
// group-engine checks (tests): the device functions of k_group (brhip_group.hpp) on their own, with
// k_group's workgroup shape, LDS blocks, global slots and buffer-resource Jacobian stores
// ------------------------------------------------------------------------------------
namespace {
// RHS and analytic Jacobian of reactors slot, slot + G, slot + 2G, ... (G = groups of the grid), one
// after another in the group's LDS block and global slot, so kd, fod and the species block are reused
// with another T as in the integrator's next reactor
template <int GL, int NM>
__global__ __launch_bounds__(64 * BR_QWPB) __attribute__((amdgpu_waves_per_eu(GL == 16 ? BR_QWPE : BR_QWPE32))) void k_group_eval(
    DevMech M, int N, const double* __restrict__ Tv, const double* __restrict__ Asvv, const double* __restrict__ U,
    double* __restrict__ DU, double* __restrict__ Jout, double* __restrict__ Jws) {
    GRP_CONTEXT(M, Jws);
    const int G = (int)gridDim.x * (BR_QWPB * GPW);
    for (int rid = slot;; rid += G) {
        if (__ballot(rid < N) == 0) break;
        if (rid < N) {                                                  // (idle groups wait, as k_group's)
            const double T = Tv[rid];
            const double Asv = Asvv ? Asvv[rid] : 1.0;
            const double Asv_th = asv_fixed ? 1.0 : Asv;
            g_init_tconst<GL>(tb, sp, kd, fod, skd, T, gl);
            const bool act = gl < n;
            const double u = act ? U[(size_t)rid * n + gl] : 0.0;
            const double fv = g_rhs<GL>(tb, sp, kd, fod, skd, T, Asv, Asv_th, u, gl, p_last);
            if (act) DU[(size_t)rid * n + gl] = fv;
            g_jac_cols<GL>(tb, sp, kd, fod, skd, T, Asv, Asv_th, gl, jst);
#pragma unroll 1
            for (int j = n; j < NM; ++j) jst(j, 0.0);                   // padding columns
            double jr[NM];
#pragma unroll
            for (int j = 0; j < NM; ++j) jr[j] = jld(j);                // the slot as k_group's LU reads it
#pragma unroll
            for (int j = 0; j < NM; ++j)
                if (act && j < n) Jout[((size_t)rid * n + gl) * n + j] = jr[j];
            wave_sync();
        }
    }
}

// g_lu + g_solve of matrix i in group i mod (64 / GL) of its wave, the rows through the group's
// saved-J slot (column-major GL x GL) as k_group loads them
template <int GL, int NM>
__global__ __launch_bounds__(64 * BR_QWPB) void k_group_lu(int N, int n, const double* __restrict__ J,
                                                           const double* __restrict__ g, const double* __restrict__ b,
                                                           double* __restrict__ x, int* __restrict__ fail_out,
                                                           int* __restrict__ perm, double* __restrict__ Jws) {
    const int gl = (int)(threadIdx.x & (GL - 1));
    const int i = blockIdx.x * (BR_QWPB * (64 / GL)) + (int)(threadIdx.x / GL);
    const __amdgpu_buffer_rsrc_t jrs = __builtin_amdgcn_make_buffer_rsrc((void*)launder(Jws), (short)0, 0x7fffffff, 0x00020000);
    const unsigned jvo = (unsigned)(i * (GL * GL) + gl) * 8u;
    if (i < N) {
        const bool act = gl < n;
#pragma unroll 1
        for (int j = 0; j < NM; ++j)
            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, (act && j < n) ? J[((size_t)i * n + gl) * n + j] : 0.0),
                                                  jrs, jvo, j * (GL * 8), 0);
        double jr[NM], a[NM];
#pragma unroll
        for (int j = 0; j < NM; ++j)
            jr[j] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(jrs, jvo, j * (GL * 8), 0));
        int orig;
        double dinv;
        const int f = g_lu<GL, NM>(jr, g[i], n, gl, a, orig, dinv);
        double r = 0.0;
        if (!f) r = g_solve<GL, NM>(a, orig, dinv, n, gl, act ? b[(size_t)i * n + gl] : 0.0);
        if (act) {
            x[(size_t)i * n + gl] = r;
            perm[(size_t)i * n + gl] = orig;
        }
        if (gl == 0) fail_out[i] = f;
    }
}
}  // namespace

extern "C" int br_debug_group_eval(br_mech* m, int N, const double* T, const double* Asv, const double* u, double* du,
                                   double* J) {
    if (!m || N <= 0 || !T || !u || !du || !J) return fail(BR_ERR_INPUT, "bad argument");
    if (!m->grp_gl) return fail(BR_ERR_UNSUPPORTED, "mechanism is not eligible for a group engine");
    HIPCHK(hipSetDevice(m->device));
    const int n = m->n, GL = m->grp_gl, NM = m->grp_nm;
    const int gpb = BR_QWPB * (64 / GL);
    const int blocks = std::min(2, (N + gpb - 1) / gpb);                // small fixed grid: the groups reuse their slots
    double *dT, *dA, *du_, *ddu, *dJ, *dws;
    DevScratch S;
    HIPCHK(S.alloc(&dT, (size_t)N * 8));
    HIPCHK(S.alloc(&dA, (size_t)N * 8));
    HIPCHK(S.alloc(&du_, (size_t)N * n * 8));
    HIPCHK(S.alloc(&ddu, (size_t)N * n * 8));
    HIPCHK(S.alloc(&dJ, (size_t)N * n * n * 8));
    HIPCHK(S.alloc(&dws, (size_t)blocks * gpb * grp::slot_doubles(GL, m->nrg) * 8));
    HIPCHK(hipMemcpy(dT, T, (size_t)N * 8, hipMemcpyHostToDevice));
    if (Asv) HIPCHK(hipMemcpy(dA, Asv, (size_t)N * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(du_, u, (size_t)N * n * 8, hipMemcpyHostToDevice));
    const void* fn = grp_instance(GL, NM, [](auto g, auto w) { return (const void*)k_group_eval<g(), w()>; });
    HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)m->grp_shmem));
    const DevMech dm = m->dm;
    const double* pA = Asv ? dA : nullptr;
    void* args[] = {(void*)&dm, (void*)&N, (void*)&dT, (void*)&pA, (void*)&du_, (void*)&ddu, (void*)&dJ, (void*)&dws};
    HIPCHK(hipLaunchKernel(fn, dim3(blocks), dim3(64 * BR_QWPB), args, m->grp_shmem, 0));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(du, ddu, (size_t)N * n * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(J, dJ, (size_t)N * n * n * 8, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int br_debug_group_lu_solve(int gl, int nm, int N, int n, const double* J, const double* gamma, const double* b,
                                       double* x, int* fail_out, int* perm) {
    const void* fn = grp_instance(gl, nm, [](auto g, auto w) { return (const void*)k_group_lu<g(), w()>; });
    if (!fn || N <= 0 || n <= 0 || n > nm || !J || !gamma || !b || !x || !fail_out || !perm) return fail_code_input();
    double *dJ, *dg, *db, *dx, *dws;
    int *df, *dp;
    DevScratch S;
    HIPCHK(S.alloc(&dJ, (size_t)N * n * n * 8));
    HIPCHK(S.alloc(&dg, (size_t)N * 8));
    HIPCHK(S.alloc(&db, (size_t)N * n * 8));
    HIPCHK(S.alloc(&dx, (size_t)N * n * 8));
    HIPCHK(S.alloc(&dws, (size_t)N * gl * gl * 8));
    HIPCHK(S.alloc(&df, (size_t)N * 4));
    HIPCHK(S.alloc(&dp, (size_t)N * n * 4));
    HIPCHK(hipMemcpy(dJ, J, (size_t)N * n * n * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dg, gamma, (size_t)N * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(db, b, (size_t)N * n * 8, hipMemcpyHostToDevice));
    const int gpb = BR_QWPB * (64 / gl);
    void* args[] = {(void*)&N, (void*)&n, (void*)&dJ, (void*)&dg, (void*)&db, (void*)&dx, (void*)&df, (void*)&dp, (void*)&dws};
    HIPCHK(hipLaunchKernel(fn, dim3((N + gpb - 1) / gpb), dim3(64 * BR_QWPB), args, 0, 0));
    HIPCHK(hipMemcpy(x, dx, (size_t)N * n * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(fail_out, df, (size_t)N * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(perm, dp, (size_t)N * n * 4, hipMemcpyDeviceToHost));
    return 0;
}

// temperature-programme check: k_tprog_eval (brhip_tprog.hpp), the integrator's evaluator, on host arrays
// that pass the checks of the host entry points
extern "C" int br_debug_tprog_eval(int N, int ntprog, const double* tprog_t, const double* tprog_T, int nrows,
                                   const int* tprog_row, int nt, const double* t, double* Tout) {
    if (N <= 0 || ntprog < 1 || nt < 1 || !t || !Tout) return fail_code_input();
    if (const int rc = check_tprog_arrays(N, ntprog, tprog_t, tprog_T, nrows, tprog_row)) return rc;
    const size_t nk = (size_t)nrows * ntprog, ne = (size_t)N * nt;
    double *dkt, *dkT, *dt, *dTo;
    int* drow = nullptr;
    DevScratch S;
    HIPCHK(S.alloc(&dkt, nk * 8));
    HIPCHK(S.alloc(&dkT, nk * 8));
    HIPCHK(S.alloc(&dt, ne * 8));
    HIPCHK(S.alloc(&dTo, ne * 8));
    HIPCHK(hipMemcpy(dkt, tprog_t, nk * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dkT, tprog_T, nk * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dt, t, ne * 8, hipMemcpyHostToDevice));
    if (tprog_row) {
        HIPCHK(S.alloc(&drow, (size_t)N * 4));
        HIPCHK(hipMemcpy(drow, tprog_row, (size_t)N * 4, hipMemcpyHostToDevice));
    }
    const TProg p{dkt, dkT, drow, ntprog, 0};
    hipLaunchKernelGGL(k_tprog_eval, dim3((N + 63) / 64), dim3(64), 0, 0, N, p, nt, (const double*)dt, dTo);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(Tout, dTo, ne * 8, hipMemcpyDeviceToHost));
    return 0;
}

#if BR_PHASE_CLOCKS
// diagnostic build only (not declared in brhip.h): read and reset the 16 sub-phase clock sums
// (BR_SUB_ADD slots of brhip_device.hpp)
extern "C" int br_diag_sub(double* out16) {
    std::vector<unsigned long long> v((size_t)brhip::SUB_MAXW * 16, 0ull);
    if (hipMemcpyFromSymbol(v.data(), HIP_SYMBOL(brhip::g_sub), v.size() * 8) != hipSuccess) return -1;
    for (int i = 0; i < 16; ++i) out16[i] = 0.0;
    for (size_t w = 0; w < (size_t)brhip::SUB_MAXW; ++w)
        for (int i = 0; i < 16; ++i) out16[i] += (double)v[w * 16 + i];
    std::fill(v.begin(), v.end(), 0ull);
    if (hipMemcpyToSymbol(HIP_SYMBOL(brhip::g_sub), v.data(), v.size() * 8) != hipSuccess) return -1;
    return 0;
}
#endif
