// brhip_debug.hpp -- test and diagnostic kernels (k_lu_check*, k_group_eval, k_group_lu, k_lane_eval,
// k_lane_lu, k_wave_eval, k_energy_eval, k_group_energy_eval) and their extern "C" entry points (br_debug_*, br_diag_sub). Included at the
// end of brhip.hip: they use its error helpers and br_mech.
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
// wavefront LU check (tests): lu_factor + lu_solve (lu_factor2 + lu_solve2) the way k_integrate strings them
// together: every factorization is solved with at once, the next one loads its rows in the pivot order the
// last one left, the factor area may hold anything before a factorization (in the integrator: the Jacobian
// scratch), wpb waves share a workgroup, each on its own LDS scratch and workspace slot, and a slot is
// reused by the wave's next matrix.
// ------------------------------------------------------------------------------------
namespace {
struct WaveLuArgs {
    int N, n, wpb, dirty;
    const double *J0, *J1, *g0, *g1, *b;
    const int* perm_in;
    double* x;      // [2][N][n]
    int* fail;      // [2][N]
    int* perm;      // [2][N][n]
    double* F;      // [2][N][lu_ws_doubles(NMAX)]
    double* ws;     // [slots][NMAX * col_rows(NMAX) + lu_ws_doubles(NMAX)]
};
// matrices slot, slot + G, ... (G = waves of the grid) one after another in the wave's slot. Leg A: I - g0 J0
// with the rows placed as perm_in says (identity when null); leg B: I - g1 J1 (null: leg A's) with the rows in
// leg A's pivot order. One copy of the factorization and of the solve (the leg loop stays rolled).
template <int NMAX>
__global__ __launch_bounds__(64 * br_maxrpb(NMAX)) void k_wave_lu(WaveLuArgs a) {
    constexpr int CPL = NMAX > 64 ? 2 : 1;
    constexpr int JW = NMAX > 64 ? CR2 : 64;                            // column stride of the saved J (col_rows)
    constexpr int FD = NMAX > 64 ? (NMAX + 1) * CR2 : NMAX * NMAX + WAVE;   // lu_ws_doubles(NMAX)
    constexpr int SCR = Lay<CPL>::DOUBLES - Lay<CPL>::ACCW;             // k_integrate's scr: the species block from ACCW on
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int wave = uni((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int slot = (int)blockIdx.x * a.wpb + wave;
    const int G = (int)gridDim.x * a.wpb;
    const int N = a.N, n = a.n;
    LDSd* scr = (LDSd*)(reinterpret_cast<double*>(smem_raw) + wave * SCR);
    double* Jsave = a.ws + (size_t)slot * (NMAX * JW + FD);
    double* LUsave = Jsave + NMAX * JW;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    const double pad = a.dirty ? qnan : 0.0;
    for (int rid = slot; rid < N; rid += G) {
        wave_sync();
        int perm[CPL];
#pragma unroll
        FOR_S perm[s] = (a.perm_in && CS < n) ? a.perm_in[(size_t)rid * n + CS] : CS;
        if (a.dirty)
            for (int i = lane; i < FD; i += 64) LUsave[i] = qnan;
#pragma unroll 1
        for (int leg = 0; leg < 2; ++leg) {
            const double* J = (leg && a.J1) ? a.J1 : a.J0;
            const double gam = uni((leg && a.g1) ? a.g1[rid] : a.g0[rid]);
            // the saved J as jacobian() leaves it: column-major, JW rows per column, row per lane
#pragma unroll 1
            for (int j = 0; j < NMAX; ++j)
#pragma unroll
                FOR_S if (CS < JW) Jsave[j * JW + CS] = (CS < n && j < n) ? J[((size_t)rid * n + CS) * n + j] : pad;
            wave_sync();
            int f;
            if constexpr (CPL == 1) f = lu_factor<NMAX>(Jsave, LUsave, gam, n, lane, perm[0]);
            else f = lu_factor2<NMAX>(Jsave, LUsave, scr, gam, n, lane, perm);
            wave_sync();
            const size_t o = (size_t)leg * N + rid;
            if (!f) {                                                   // (k_integrate: no solve after a zero pivot)
                double r[CPL];
#pragma unroll
                FOR_S r[s] = CS < n ? a.b[(size_t)rid * n + CS] : 0.0;
                if constexpr (CPL == 1) r[0] = lu_solve<NMAX>(LUsave, n, lane, perm[0], r[0], scr);
                else lu_solve2<NMAX>(LUsave, scr, n, lane, perm, r);
#pragma unroll
                FOR_S if (CS < n) a.x[o * n + CS] = r[s];
            }
#pragma unroll
            FOR_S if (CS < n) a.perm[o * n + CS] = perm[s];
            if (lane == 0) a.fail[o] = f;
            for (int i = lane; i < FD; i += 64) a.F[o * FD + i] = LUsave[i];
            wave_sync();
        }
    }
}
}  // namespace

extern "C" int br_debug_wave_lu(int N, int n, int wpb, int dirty, const double* J0, const double* J1, const double* gamma0,
                                const double* gamma1, const double* b, const int* perm_in, double* x, int* fail_out,
                                int* perm, double* F) {
    if (N <= 0 || n < 1 || n > 72 || !J0 || !gamma0 || !b || !x || !fail_out || !perm || !F) return fail_code_input();
    const int nmax = nmax_of(n);
    if (wpb < 1 || wpb > br_maxrpb(nmax)) return fail(BR_ERR_INPUT, "wpb: 1 .. br_maxrpb(nmax) waves per workgroup");
    if (perm_in) {
        std::vector<char> seen(n);
        for (int i = 0; i < N; ++i) {
            std::fill(seen.begin(), seen.end(), 0);
            for (int s = 0; s < n; ++s) {
                const int r = perm_in[(size_t)i * n + s];
                if (r < 0 || r >= n || seen[r]) return fail(BR_ERR_INPUT, "perm_in: not a permutation of 0..n-1");
                seen[r] = 1;
            }
        }
    }
    // small fixed grid: one workgroup up to 4 wpb matrices, else two (as br_debug_wave_eval), so that every
    // wave takes further matrices in the slot of its first from N = 2 wpb (one workgroup) or 4 wpb (two) on
    const int blocks = std::min(2, (N + 4 * wpb - 1) / (4 * wpb));
    const size_t fd = lu_ws_doubles(nmax), slot = (size_t)nmax * col_rows(nmax) + fd, nn = (size_t)N * n;
    const size_t scr = nmax > 64 ? Lay<2>::DOUBLES - Lay<2>::ACCW : Lay<1>::DOUBLES - Lay<1>::ACCW;
    double *dJ0, *dJ1 = nullptr, *dg0, *dg1 = nullptr, *db, *dx, *dF, *dws;
    int *dpi = nullptr, *df, *dp;
    DevScratch S;
    HIPCHK(S.alloc(&dJ0, nn * n * 8));
    HIPCHK(S.alloc(&dg0, (size_t)N * 8));
    HIPCHK(S.alloc(&db, nn * 8));
    HIPCHK(S.alloc(&dx, 2 * nn * 8));
    HIPCHK(S.alloc(&df, 2 * (size_t)N * 4));
    HIPCHK(S.alloc(&dp, 2 * nn * 4));
    HIPCHK(S.alloc(&dF, 2 * (size_t)N * fd * 8));
    HIPCHK(S.alloc(&dws, (size_t)blocks * wpb * slot * 8));
    HIPCHK(hipMemcpy(dJ0, J0, nn * n * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dg0, gamma0, (size_t)N * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(db, b, nn * 8, hipMemcpyHostToDevice));
    if (J1) {
        HIPCHK(S.alloc(&dJ1, nn * n * 8));
        HIPCHK(hipMemcpy(dJ1, J1, nn * n * 8, hipMemcpyHostToDevice));
    }
    if (gamma1) {
        HIPCHK(S.alloc(&dg1, (size_t)N * 8));
        HIPCHK(hipMemcpy(dg1, gamma1, (size_t)N * 8, hipMemcpyHostToDevice));
    }
    if (perm_in) {
        HIPCHK(S.alloc(&dpi, nn * 4));
        HIPCHK(hipMemcpy(dpi, perm_in, nn * 4, hipMemcpyHostToDevice));
    }
    // (x starts from the caller's values: a matrix with a zero pivot writes none)
    HIPCHK(hipMemcpy(dx, x, 2 * nn * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(dws, 0, (size_t)blocks * wpb * slot * 8));
    const WaveLuArgs a{N, n, wpb, dirty != 0, dJ0, dJ1, dg0, dg1, db, dpi, dx, df, dp, dF, dws};
    const void* fn = nmax == 16 ? (const void*)k_wave_lu<16> : nmax == 32 ? (const void*)k_wave_lu<32>
                   : nmax == 56 ? (const void*)k_wave_lu<56> : nmax == 64 ? (const void*)k_wave_lu<64>
                                                                            : (const void*)k_wave_lu<72>;
    void* args[] = {(void*)&a};
    HIPCHK(hipLaunchKernel(fn, dim3(blocks), dim3(64 * wpb), args, (size_t)wpb * scr * 8, 0));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(x, dx, 2 * nn * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(fail_out, df, 2 * (size_t)N * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(perm, dp, 2 * nn * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(F, dF, 2 * (size_t)N * fd * 8, hipMemcpyDeviceToHost));
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
    if (!m->grp.gl) return fail(BR_ERR_UNSUPPORTED, "mechanism is not eligible for a group engine");
    HIPCHK(hipSetDevice(m->device));
    const int n = m->n, GL = m->grp.gl, NM = m->grp.nm, gpb = m->grp.rpb;
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
    HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)m->grp.shmem));
    const DevMech dm = m->dm;
    const double* pA = Asv ? dA : nullptr;
    void* args[] = {(void*)&dm, (void*)&N, (void*)&dT, (void*)&pA, (void*)&du_, (void*)&ddu, (void*)&dJ, (void*)&dws};
    HIPCHK(hipLaunchKernel(fn, dim3(blocks), dim3(m->grp.threads), args, m->grp.shmem, 0));
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

// rate multipliers of a check's launch (host arrays, checked as br_integrate checks them): the table and the
// row indices to the device, the launch's half of the MultBlock, and the tag on the launch's g_par
static int debug_stage_mult(br_mech* m, int N, int nmult, const double* mult, const int* row, DevScratch& S, DevMech& dm) {
    if (nmult == 0) return 0;
    br_opts o{};
    o.nmult = nmult; o.rate_mult = mult; o.rate_mult_row = row;
    if (const int rc = check_mult_host(m, N, &o)) return rc;
    const size_t nt = (size_t)nmult * (m->nrg + m->nrs);
    double* dmult;
    int* drow = nullptr;
    HIPCHK(S.alloc(&dmult, std::max<size_t>(nt, 1) * 8));
    HIPCHK(hipMemcpy(dmult, mult, nt * 8, hipMemcpyHostToDevice));
    if (row) {
        HIPCHK(S.alloc(&drow, (size_t)N * 4));
        HIPCHK(hipMemcpy(drow, row, (size_t)N * 4, hipMemcpyHostToDevice));
    }
    hipLaunchKernelGGL(k_mult_block, dim3(1), dim3(64), 0, 0, m->mult_hdr, (const double*)dmult, (const int*)drow);
    HIPCHK(hipGetLastError());
    dm.g_par = reinterpret_cast<const double*>(reinterpret_cast<size_t>(dm.g_par) | 1u);
    return 0;
}

// ------------------------------------------------------------------------------------
// lane-engine checks (tests): the device functions of k_lane (brhip_lane.hpp) on their own, with k_lane's
// workgroup shape, LDS rows, global rows and buffer resource
// ------------------------------------------------------------------------------------
namespace {
// RHS and analytic Jacobian of reactors lane + 64 (block + k blocks), k = 0, 1, ..., one after another in the
// lane's LDS rows and global rows: a lane that gets a second reactor (N > 64 blocks) reuses the T-only
// constants', the concentrations' and the saved-J rows with another T as in k_lane's refill. A lane without a
// reactor stays masked until the wave is done.
template <int NM>
__global__ __launch_bounds__(64) void k_lane_eval(DevMech M, int N, const double* __restrict__ Tv,
                                                  const double* __restrict__ U, double* __restrict__ DU,
                                                  double* __restrict__ Jout, double* __restrict__ Jg) {
    const int lane = threadIdx.x;
    const int n = MF(n);
    const LaneLay LL = lane_lay(NM, n, MF(nset), MF(nrg), MF(nfo));
    double* Lp = reinterpret_cast<double*>(br_lds) + lane;
    Lp[(LL.conc + n) * 64] = 1.0;
    GRows G;
    G.r = __builtin_amdgcn_make_buffer_rsrc(Jg, 0, 0x7fffffff, 0x00020000);
    G.vo = lane * 8;
    G.base = blockIdx.x * LL.g_rows * 512;
    const int stride = 64 * (int)gridDim.x;
    for (int rid = lane + 64 * (int)blockIdx.x;; rid += stride) {
        const bool has = rid < N;
        if (!__any(has)) break;
        if (has) {
            lane_tconst(LL, Lp, G, Tv[rid], n, rid);
            double y[NM], f[NM];
#pragma unroll
            for (int i = 0; i < NM; ++i) y[i] = i < n ? U[(size_t)rid * n + i] : 0.0;
            lane_rhs<NM>(LL, Lp, G, y, n, f);
#pragma unroll
            for (int i = 0; i < NM; ++i) if (i < n) DU[(size_t)rid * n + i] = f[i];
            lane_jac<NM>(LL, Lp, G, n);                                 // (reads the concentrations the RHS left)
#pragma unroll
            for (int j = 0; j < NM; ++j)
#pragma unroll
                for (int i = 0; i < NM; ++i)                            // the saved-J rows as k_lane's LU setup reads them
                    if (i < n && j < n) Jout[((size_t)rid * n + i) * n + j] = G.ld(j * NM + i);
        }
    }
}

// l_getrf + l_getrs of matrix i in lane i mod 64 of block i / 64: J through the lane's saved-J rows, I - gamma J
// in k_lane's expression order, the factors and reciprocal pivots through the g_lu / g_rpv rows. A lane with
// skip[i] != 0 does nothing (in the integrator only some lanes of a wave set up).
template <int NM>
__global__ __launch_bounds__(64) void k_lane_lu(int N, int n, const double* __restrict__ J, const double* __restrict__ g,
                                                const double* __restrict__ b, const int* __restrict__ skip,
                                                double* __restrict__ x, int* __restrict__ fail_out, int* __restrict__ piv,
                                                double* __restrict__ Jg) {
    const int lane = threadIdx.x;
    const int i = (int)blockIdx.x * 64 + lane;
    const LaneLay LL = lane_lay(NM, n, 0, 0, 0);
    GRows G;
    G.r = __builtin_amdgcn_make_buffer_rsrc(Jg, 0, 0x7fffffff, 0x00020000);
    G.vo = lane * 8;
    G.base = blockIdx.x * LL.g_rows * 512;
    const bool act = i < N && !(skip && skip[i]);
    if (act) {
#pragma unroll
        for (int c = 0; c < NM; ++c)
#pragma unroll
            for (int r = 0; r < NM; ++r)
                if (r < n && c < n) G.st(c * NM + r, J[((size_t)i * n + r) * n + c]);
        const double mg = -g[i];
        double a[NM][NM], rpv[NM], rhs_[NM];
        unsigned long long pv = 0;
#pragma unroll
        for (int c = 0; c < NM; ++c)
#pragma unroll
            for (int r = 0; r < NM; ++r) a[r][c] = (r < n && c < n) ? G.ld(c * NM + r) : 0.0;
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int c = 0; c < NM; ++c)
#pragma unroll
            for (int r = 0; r < NM; ++r) a[r][c] = a[r][c] * mg + (r == c ? 1.0 : 0.0);
        const int f = l_getrf<NM>(a, pv, rpv);
#pragma unroll
        for (int c = 0; c < NM; ++c) {
            G.st(LL.g_rpv + c, rpv[c]);
#pragma unroll
            for (int r = 0; r < NM; ++r) G.st(LL.g_lu + c * NM + r, a[r][c]);
        }
#pragma unroll
        for (int r = 0; r < NM; ++r) rhs_[r] = r < n ? b[(size_t)i * n + r] : 0.0;
        if (!f) l_getrs<NM>(G, LL, pv, rhs_);                           // (k_lane: no solve after a zero pivot)
#pragma unroll
        for (int r = 0; r < NM; ++r)
            if (r < n) {
                x[(size_t)i * n + r] = f ? 0.0 : rhs_[r];
                piv[(size_t)i * n + r] = (int)((pv >> (4 * r)) & 15);
            }
        fail_out[i] = f;
    }
}

// ------------------------------------------------------------------------------------
// wavefront-engine check (tests): init_tconst<CPL, true>, rhs and jacobian in the integrator's configuration
// (wave_ctx<CPL, NMAX>, rpb waves per workgroup on one table block, the per-slot workspace of k_integrate)
// ------------------------------------------------------------------------------------
// RHS and analytic Jacobian of reactors slot, slot + G, slot + 2G, ... (G = waves of the grid), one after
// another in the wave's LDS block and workspace slot. With Tprev: the constants are first built at Tprev[rid]
// and used by one discarded RHS, then rebuilt at T[rid] in the live slot by the refresh sequence of
// k_integrate's temperature-programme instances (wave_sync, init_tconst) before the evaluation.
template <int NMAX>
__global__ __launch_bounds__(64 * br_maxrpb(NMAX)) void k_wave_eval(DevMech M, int N, int rpb, const double* __restrict__ Tv,
                                                                    const double* __restrict__ Asvv,
                                                                    const double* __restrict__ U,
                                                                    const double* __restrict__ Tprev,
                                                                    double* __restrict__ DU, double* __restrict__ Jout,
                                                                    double* __restrict__ Jws) {
    constexpr int CPL = NMAX > 64 ? 2 : 1;
    constexpr int JW = NMAX > 64 ? CR2 : 64;                            // column stride of the saved J (col_rows)
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const WaveCtx W = wave_ctx<CPL, NMAX>(M, smem_raw, rpb, Jws);
    const int widx = W.rid;                                             // workspace slot of this wave
    const int G = (int)gridDim.x * rpb;
    const int lane = W.lane;
    const Tab& tb = W.tb;
    const RView& S = W.R;
    const int n = M.n;
    double* Jsave = Jws + (size_t)widx * ws_doubles(NMAX, M.nrg);       // as k_integrate lays its slot out
    double* jscr = Jsave + NMAX * col_rows(NMAX);
    double* p_last = reinterpret_cast<double*>(W.rbase);
    const int legs = Tprev ? 2 : 1;
    for (int rid = widx; rid < N; rid += G) {
        wave_sync();
        const double Asv = Asvv ? Asvv[rid] : 1.0;
        const double Asv_th = (M.conv & 4) ? 1.0 : Asv;
        double u[CPL], du[CPL];
#pragma unroll
        FOR_S u[s] = CS < n ? U[(size_t)rid * n + CS] : 0.0;
        double T = 0.0;
#pragma unroll 1
        for (int leg = 0; leg < legs; ++leg) {                          // (one copy of init_tconst and rhs)
            T = uni(leg == legs - 1 ? Tv[rid] : Tprev[rid]);
            if (leg) wave_sync();                                       // tprog_refresh
            init_tconst<CPL, true>(M, tb, S, T, lane, rid);
            rhs<CPL>(M, tb, S, T, Asv, Asv_th, u, lane, p_last, du);    // (leg 0 of 2: discarded)
        }
#pragma unroll
        FOR_S if (CS < n) DU[(size_t)rid * n + CS] = du[s];
        jacobian<CPL>(M, tb, S, T, Asv, Asv_th, u, lane, Jsave, jscr);
        // the saved J as lu_factor / lu_factor2 read it: a buffer of n columns of JW rows, row per lane
        const __amdgpu_buffer_rsrc_t rj =
            __builtin_amdgcn_make_buffer_rsrc((void*)launder(Jsave), (short)0, n * (JW * 8), 0x00020000);
#pragma unroll
        FOR_S {
            if (CS < n) {
                double* row = Jout + ((size_t)rid * n + CS) * n;
                for (int j = 0; j < n; ++j)
                    row[j] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rj, (unsigned)CS * 8u, j * (JW * 8), 0));
            }
        }
    }
}

// ------------------------------------------------------------------------------------
// energy-run check (tests): the right-hand side of k_integrate<NMAX, false, true> through its own device
// functions (energy_wave_ctx, energy_tclamp, init_tconst<1, true>, energy_thermo, rhs<1>, energy_tdot), rpb
// waves per workgroup on one table block, the per-slot workspace of the integrator. Reactors slot, slot + G, ...
// one after another in the wave's block and slot. Two legs per reactor, as a refresh in a run: the constants
// and e_k, cv_k are first built at a temperature 150 K above (one discarded evaluation), then rebuilt at T.
// ------------------------------------------------------------------------------------
template <int NMAX>
__global__ __launch_bounds__(64 * br_maxrpb(NMAX)) void k_energy_eval(DevMech M, int N, int rpb, const double* __restrict__ Tv,
                                                                      const double* __restrict__ U, double* __restrict__ DU,
                                                                      double* __restrict__ Jws) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const WaveCtx W = energy_wave_ctx<NMAX>(M, smem_raw, rpb, Jws);
    const int widx = W.rid;
    const int G = (int)gridDim.x * rpb;
    const int lane = W.lane;
    const Tab& tb = W.tb;
    const RView& S = W.R;
    const int n = M.n;
    double* p_last = reinterpret_cast<double*>(W.rbase);
    for (int rid = widx; rid < N; rid += G) {
        wave_sync();
        double y[1], f[1];
        y[0] = lane < n ? U[(size_t)rid * n + lane] : (lane == n ? uni(Tv[rid]) : 0.0);
        double T = 0.0, ek = 0.0, cvk = 0.0;
#pragma unroll 1
        for (int leg = 0; leg < 2; ++leg) {
            const double Tl = energy_tclamp(uni(bcast(y[0], n)) + (leg == 0 ? 150.0 : 0.0));
            T = Tl;
            if (leg) wave_sync();
            init_tconst<1, true>(M, tb, S, T, lane, rid);
            energy_thermo(lane, n, T, ek, cvk);
            rhs<1>(M, tb, S, T, 1.0, 1.0, y, lane, p_last, f);
            const double Td = energy_tdot(tb, lane, n, y[0], f[0], ek, cvk);
            if (lane == n) f[0] = Td;
        }
        if (lane <= n) DU[(size_t)rid * (n + 1) + lane] = f[0];
    }
}

// ... of the group engine's energy instances (k_group<GL, NM, true>): their device functions (energy_tclamp,
// g_init_tconst<GL> with the reactor's multiplier row, energy_thermo, g_rhs<GL>, energy_tdot<GL>) in k_group's
// workgroup shape, LDS blocks and global slots. Reactors slot, slot + G, ... one after another in the group's
// block and slot; two legs per reactor as above, the second through the refresh sequence of k_group (wave_sync,
// g_init_tconst in the live slot), under the same group divergence.
template <int GL, int NM>
__global__ __launch_bounds__(64 * BR_QWPB) __attribute__((amdgpu_waves_per_eu(GL == 16 ? BR_QWPE : BR_QWPE32))) void k_group_energy_eval(
    DevMech M, int N, const double* __restrict__ Tv, const double* __restrict__ U, double* __restrict__ DU,
    double* __restrict__ Jws) {
    GRP_CONTEXT(M, Jws);
    (void)asv_fixed; (void)jst; (void)jld;                              // (gas-only, no Jacobian here)
    const int G = (int)gridDim.x * (BR_QWPB * GPW);
    for (int rid = slot;; rid += G) {
        if (__ballot(rid < N) == 0) break;
        if (rid < N) {                                                  // (idle groups wait, as k_group's)
            const double y = gl < n ? U[(size_t)rid * n + gl] : (gl == n ? Tv[rid] : 0.0);
            double T = 0.0, ek = 0.0, cvk = 0.0, fv = 0.0;
#pragma unroll 1
            for (int leg = 0; leg < 2; ++leg) {
                T = energy_tclamp(gbcast<GL>(y, n) + (leg == 0 ? 150.0 : 0.0));
                if (leg) wave_sync();
                g_init_tconst<GL>(tb, sp, kd, fod, skd, T, gl, rid);
                energy_thermo(gl, n, T, ek, cvk);
                fv = g_rhs<GL>(tb, sp, kd, fod, skd, T, 1.0, 1.0, y, gl, p_last);
                const double Td = energy_tdot<GL>(tb, gl, n, y, fv, ek, cvk);
                if (gl == n) fv = Td;
            }
            if (gl <= n) DU[(size_t)rid * (n + 1) + gl] = fv;
            wave_sync();
        }
    }
}
}  // namespace

static const void* energy_eval_kernel(int nmax) {
    return nmax == 16 ? (const void*)k_energy_eval<16> : nmax == 32 ? (const void*)k_energy_eval<32>
         : nmax == 56 ? (const void*)k_energy_eval<56> : nullptr;
}
static const void* lane_eval_kernel(int nm) {
    return nm == 9 ? (const void*)k_lane_eval<9> : nm == 12 ? (const void*)k_lane_eval<12> : nullptr;
}
static const void* lane_lu_kernel(int nm) {
    return nm == 9 ? (const void*)k_lane_lu<9> : nm == 12 ? (const void*)k_lane_lu<12> : nullptr;
}
static const void* wave_eval_kernel(int nmax) {
    return nmax == 16 ? (const void*)k_wave_eval<16> : nmax == 32 ? (const void*)k_wave_eval<32>
         : nmax == 56 ? (const void*)k_wave_eval<56> : nmax == 64 ? (const void*)k_wave_eval<64>
         : nmax == 72 ? (const void*)k_wave_eval<72> : nullptr;
}

extern "C" int br_debug_lane_eval(br_mech* m, int N, const double* T, const double* u, int nmult, const double* rate_mult,
                                  const int* rate_mult_row, double* du, double* J) {
    if (!m || N <= 0 || !T || !u || !du || !J) return fail(BR_ERR_INPUT, "bad argument");
    if (!m->lane.nm) return fail(BR_ERR_UNSUPPORTED, "mechanism is not eligible for the lane engine");
    HIPCHK(hipSetDevice(m->device));
    const int n = m->n, NM = m->lane.nm;
    // small fixed grid: one workgroup up to 128 reactors, else two, so that lanes take a second reactor in
    // the rows of their first from N = 65 on (N = 100: lanes 0..35 of the one workgroup; N >= 192: every lane)
    const int blocks = std::min(2, (N + 127) / 128);
    const size_t rows = (size_t)lane_lay(NM, n, m->dm.nset, m->nrg, m->dm.nfo).g_rows;
    double *dT, *du_, *ddu, *dJ, *dws;
    DevScratch S;
    DevMech dm = m->dm;
    if (const int rc = debug_stage_mult(m, N, nmult, rate_mult, rate_mult_row, S, dm)) return rc;
    HIPCHK(S.alloc(&dT, (size_t)N * 8));
    HIPCHK(S.alloc(&du_, (size_t)N * n * 8));
    HIPCHK(S.alloc(&ddu, (size_t)N * n * 8));
    HIPCHK(S.alloc(&dJ, (size_t)N * n * n * 8));
    HIPCHK(S.alloc(&dws, rows * blocks * 64 * 8));
    HIPCHK(hipMemcpy(dT, T, (size_t)N * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(du_, u, (size_t)N * n * 8, hipMemcpyHostToDevice));
    const void* fn = lane_eval_kernel(NM);
    if (!fn) return fail(BR_ERR_UNSUPPORTED, "no lane check kernel of this width");
    HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)m->lane.shmem));
    void* args[] = {(void*)&dm, (void*)&N, (void*)&dT, (void*)&du_, (void*)&ddu, (void*)&dJ, (void*)&dws};
    HIPCHK(hipLaunchKernel(fn, dim3(blocks), dim3(64), args, m->lane.shmem, 0));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(du, ddu, (size_t)N * n * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(J, dJ, (size_t)N * n * n * 8, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int br_debug_lane_lu_solve(int nm, int N, int n, const double* J, const double* gamma, const double* b,
                                      const int* skip, double* x, int* fail_out, int* piv) {
    const void* fn = lane_lu_kernel(nm);
    if (!fn || N <= 0 || n < 1 || n > nm || !J || !gamma || !b || !x || !fail_out || !piv) return fail_code_input();
    const int blocks = (N + 63) / 64;
    const size_t rows = (size_t)lane_lay(nm, n, 0, 0, 0).g_rows;
    double *dJ, *dg, *db, *dx, *dws;
    int *df, *dp, *dsk = nullptr;
    DevScratch S;
    HIPCHK(S.alloc(&dJ, (size_t)N * n * n * 8));
    HIPCHK(S.alloc(&dg, (size_t)N * 8));
    HIPCHK(S.alloc(&db, (size_t)N * n * 8));
    HIPCHK(S.alloc(&dx, (size_t)N * n * 8));
    HIPCHK(S.alloc(&dws, rows * blocks * 64 * 8));
    HIPCHK(S.alloc(&df, (size_t)N * 4));
    HIPCHK(S.alloc(&dp, (size_t)N * n * 4));
    HIPCHK(hipMemcpy(dJ, J, (size_t)N * n * n * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dg, gamma, (size_t)N * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(db, b, (size_t)N * n * 8, hipMemcpyHostToDevice));
    // (the outputs start from the caller's values: a skipped lane writes none)
    HIPCHK(hipMemcpy(dx, x, (size_t)N * n * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(df, fail_out, (size_t)N * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dp, piv, (size_t)N * n * 4, hipMemcpyHostToDevice));
    if (skip) {
        HIPCHK(S.alloc(&dsk, (size_t)N * 4));
        HIPCHK(hipMemcpy(dsk, skip, (size_t)N * 4, hipMemcpyHostToDevice));
    }
    void* args[] = {(void*)&N, (void*)&n, (void*)&dJ, (void*)&dg, (void*)&db, (void*)&dsk, (void*)&dx, (void*)&df, (void*)&dp,
                    (void*)&dws};
    HIPCHK(hipLaunchKernel(fn, dim3(blocks), dim3(64), args, 0, 0));
    HIPCHK(hipMemcpy(x, dx, (size_t)N * n * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(fail_out, df, (size_t)N * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(piv, dp, (size_t)N * n * 4, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int br_debug_wave_eval(br_mech* m, int N, const double* T, const double* Asv, const double* u, const double* T_prev,
                                  int nmult, const double* rate_mult, const int* rate_mult_row, double* du, double* J) {
    if (!m || N <= 0 || !T || !u || !du || !J) return fail(BR_ERR_INPUT, "bad argument");
    HIPCHK(hipSetDevice(m->device));
    const int n = m->n, rpb = m->wave.rpb;
    // small fixed grid: one workgroup up to 4 rpb reactors, else two, so that every wave takes a second
    // reactor in the slot of its first from N = 2 rpb (one workgroup) or 4 rpb (two) on
    const int blocks = std::min(2, (N + 4 * rpb - 1) / (4 * rpb));
    double *dT, *dA, *du_, *dTp = nullptr, *ddu, *dJ, *dws;
    DevScratch S;
    DevMech dm = m->dm;
    if (const int rc = debug_stage_mult(m, N, nmult, rate_mult, rate_mult_row, S, dm)) return rc;
    HIPCHK(S.alloc(&dT, (size_t)N * 8));
    HIPCHK(S.alloc(&dA, (size_t)N * 8));
    HIPCHK(S.alloc(&du_, (size_t)N * n * 8));
    HIPCHK(S.alloc(&ddu, (size_t)N * n * 8));
    HIPCHK(S.alloc(&dJ, (size_t)N * n * n * 8));
    HIPCHK(S.alloc(&dws, (size_t)blocks * rpb * ws_doubles(m->nmax, m->nrg) * 8));
    HIPCHK(hipMemcpy(dT, T, (size_t)N * 8, hipMemcpyHostToDevice));
    if (Asv) HIPCHK(hipMemcpy(dA, Asv, (size_t)N * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(du_, u, (size_t)N * n * 8, hipMemcpyHostToDevice));
    if (T_prev) {
        HIPCHK(S.alloc(&dTp, (size_t)N * 8));
        HIPCHK(hipMemcpy(dTp, T_prev, (size_t)N * 8, hipMemcpyHostToDevice));
    }
    const void* fn = wave_eval_kernel(m->nmax);
    if (!fn) return fail(BR_ERR_UNSUPPORTED, "no wavefront check kernel of this width");
    HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)m->wave.shmem));
    const double* pA = Asv ? dA : nullptr;
    void* args[] = {(void*)&dm, (void*)&N, (void*)&rpb, (void*)&dT, (void*)&pA, (void*)&du_, (void*)&dTp, (void*)&ddu, (void*)&dJ,
                    (void*)&dws};
    HIPCHK(hipLaunchKernel(fn, dim3(blocks), dim3(64 * rpb), args, m->wave.shmem, 0));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(du, ddu, (size_t)N * n * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(J, dJ, (size_t)N * n * n * 8, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int br_debug_energy_eval(br_mech* m, int N, const double* T, const double* u, int nmult, const double* rate_mult,
                                    const int* rate_mult_row, double* du) {
    if (!m || N <= 0 || !T || !u || !du) return fail(BR_ERR_INPUT, "bad argument");
    HIPCHK(hipSetDevice(m->device));
    if (const int rc = energy_shape(m)) return rc;
    const int n = m->n, rpb = m->wave_e.rpb, nmax = m->wave_e.nm;
    const int blocks = std::min(2, (N + 4 * rpb - 1) / (4 * rpb));   // (as br_debug_wave_eval)
    double *dT, *du_, *ddu, *dws;
    DevScratch S;
    DevMech dm = m->dm;
    if (const int rc = debug_stage_mult(m, N, nmult, rate_mult, rate_mult_row, S, dm)) return rc;
    HIPCHK(S.alloc(&dT, (size_t)N * 8));
    HIPCHK(S.alloc(&du_, (size_t)N * n * 8));
    HIPCHK(S.alloc(&ddu, (size_t)N * (n + 1) * 8));
    HIPCHK(S.alloc(&dws, (size_t)blocks * rpb * ws_doubles(nmax, m->nrg) * 8));
    HIPCHK(hipMemcpy(dT, T, (size_t)N * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(du_, u, (size_t)N * n * 8, hipMemcpyHostToDevice));
    const void* fn = energy_eval_kernel(nmax);
    if (!fn) return fail(BR_ERR_UNSUPPORTED, "no energy check kernel of this width");
    HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)m->wave_e.shmem));
    void* args[] = {(void*)&dm, (void*)&N, (void*)&rpb, (void*)&dT, (void*)&du_, (void*)&ddu, (void*)&dws};
    HIPCHK(hipLaunchKernel(fn, dim3(blocks), dim3(64 * rpb), args, m->wave_e.shmem, 0));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(du, ddu, (size_t)N * (n + 1) * 8, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int br_debug_group_energy_eval(br_mech* m, int N, const double* T, const double* u, int nmult,
                                          const double* rate_mult, const int* rate_mult_row, double* du) {
    if (!m || N <= 0 || !T || !u || !du) return fail(BR_ERR_INPUT, "bad argument");
    HIPCHK(hipSetDevice(m->device));
    if (!group_energy_shape(m))
        return fail(BR_ERR_UNSUPPORTED, "mechanism has no group energy instance (gas-only, ng + 1 <= 32, <= 32 efficiency sets)");
    const int n = m->n, GL = m->grp_e.gl, NM = m->grp_e.nm, gpb = m->grp_e.rpb;
    const int blocks = std::min(2, (N + gpb - 1) / gpb);                // small fixed grid: the groups reuse their slots
    double *dT, *du_, *ddu, *dws;
    DevScratch S;
    DevMech dm = m->dm;
    if (const int rc = debug_stage_mult(m, N, nmult, rate_mult, rate_mult_row, S, dm)) return rc;
    HIPCHK(S.alloc(&dT, (size_t)N * 8));
    HIPCHK(S.alloc(&du_, (size_t)N * n * 8));
    HIPCHK(S.alloc(&ddu, (size_t)N * (n + 1) * 8));
    HIPCHK(S.alloc(&dws, (size_t)blocks * gpb * grp::slot_doubles(GL, m->nrg) * 8));
    HIPCHK(hipMemcpy(dT, T, (size_t)N * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(du_, u, (size_t)N * n * 8, hipMemcpyHostToDevice));
    const void* fn = grp_instance(GL, NM, [](auto g, auto w) { return (const void*)k_group_energy_eval<g(), w()>; });
    HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)m->grp_e.shmem));
    void* args[] = {(void*)&dm, (void*)&N, (void*)&dT, (void*)&du_, (void*)&ddu, (void*)&dws};
    HIPCHK(hipLaunchKernel(fn, dim3(blocks), dim3(m->grp_e.threads), args, m->grp_e.shmem, 0));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(du, ddu, (size_t)N * (n + 1) * 8, hipMemcpyDeviceToHost));
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
