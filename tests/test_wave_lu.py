"""The wavefront integrator's LU and solve (lu_factor / lu_solve, lu_factor2 / lu_solve2 of brhip_device.hpp) through
br_debug_wave_lu, which strings them together as k_integrate does: every factorization is solved with, the second
one loads its rows in the first one's pivot order, the workspace is dirty, several waves share a workgroup.
References (wave_lu_ref.py): denseGETRF's pivot order in float64 and long double on the matrix the device forms,
and the factors rebuilt from the device layout in long double against the componentwise backward bound."""
import functools

import numpy as np
import pytest

import wave_lu_ref as R
from test_group_kernels import _getrf_order, _lu_inputs

pytestmark = pytest.mark.gpu

BR_ERR_INPUT = -10
FILL = -7.0


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _live(F, n):
    """the factors in rows and columns < n, and D^-1 below n, of workspace copies F [..., W]"""
    Rr, Cc, _ = R.layout(n)
    M = F[..., :Rr * Cc].reshape(F.shape[:-1] + (Cc, Rr))[..., :n, :n]
    return np.concatenate([M.reshape(F.shape[:-1] + (-1,)), F[..., Rr * Cc:Rr * Cc + n]], axis=-1)


def _wave_lu(*a, **k):
    import _pkgload
    return _pkgload.load().Engine.wave_lu(*a, **k)


def _check_leg(n, A, b, x, f, perm, F, i, order=None, tag=""):
    """one matrix of one leg: no zero pivot, the solve's backward error, the pivot order, the structure the solve
    relies on and the factors' componentwise backward error; returns the two ratios"""
    assert f[i] == 0, (tag, i, f[i])
    assert np.all(np.isfinite(x[i])), (tag, i)
    rb = R.backward_ratio(A[i], b[i], x[i])
    assert rb <= 1e-12, (tag, i, rb)
    assert sorted(perm[i]) == list(range(n)), (tag, i, perm[i])
    if order is not None:
        assert np.array_equal(perm[i], order), (tag, i, perm[i], order)
    assert R.structure_errors(F[i], n) == [], (tag, i)
    rr = R.recon_ratio(F[i], n, A[i], perm[i])
    assert rr <= 1.0, (tag, i, rr)
    return rb, rr


# ---------------------------------------------------------------------------------------------
# 1-3. every size: the gather path against the no-gather path, the structure, the factors
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _every_size(n):
    J, g, b = _lu_inputs(n, 64, 7000 + n)
    A = R.newton_matrix(J, g)
    x, f, perm, F = _wave_lu(J, g, b, dirty=True, wpb=1)   # 64 matrices on 2 waves: 32 per slot
    order = [_getrf_order(A[i]) for i in range(64)]
    for a in (A, b, x, f, perm, F):
        a.setflags(write=False)
    return A, b, x, f, perm, F, order


@pytest.mark.parametrize("n", range(1, 73))
def test_every_size_solve_and_order(gpu, n):
    """n = 1..72, a reactor's first LU (identity order: search and gather) and its second (the first one's pivot
    order: fast path, no gather) of the same matrix, NaNs in the workspace: no failure, the 1e-12 backward error of
    both solves, both row orders denseGETRF's, and bit for bit the same x and factors from the two paths."""
    A, b, x, f, perm, F, order = _every_size(n)
    assert np.all(f == 0), f
    worst = 0.0
    for leg in range(2):
        for i in range(64):
            rb = R.backward_ratio(A[i], b[i], x[leg, i])
            worst = max(worst, rb)
            assert np.all(np.isfinite(x[leg, i])) and rb <= 1e-12, (leg, i, rb)
            assert np.array_equal(perm[leg, i], order[i]), (leg, i, perm[leg, i], order[i])
    assert _same_bits(x[0], x[1])
    assert _same_bits(_live(F[0], n), _live(F[1], n))
    print(f"wave_lu n={n} backward/1e-12 = {worst / 1e-12:.3e}")


@pytest.mark.parametrize("n", range(1, 73))
def test_every_size_structure(gpu, n):
    """what lu_solve / lu_solve2 rely on, in both workspace copies of every matrix, after a start from NaNs: exact
    zeros on the diagonal, in rows >= n and (n <= 64) in columns >= n, finite D^-1 with zeros beyond n, |L| <= 1"""
    A, b, x, f, perm, F, order = _every_size(n)
    for leg in range(2):
        for i in range(64):
            assert R.structure_errors(F[leg, i], n) == [], (leg, i)


@pytest.mark.parametrize("n", range(1, 73))
def test_every_size_reconstruction(gpu, n):
    """|L U - P A| <= gamma_(n+4) |L| |U| componentwise in long double, L, U from the device layout and P the
    device's own row order, for both factorizations of every matrix"""
    A, b, x, f, perm, F, order = _every_size(n)
    worst = 0.0
    for leg in range(2):
        for i in range(64):
            rr = R.recon_ratio(F[leg, i], n, A[i], perm[leg, i])
            worst = max(worst, rr)
            assert rr <= 1.0, (leg, i, rr)
    print(f"wave_lu n={n} reconstruction/bound = {worst:.3f}")


# ---------------------------------------------------------------------------------------------
# 4. a changed pivot order: the second matrix differs, some pivots keep their lane and some do not
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [9, 16, 20, 32, 33, 53, 56, 60, 64, 66, 72])
def test_changed_pivot_order(gpu, n):
    """Leg B factors J1 = J0 (1 + 0.3 xi), gamma1 = 1.7 gamma0 with the rows where leg A's pivots left them: in at
    least half the matrices the order changes, with pivots both on and off their own lane (fast path and full
    search mixed, a gather from a non-identity placement). Leg B's solve, row order and factors are checked as a
    first LU's, and must equal bit for bit those of the same matrix factored from the identity order."""
    N = 64
    seed = {9: 9109}.get(n, 8000 + n)                # (n = 9: a seed whose inputs meet the first assertion below)
    J0, g0, b = _lu_inputs(n, N, seed)
    rng = np.random.default_rng(seed + 100)
    J1 = J0 * (1 + 0.3 * rng.standard_normal(J0.shape))
    g1 = 1.7 * g0
    A0, A1 = R.newton_matrix(J0, g0), R.newton_matrix(J1, g1)
    o0 = [_getrf_order(A0[i]) for i in range(N)]
    o1 = [_getrf_order(A1[i]) for i in range(N)]
    changed = [i for i in range(N) if not np.array_equal(o0[i], o1[i])]
    assert 2 * len(changed) >= N, len(changed)
    for i in changed:                                # (a step keeps its lane when both orders name the same row)
        assert np.any(o0[i] == o1[i]) and np.any(o0[i] != o1[i]), i
    x, f, perm, F = _wave_lu(J0, g0, b, J1=J1, gamma1=g1, dirty=True)
    xs, fs, ps, Fs = _wave_lu(J1, g1, b, dirty=True)
    for i in range(N):
        _check_leg(n, A0, b, x[0], f[0], perm[0], F[0], i, o0[i], "A")
        _check_leg(n, A1, b, x[1], f[1], perm[1], F[1], i, o1[i], "B")
    assert np.all(fs[0] == 0) and np.array_equal(ps[0], perm[1])
    assert _same_bits(xs[0], x[1])
    assert _same_bits(_live(Fs[0], n), _live(F[1], n))


# ---------------------------------------------------------------------------------------------
# 5. ties and the tie key
# ---------------------------------------------------------------------------------------------
_TIE_KINDS = ("pm", "mp", "low", "flat", "diag", "inter")


def _tie_matrix(n, c, kind, seed):
    """one ill-scaled matrix whose leading c x c block of I - gamma J is the identity with zeros below it, so that
    steps 0..c-1 leave the rest untouched and column c reaches step c exactly as planted (gamma a power of two):
    pm / mp: +v, -v / -v, +v on rows r1 < r2; low: v, v (1 + 2^-40), v (1 + 2^-40) on r1 < r2 < r3 (they differ in
    the low word only); flat: every |a_ic| = 1, i >= c; diag: +v on row c itself and -v on r2; inter: no tie, a
    larger entry two rows down. Returns (J, gamma, b, winner, the other tied row or None)."""
    J, g, b = _lu_inputs(n, 1, seed)
    J, g, b = J[0], g[0], b[0]
    g = 2.0 ** np.round(np.log2(g))
    J[c:, :c] = 0.0
    J[:c, :c] = 0.0
    r1, r2, r3 = c + 1, c + (n - c) // 2 + 1, n - 1
    assert c < r1 < r2 < r3
    big = np.ldexp(1.25, int(np.ceil(np.log2(4 * np.abs(J[c:, c]).max() + 4 / g))))   # g big > every |a_ic|
    if kind == "pm":
        J[r1, c], J[r2, c] = -big, big
        win, other = r1, r2
    elif kind == "mp":
        J[r1, c], J[r2, c] = big, -big
        win, other = r1, r2
    elif kind == "low":
        J[r1, c], J[r2, c], J[r3, c] = big, -big * (1 + 2.0 ** -40), big * (1 + 2.0 ** -40)
        win, other = r2, r3
    elif kind == "flat":
        J[c:, c] = np.where(np.arange(c, n) % 2, 1.0, -1.0) / g
        J[c, c] = 0.0
        win, other = c, r3
    elif kind == "diag":
        v = g * big
        assert v >= 5.0 and v == np.floor(v) and v < 2.0 ** 52
        J[c, c], J[r2, c] = -(v - 1.0) / g, big      # a_cc = 1 + (v - 1) = v exactly, a_r2c = -v
        win, other = c, r2
    else:
        J[c, c], J[c + 2, c] = 0.0, -big
        win, other = c + 2, None
    A = R.newton_matrix(J[None], np.array([g]))[0]
    assert np.array_equal(A[:c, :c], np.eye(c)) and not np.any(A[c:, :c])
    col = np.abs(A[c:, c])
    assert c + int(np.argmax(col)) == win
    ties = int(np.sum(col == col.max()))
    assert ties == {"flat": n - c, "inter": 1}.get(kind, 2), (kind, ties)
    if kind == "low":
        assert col[r1 - c] < col.max() and _bits(col[r1 - c]) >> 32 == _bits(col.max()) >> 32
    return J, g, b, win, other


def _place(n, where):
    """row order (position -> original row) that differs from the identity by the fewest exchanges that put
    row r on position p for every (r, p) of `where`"""
    v = np.arange(n, dtype=np.int32)
    for r, p in where:
        cur = int(np.flatnonzero(v == r)[0])
        v[[cur, p]] = v[[p, cur]]
    for r, p in where:
        assert v[p] == r
    assert sorted(v) == list(range(n))
    return v


def _placements(n, c, win, other):
    """the identity; the loser on the winner's position and the winner on the loser's (the higher-numbered tied
    row on the lower lane; for a tie with row c itself the loser on lane c); n > 64: the loser in slot 0 with
    the winner in slot 1 (a lower position, and the slot that is looked at first), and the loser on lane 0 of
    slot 1 with the winner on a higher lane of slot 0 (a lower lane, in the other slot)"""
    pl = [np.arange(n, dtype=np.int32)]
    if other is None:
        return pl
    pl.append(_place(n, [(other, win), (win, other)]))
    if n > 64:
        pl.append(_place(n, [(other, c + 1 if c + 1 < 64 else 3), (win, n - 1)]))
        pl.append(_place(n, [(other, 64), (win, c + 5 if c + 5 < 64 else 40)]))
    return pl


@pytest.mark.parametrize("n,c", [(9, 0), (16, 0), (20, 0), (53, 0), (40, 32), (53, 32), (64, 32), (66, 0), (72, 16),
                                 (70, 64), (72, 64)])
def test_ties_go_to_the_lowest_original_row(gpu, n, c):
    """Exact ties at step c (column 0; the first column of the second panel of lu_factor; columns 16 and 64 of
    lu_factor2) under several row placements: the identity, the two tied rows exchanged (the higher-numbered one
    on the lower position), for n > 64 the winner moved to the other slot, and for the tie with row c itself the
    loser on lane c (the fast path must give way to the search). No interchange precedes step c, so denseGETRF's
    first maximum is the lower ORIGINAL row: that is the pivot every time,
    and row order, x and factors are those of the identity placement bit for bit."""
    mats, places = [], []
    for kind in _TIE_KINDS:
        J, g, b, win, other = _tie_matrix(n, c, kind, 9000 + 100 * n + c)
        for p in _placements(n, c, win, other):
            mats.append((kind, J, g, b, win))
            places.append(p)
    N = len(mats)
    J = np.stack([m[1] for m in mats])
    g = np.array([m[2] for m in mats])
    b = np.stack([m[3] for m in mats])
    A = R.newton_matrix(J, g)
    x, f, perm, F = _wave_lu(J, g, b, perm_in=np.stack(places), dirty=True)
    base = 0
    for i, (kind, _, _, _, win) in enumerate(mats):
        if np.array_equal(places[i], np.arange(n)):
            base = i                                 # the identity placement of this matrix
        order = _getrf_order(A[i])
        assert order[c] == win
        for leg in range(2):
            assert perm[leg, i][c] == win, (kind, i, leg, perm[leg, i][c], win)
            _check_leg(n, A, b, x[leg], f[leg], perm[leg], F[leg], i, order, f"{kind}/{leg}")
            assert np.array_equal(perm[leg, i], perm[0, base]), (kind, i, leg)
            assert _same_bits(x[leg, i], x[0, base]), (kind, i, leg)
            assert _same_bits(_live(F[leg, i], n), _live(F[0, base], n)), (kind, i, leg)
    kinds = [m[0] for m in mats]
    i_flat, i_int = kinds.index("flat"), kinds.index("inter")
    assert perm[0, i_flat][c] == c and perm[0, i_int][c] == c + 2   # no interchange next to one that interchanges


@pytest.mark.parametrize("n", [9, 20, 53, 64, 66, 72])
def test_tie_after_an_interchange_follows_getrf(gpu, n):
    """Step 0 takes row 4 (|a_40| = 4 > a_00 = 1), so denseGETRF moves row 0 to position 4; at step 1 rows 0 and 2
    tie exactly (+8, -8). denseGETRF's first maximum is then row 2 (position 2), not row 0, the lower original row:
    the tie key is the position in denseGETRF's interchanged order. Every placement gives that order, and x and
    the factors of the identity placement bit for bit."""
    J, g, b = _lu_inputs(n, 1, 9500 + n)
    J, g, b = J[0], 2.0 ** np.round(np.log2(g[0])), b[0]
    J[:, :2] = 0.0
    J[4, 0] = -4.0 / g                               # a_40 = 4
    J[0, 1], J[2, 1] = -8.0 / g, 8.0 / g             # a_01 = 8, a_21 = -8 (a_41 = 0: row 0 keeps its 8 at step 0)
    places = _placements(n, 1, 2, 0)
    N = len(places)
    Js, gs, bs = np.stack([J] * N), np.full(N, g), np.stack([b] * N)
    A = R.newton_matrix(Js, gs)
    order = _getrf_order(A[0])
    assert list(order[:2]) == [4, 2] and list(np.abs(A[0][[0, 2], 1])) == [8.0, 8.0] and np.abs(A[0][:, 1]).max() == 8.0
    x, f, perm, F = _wave_lu(Js, gs, bs, perm_in=np.stack(places), dirty=True)
    for i in range(N):
        for leg in range(2):
            assert list(perm[leg, i][:2]) == [4, 2], (i, leg, perm[leg, i][:3])
            _check_leg(n, A, bs, x[leg], f[leg], perm[leg], F[leg], i, order, f"place {i} leg {leg}")
            assert _same_bits(x[leg, i], x[0, 0]) and _same_bits(_live(F[leg, i], n), _live(F[0, 0], n)), (i, leg)


# ---------------------------------------------------------------------------------------------
# 6. sparse stoichiometric matrices: ties at many steps
# ---------------------------------------------------------------------------------------------
def _sparse_inputs(n, N, seed):
    rng = np.random.default_rng(seed)
    J = rng.integers(-2, 3, (N, n, n)).astype(np.float64) * (rng.random((N, n, n)) < 0.25)
    return J, np.full(N, 0.25), rng.standard_normal((N, n))


@pytest.mark.parametrize("n", range(1, 73))
def test_sparse_integer_matrices(gpu, n):
    """J with entries -2..2 at density 0.25, gamma = 0.25: exact small multiples of 1/4, so equal column entries
    (ties) at many steps. Backward error, reconstruction bound, structure and the bit identity of the two legs
    for every matrix; the row order wherever denseGETRF in float64 and in long double agree on it (a tie that
    rounding makes or breaks has no single reference order). At most 2 of the 64 matrices may be exempt, which the
    references alone must meet."""
    N = 64
    J, g, b = _sparse_inputs(n, N, 10000 + n)
    A = R.newton_matrix(J, g)
    assert np.array_equal(A, np.eye(n) - 0.25 * J)
    o64 = [_getrf_order(A[i]) for i in range(N)]
    old = [R.getrf_order(A[i], R.LD) for i in range(N)]
    agree = [np.array_equal(o64[i], old[i]) for i in range(N)]
    assert N - sum(agree) <= 2, N - sum(agree)
    assert max(np.linalg.cond(A[i]) for i in range(N)) < 1e8          # (none singular: integer matrices can be)
    x, f, perm, F = _wave_lu(J, g, b, dirty=True)
    for i in range(N):
        for leg in range(2):
            _check_leg(n, A, b, x[leg], f[leg], perm[leg], F[leg], i, o64[i] if agree[i] else None, f"leg {leg}")
    assert np.array_equal(perm[0], perm[1])
    assert _same_bits(x[0], x[1])
    assert _same_bits(_live(F[0], n), _live(F[1], n))


# ---------------------------------------------------------------------------------------------
# 7. zero pivots
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 9, 20, 33, 53, 60, 64, 66, 72])
def test_zero_pivot_flag(gpu, n):
    """Column k of I - gamma J exactly zero (gamma = 0.5, J[:, k] = 2 e_k) for k = 0, n - 1 and every panel edge
    below n (31, 32 of lu_factor; 15, 16, 47, 48, 63, 64 of lu_factor2), NaNs in the workspace: fail = k + 1 in
    both legs and x untouched; two zero columns report the first; the matrices in between are unaffected."""
    edges = (15, 16, 47, 48, 63, 64) if n > 64 else (31, 32)
    ks = sorted({0, n - 1} | {k for k in edges if k < n})
    N = 3 * len(ks) + 4
    J, g, b = _lu_inputs(n, N, 11000 + n)
    sing = {}
    for c, k in enumerate(ks):
        i = 3 * c + 1
        g[i] = 0.5
        J[i, :, k] = 0.0
        J[i, k, k] = 2.0
        sing[i] = k
    if len(ks) > 1:                                  # two zero columns: the first is reported
        i = 3 * len(ks) + 1
        g[i] = 0.5
        for k in (ks[-1], ks[(len(ks) - 1) // 2]):
            J[i, :, k] = 0.0
            J[i, k, k] = 2.0
        sing[i] = ks[(len(ks) - 1) // 2]
    A = R.newton_matrix(J, g)
    for i, k in sing.items():
        assert not np.any(A[i][:, k])
    x, f, perm, F = _wave_lu(J, g, b, dirty=True, fill=FILL)
    for i in range(N):
        for leg in range(2):
            if i in sing:
                assert f[leg, i] == sing[i] + 1, (i, leg, f[leg, i], sing[i])
                assert np.all(x[leg, i] == FILL), (i, leg)
            else:
                _check_leg(n, A, b, x[leg], f[leg], perm[leg], F[leg], i, _getrf_order(A[i]), f"leg {leg}")


# ---------------------------------------------------------------------------------------------
# 8. workgroup shape
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [9, 20, 53, 60, 66])
def test_waves_per_workgroup(gpu, n):
    """The integrator's largest workgroup (br_maxrpb waves, each on its own LDS scratch and slot) against one wave
    per workgroup: N = 2 grids of waves + 5, so every wave takes two matrices, five a third, and the last round is
    ragged; both legs with a changed second matrix. Every output bit for bit, the whole workspace copies included."""
    wpb = R.max_wpb(R.nmax_of(n))
    N = 2 * (2 * wpb) + 5
    J0, g0, b = _lu_inputs(n, N, 12000 + n)
    rng = np.random.default_rng(12100 + n)
    J1 = J0 * (1 + 0.3 * rng.standard_normal(J0.shape))
    one = _wave_lu(J0, g0, b, J1=J1, gamma1=1.7 * g0, dirty=True, wpb=1)
    many = _wave_lu(J0, g0, b, J1=J1, gamma1=1.7 * g0, dirty=True, wpb=wpb)
    assert np.all(one[1] == 0) and np.array_equal(one[1], many[1])
    assert np.array_equal(one[2], many[2])
    assert _same_bits(one[0], many[0])
    assert _same_bits(one[3], many[3])
    A1 = R.newton_matrix(J1, 1.7 * g0)
    for i in range(N):
        assert R.backward_ratio(A1[i], b[i], many[0][1, i]) <= 1e-12, i


# ---------------------------------------------------------------------------------------------
# 9. input rejection
# ---------------------------------------------------------------------------------------------
def test_wave_lu_rejects_bad_input(pkg, gpu):
    """n < 1, n > 72, wpb outside 1..br_maxrpb(nmax) and a perm_in row that is no permutation: BR_ERR_INPUT"""
    L = pkg._lib

    def call(n, wpb, perm_in=None, N=2):
        m = max(n, 1)
        J, v = np.zeros((N, m, m)), np.zeros((N, m))
        x, f, p = np.zeros((2, N, m)), np.zeros((2, N), np.int32), np.zeros((2, N, m), np.int32)
        F = np.zeros((2, N, R.ws_doubles(min(m, 72))))
        return L.lib().br_debug_wave_lu(N, n, wpb, 1, L.dptr(J), None, L.dptr(np.ones(N)), None, L.dptr(v),
                                        L.iptr(perm_in), L.dptr(x), L.iptr(f), L.iptr(p), L.dptr(F))

    assert call(5, 1) == 0
    for n, wpb in ((0, 1), (-3, 1), (73, 1), (9, 0), (9, 5), (20, 5), (53, 17), (64, 17), (66, 13), (9, -1)):
        assert call(n, wpb) == BR_ERR_INPUT, (n, wpb)
    for n, wpb in ((9, 4), (53, 16), (66, 12)):
        assert call(n, wpb) == 0, (n, wpb)
    ok = np.array([[0, 1, 2, 3, 4], [4, 3, 2, 1, 0]], np.int32)
    assert call(5, 1, ok) == 0
    for bad in ([0, 1, 2, 3, 3], [0, 1, 2, 3, 5], [-1, 1, 2, 3, 4]):
        p = ok.copy()
        p[1] = bad
        assert call(5, 1, p) == BR_ERR_INPUT, bad
