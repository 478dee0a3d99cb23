"""Prescribed temperature programmes T(t) (br_opts.ntprog, include/brhip.h): piecewise-linear knots
(t_j, T_j), t_0 = 0, T held at the last knot's value beyond it. One TemperatureProgram is one row of the
table the integrate calls take; `table` stacks several (ragged rows padded with NaN times)."""
import numpy as np


class TemperatureProgram:
    def __init__(self, t, T):
        t = np.array(t, dtype=np.float64).ravel()
        T = np.array(T, dtype=np.float64).ravel()
        if t.shape != T.shape or t.size < 1:
            raise ValueError(f"tprog: t and T must be 1-D and of equal length >= 1, got {t.shape} and {T.shape}")
        k = np.isnan(t)
        nk = int(t.size - k.sum())
        if k[:nk].any() or nk < 1:
            raise ValueError("tprog: a NaN knot time is trailing padding only")
        t, T = t[:nk], T[:nk]
        if t[0] != 0.0:
            raise ValueError(f"tprog: the first knot time must be 0, got {t[0]}")
        if np.any(np.diff(t) < 0) or not np.all(np.isfinite(t)):
            raise ValueError("tprog: knot times must be finite and ascending")
        if not np.all(np.isfinite(T)) or np.any(T <= 0):
            raise ValueError("tprog: temperatures must be finite and > 0")
        self.t, self.T = t, T

    @classmethod
    def from_knots(cls, t, T):
        """the programme through the knots (t_j, T_j): t ascending, t[0] == 0, T in K"""
        return cls(t, T)

    @classmethod
    def ramp(cls, T0, rate, Tmax):
        """T0 at t = 0, then `rate` K/s (negative: cooling) until Tmax is reached, held there"""
        if rate == 0 or T0 == Tmax:
            return cls([0.0], [T0])
        if (Tmax - T0) / rate < 0:
            raise ValueError(f"tprog: a ramp of {rate} K/s from {T0} K never reaches {Tmax} K")
        return cls([0.0, (Tmax - T0) / rate], [T0, Tmax])

    @classmethod
    def constant(cls, T):
        return cls([0.0], [T])

    def __call__(self, t):
        """T(t), the header's formula operation for operation:
        T_j + (t - t_j) * ((T_{j+1} - T_j) / (t_{j+1} - t_j)) for t_j <= t < t_{j+1}, T of the last knot at
        and beyond it. t: scalar or array, >= 0."""
        return evaluate(self.t, self.T, t)

    def __len__(self):
        return self.t.size


def evaluate(kt, kT, t):
    """T(t) of one row of knots (NaN times = trailing padding), in numpy, with the header's formula"""
    kt, kT = np.asarray(kt, np.float64), np.asarray(kT, np.float64)
    nk = int(np.count_nonzero(~np.isnan(kt)))
    kt, kT = kt[:nk], kT[:nk]
    tt = np.asarray(t, dtype=np.float64)
    # the segment: the last knot at or before t (of equal knot times, a jump, the last one)
    j = np.clip(np.searchsorted(kt, tt, side="right") - 1, 0, nk - 1)
    j1 = np.minimum(j + 1, nk - 1)
    last = j1 == j
    with np.errstate(invalid="ignore", divide="ignore"):
        slope = (kT[j1] - kT[j]) / (kt[j1] - kt[j])
        out = np.where(last, kT[j], kT[j] + (tt - kt[j]) * slope)
    return out if out.ndim else float(out)


def table(tprog, tprog_row, N):
    """The tprog / tprog_row arguments of the integrate calls as C arrays: (t [nrows, nk], T [nrows, nk],
    rows [N] int32 or None). tprog: one TemperatureProgram (shared by all N reactors), a sequence of them
    (one per reactor, or the rows tprog_row [N] points into), or a pair (t, T) of [nrows, nk] arrays
    (handed to the library as they are, NaN-padded). Shapes are checked here (ValueError, before the
    library is called); the knots by the library, which names the first bad reactor."""
    if tprog is None:
        if tprog_row is not None:
            raise ValueError("tprog_row without tprog")
        return None, None, None
    if isinstance(tprog, TemperatureProgram):
        if tprog_row is not None:
            raise ValueError("tprog_row with a single tprog: pass a sequence of programmes")
        tprog, tprog_row = [tprog], np.zeros(N, np.int32)
    if isinstance(tprog, tuple) and len(tprog) == 2 and not isinstance(tprog[0], TemperatureProgram):
        kt = np.ascontiguousarray(np.atleast_2d(tprog[0]), dtype=np.float64)
        kT = np.ascontiguousarray(np.atleast_2d(tprog[1]), dtype=np.float64)
        if kt.ndim != 2 or kt.shape != kT.shape or kt.shape[0] < 1 or kt.shape[1] < 1:
            raise ValueError(f"tprog: (t, T) must be two [nrows, nk] arrays, got {kt.shape} and {kT.shape}")
    else:
        progs = list(tprog)
        if not progs or not all(isinstance(p, TemperatureProgram) for p in progs):
            raise ValueError("tprog: a TemperatureProgram, a sequence of them, or a pair (t, T) of arrays")
        nk = max(len(p) for p in progs)
        kt = np.full((len(progs), nk), np.nan)
        kT = np.full((len(progs), nk), np.nan)
        for r, p in enumerate(progs):
            kt[r, :len(p)], kT[r, :len(p)] = p.t, p.T
    if tprog_row is None:
        if kt.shape[0] != N:
            raise ValueError(f"tprog has {kt.shape[0]} rows for N = {N} reactors: pass tprog_row, or one row per reactor")
        return kt, kT, None
    rows = np.asarray(tprog_row)
    if rows.shape != (N,) or not np.issubdtype(rows.dtype, np.integer):
        raise ValueError(f"tprog_row must be {N} integers, got shape {rows.shape} of {rows.dtype}")
    return kt, kT, np.ascontiguousarray(rows, dtype=np.int32)
