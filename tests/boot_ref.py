"""Restatement of the paired bootstrap (docs/SEMANTICS.md 9) for
tests/test_boot_ref.py and tests/test_gpu_boot.py. The resampling indices come
from util_ref.philox, the deltas from paired_ref.Prepared (Python ints), the
ranks from sweep_stat_ref.rank. A replicate sum is the Python int
sum_j count[r][j] * d[j], wrapped with paired_ref.wrap; the products over the
positions are taken in numpy on the two 32-bit halves of every delta, which is
exact while n < 2^31 (every partial sum stays below 2^63), and joined as
Python ints. equal() compares every field, then the bytes."""
from __future__ import annotations

import numpy as np

import paired_ref
from ccka import abi
from paired_ref import SAME, wrap
from sweep_stat_ref import rank
from util_ref import I64_MAX, philox

ROW_DTYPE = abi.boot_dtype()
OBJ_FIELDS = ("sum", "lo", "hi", "n_less", "n_greater")
TAG = 0xB0075EED   # counter word 3 of every resampling call
M32 = (1 << 32) - 1


def words(n: int, B: int, seed: int) -> np.ndarray:
    """w(r, i) as uint64 [B][n]: W = philox(i div 4, r, 0, TAG; seed lo, seed hi), w = W[i mod 4]."""
    assert 1 <= n <= 1 << 31 and B >= 1
    calls = (n + 3) // 4
    c0 = np.arange(calls, dtype=np.uint64)[None, :]
    c1 = np.arange(B, dtype=np.uint64)[:, None]
    W = philox(c0, c1, 0, TAG, seed & M32, (seed >> 32) & M32)            # four [B][calls]
    return np.stack([np.broadcast_to(x, (B, calls)) for x in W], axis=2).reshape(B, 4 * calls)[:, :n]


def indices(n: int, B: int, seed: int) -> np.ndarray:
    """j(r, i) = (w(r, i) n) div 2^32 as int64 [B][n]."""
    return ((words(n, B, seed) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)   # w n < 2^63


def counts(n: int, B: int, seed: int) -> np.ndarray:
    """count[r][j] = how often replicate r draws position j, int64 [B][n]."""
    idx = indices(n, B, seed)
    out = np.zeros((B, n), np.int64)
    np.add.at(out, (np.arange(B)[:, None], idx), 1)
    return out


def replicate_sums(d, cnt: np.ndarray, wrapped: bool = True):
    """[B] Python ints: S[r] = sum_j cnt[r][j] d[j] for int64-range Python ints d."""
    a = np.array([int(x) & M32 for x in d], np.int64)          # low halves, 0 .. 2^32 - 1
    b = np.array([int(x) >> 32 for x in d], np.int64)          # high halves, signed
    lo, hi = (cnt @ a).tolist(), (cnt @ b).tolist()
    return [wrap((h << 32) + l) if wrapped else (h << 32) + l for h, l in zip(hi, lo)]


class Boot:
    """The bootstrap rows of every current grid against its baseline grid."""

    def __init__(self, cur, base, grid_size: int, base_grid: int = SAME, first_grid: int = 0,
                 snap_first_grid: int = 0):
        self.p = paired_ref.Prepared(cur, base, grid_size, base_grid, first_grid, snap_first_grid)
        self.ovf = self.p.ovf
        self._sums = {}

    def sums(self, B: int, seed: int):
        """S[grid][objective][r] as wrapped Python ints (meaningful when not self.ovf)."""
        key = (B, seed)
        if key not in self._sums:
            cnt = counts(self.p.G, B, seed)
            self._sums[key] = [[replicate_sums(d, cnt) for d in per] for per in self.p.d]
        return self._sums[key]

    def rows(self, B: int = 1000, seed: int = 0, lo_ppm: int = 25000, hi_ppm: int = 975000) -> np.ndarray:
        p = self.p
        S = self.sums(B, seed)
        k_lo, k_hi = rank(B, lo_ppm), rank(B, hi_ppm)
        out = np.zeros(p.ng, ROW_DTYPE)
        for g in range(p.ng):
            r = out[g]
            r["grid"], r["base"], r["pairs"], r["replicates"] = p.grid[g], p.base[g], p.G, B
            dom = domd = 0
            for three in zip(S[g][0], S[g][2], S[g][1]):   # cost, gCO2, SLO minutes
                dom += max(three) <= 0 and min(three) < 0
                domd += min(three) >= 0 and max(three) > 0
            r["n_dominates"], r["n_dominated"] = dom, domd
            for o in range(4):
                s = sorted(S[g][o])
                ob = r["obj"][o]
                ob["sum"] = wrap(sum(p.d[g][o]))
                ob["lo"], ob["hi"] = s[k_lo - 1], s[k_hi - 1]
                ob["n_less"] = sum(x < 0 for x in s)
                ob["n_greater"] = sum(x > 0 for x in s)
        return out


def equal(got, want, what=""):
    """Every field of every row, exactly; then the bytes."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for f in ("grid", "base", "pairs", "replicates", "n_dominates", "n_dominated"):
        assert np.array_equal(got[f], want[f]), (what, f, got[f], want[f])
    for f in OBJ_FIELDS:
        bad = np.argwhere(got["obj"][f] != want["obj"][f])
        assert bad.size == 0, f"{what}: obj.{f} differs at (row, objective) {bad[:5].tolist()}: " \
                              f"got {got['obj'][f][tuple(bad[0])]} want {want['obj'][f][tuple(bad[0])]}"
    assert got.tobytes() == want.tobytes(), what


def scaled_columns(g: int, n_cur_grids: int = 6, n_base_grids: int = 6):
    """paired_ref._columns with the cost deltas against the same-index baseline
    grid and the baseline costs both shifted right by s bits, 2^s > 2 g: the
    patterns keep their shape (0 stays 0, a constant stays one), and against
    any baseline grid |d| < 2^63 / 2^s < 2^62 / g, so no replicate sum wraps
    (g max|d| <= INT64_MAX). The other objectives' deltas are far smaller."""
    cur, base = paired_ref._columns(g, n_cur_grids, n_base_grids)
    s = int(g).bit_length() + 1
    bcost = base["cost_uphmin"].reshape(n_base_grids, g)
    delta = cur["cost_uphmin"].reshape(n_cur_grids, g) - bcost[np.arange(n_cur_grids) % n_base_grids]
    cur, base = dict(cur), dict(base)
    base["cost_uphmin"] = (bcost >> s).ravel()
    cur["cost_uphmin"] = ((delta >> s) + (bcost >> s)[np.arange(n_cur_grids) % n_base_grids]).ravel()
    return cur, base


def no_wrap(rows) -> bool:
    """The sufficient condition of the text on ccka_get_paired rows: pairs * max(|min|, |max|) <= INT64_MAX."""
    m = np.maximum(np.abs(rows["obj"]["min"].astype(object)), np.abs(rows["obj"]["max"].astype(object)))
    return bool((m * rows["pairs"].astype(object)[:, None] <= I64_MAX).all())
