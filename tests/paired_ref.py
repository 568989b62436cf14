"""Python-int and numpy restatement of the paired comparison (docs/SEMANTICS.md
8): the integer vector of every scenario (util_ref.fix6 for gCO2 and energy),
the per-position deltas of a current grid against a baseline grid, and per
objective their sum, extrema, sign counts and order statistic (a sort;
sweep_stat_ref.rank), with the dominance counts. Every intermediate is an
unbounded Python int: what wraps or overflows does so only where the text says.
The checker of tests/test_paired_ref.py and tests/test_gpu_paired.py."""
from __future__ import annotations

import bisect
import itertools

import numpy as np

from ccka import abi
from sweep_stat_ref import FIELDS, QUANTILE, SUM, TAIL, rank
from util_ref import I64_MAX, I64_MIN, fix6

SAME = abi.PAIRED_SAME
ROW_DTYPE = abi.paired_dtype()
OBJ_FIELDS = ("sum", "min", "max", "q_value", "n_less", "n_greater")
I32_MAX = 0x7FFFFFFF


def wrap(x: int) -> int:
    """x mod 2^64 as a signed int64."""
    return ((int(x) + (1 << 63)) % (1 << 64)) - (1 << 63)


def vectors(cols):
    """([4][n] Python ints, flag): v = (cost, SLO minutes, llrint(gco2 * 1e6),
    llrint(energy * 1e6)) per scenario in FIELDS order; flag: some fix6 flagged."""
    out, ovf = [], False
    for f in FIELDS[:2]:
        out.append([int(v) for v in np.asarray(cols[f]).tolist()])
    for f in FIELDS[2:]:
        fixed = [fix6(v) for v in np.asarray(cols[f], np.float64).tolist()]
        ovf = ovf or any(flag for _, flag in fixed)
        out.append([v for v, _ in fixed])
    return out, ovf


def block(cols, grid_size: int, local_grid: int) -> np.ndarray:
    """The [4][grid_size] int64 block ccka_paired_export returns for that grid."""
    v, ovf = vectors(cols)
    assert not ovf
    lo = local_grid * grid_size
    return np.array([col[lo:lo + grid_size] for col in v], np.int64)


class Prepared:
    """The deltas of every current grid against its baseline grid, sorted once:
    rows() then costs an index per objective."""

    def __init__(self, cur, base, grid_size: int, base_grid: int = SAME, first_grid: int = 0,
                 snap_first_grid: int = 0):
        cv, f1 = vectors(cur)
        bv, f2 = vectors(base)
        n, nb, G = len(cv[0]), len(bv[0]), grid_size
        assert n % G == 0 and nb % G == 0
        self.G, self.ng = G, n // G
        self.ovf = f1 or f2   # an unrepresentable fixed-point value, or a delta outside int64
        self.grid = [first_grid + g for g in range(self.ng)]
        self.base = [first_grid + g if base_grid == SAME else base_grid for g in range(self.ng)]
        self.d, self.srt, self.suffix, self.fixed = [], [], [], None
        for g in range(self.ng):
            b = self.base[g] - snap_first_grid
            assert 0 <= b < nb // G, "baseline grid outside the snapshot"
            per, srt, suf = [], [], []
            for o in range(4):
                d = [cv[o][g * G + j] - bv[o][b * G + j] for j in range(G)]
                self.ovf = self.ovf or min(d) < I64_MIN or max(d) > I64_MAX
                s = sorted(d)
                per.append(d)
                srt.append(s)
                # suffix[i] = s[i] + ... + s[G - 1]
                suf.append(list(itertools.accumulate(reversed(s)))[::-1])
            self.d.append(per)
            self.srt.append(srt)
            self.suffix.append(suf)

    def _fixed(self) -> np.ndarray:
        """The rows without a selection (q_value 0), computed once."""
        G = self.G
        out = np.zeros(self.ng, ROW_DTYPE)
        for g in range(self.ng):
            r = out[g]
            r["grid"], r["base"], r["pairs"] = self.grid[g], self.base[g], G
            d = self.d[g]
            dom = domd = 0
            for three in zip(d[0], d[2], d[1]):  # cost, gCO2, SLO minutes: the frontier's objectives
                dom += max(three) <= 0 and min(three) < 0
                domd += min(three) >= 0 and max(three) > 0
            r["n_dominates"], r["n_dominated"] = dom, domd
            for o in range(4):
                s = self.srt[g][o]
                ob = r["obj"][o]
                ob["sum"] = wrap(sum(s))
                ob["min"], ob["max"] = wrap(s[0]), wrap(s[-1])
                ob["n_less"] = sum(x < 0 for x in s)
                ob["n_greater"] = sum(x > 0 for x in s)
        return out

    def rows(self, kinds=(SUM,) * 4, q_ppms=(0,) * 4) -> np.ndarray:
        """The rows ccka_get_paired returns (meaningful when not self.ovf)."""
        if self.fixed is None:
            self.fixed = self._fixed()
        G = self.G
        out = self.fixed.copy()
        for g in range(self.ng):
            for o in range(4):
                if kinds[o] == SUM:
                    continue
                s = self.srt[g][o]
                k = rank(G, q_ppms[o])
                xk = s[k - 1]
                if kinds[o] == QUANTILE:
                    out[g]["obj"][o]["q_value"] = wrap(xk)
                else:
                    assert kinds[o] == TAIL
                    # sum{d > x(k)} + m x(k) with m = (G - k + 1) - #{d > x(k)}: the ties
                    # are equal terms, so this is x(k) + ... + x(G)
                    first_above = bisect.bisect_right(s, xk)
                    m = (G - k + 1) - (G - first_above)
                    above = self.suffix[g][o][first_above] if first_above < G else 0
                    assert above + m * xk == self.suffix[g][o][k - 1]
                    out[g]["obj"][o]["q_value"] = wrap(above + m * xk)
        return out


def paired(cur, base, grid_size, base_grid=SAME, kinds=(SUM,) * 4, q_ppms=(0,) * 4, first_grid=0,
           snap_first_grid=0):
    """(rows, overflow flag) in one call."""
    p = Prepared(cur, base, grid_size, base_grid, first_grid, snap_first_grid)
    return p.rows(kinds, q_ppms), p.ovf


def equal(got, want, what=""):
    """Every field of every row, exactly."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for f in ("grid", "base", "pairs", "n_dominates", "n_dominated"):
        assert np.array_equal(got[f], want[f]), (what, f, got[f], want[f])
    for f in OBJ_FIELDS:
        bad = np.argwhere(got["obj"][f] != want["obj"][f])
        assert bad.size == 0, f"{what}: obj.{f} differs at (row, objective) {bad[:5].tolist()}: " \
                              f"got {got['obj'][f][tuple(bad[0])]} want {want['obj'][f][tuple(bad[0])]}"
    assert got.tobytes() == want.tobytes(), what


# ---------------------------------------------------------------------------
# adversarial columns
# ---------------------------------------------------------------------------
N_PATTERNS = 6


def _columns(g: int, n_cur_grids: int = 5, n_base_grids: int = 5):
    """(current, baseline) result columns of grids of g positions whose deltas,
    grid i against baseline grid i, stress every digit of the radix select.
    Cost, by grid index mod 6: 0 the extremes +-2^62 with 0 and -1; 1 a constant
    plus a low byte; 2 a high byte plus a constant; 3 every delta 0; 4 uniform in
    [-2^62, 2^62]; 5 every delta one constant (six grids draw them all). The
    baseline costs stay within +-2^40 and baseline grid 0 is all zero, so against
    any baseline grid no subtraction leaves int64. SLO minutes tie heavily; gCO2
    holds m / 128 (products at exact .5: ties to even), +-0.0 and negatives;
    energy holds pairs one ulp apart across the two sides."""
    rng = np.random.default_rng([g, n_cur_grids, n_base_grids])
    nb, nc = n_base_grids, n_cur_grids
    bcost = rng.integers(-(1 << 40), 1 << 40, (nb, g), dtype=np.int64, endpoint=True)
    bcost[0] = 0
    delta = np.zeros((nc, g), np.int64)
    for i in range(nc):
        k = i % N_PATTERNS
        if k == 0:
            delta[i] = np.array([-(1 << 62), 1 << 62, 0, -1], np.int64)[rng.integers(0, 4, g)]
        elif k == 1:
            delta[i] = 0x1234567890ABCD00 + rng.integers(0, 256, g)
        elif k == 2:
            delta[i] = (rng.integers(-64, 64, g).astype(np.int64) << 56) + 0x00FEDCBA98765432
        elif k == 4:
            delta[i] = rng.integers(-(1 << 62), 1 << 62, g, dtype=np.int64, endpoint=True)
        elif k == 5:
            delta[i] = -987654321012345
    cost = delta + bcost[np.arange(nc) % nb]  # |.| <= 2^62 + 2^56 + 2^40: no wrap

    def slo(rows):
        a = np.zeros((rows, g), np.int32)
        u = rng.random((rows, g))
        a[u < 0.1] = I32_MAX
        a[u > 0.9] = rng.integers(-3, 4, int((u > 0.9).sum()))
        return a

    def gco2(rows):
        a = rng.integers(-2000, 2001, (rows, g)) / 128.0
        u = rng.random((rows, g))
        a[u < 0.05] = 0.0
        a[u > 0.95] = -0.0
        return a

    benergy = rng.standard_normal((nb, g)) * 10.0 ** rng.integers(-5, 6, (nb, g))
    energy = benergy[np.arange(nc) % nb].copy()
    energy[:, 1::2] = np.nextafter(energy[:, 1::2], np.inf)   # one ulp above the baseline's
    energy[:, 2::4] = rng.standard_normal(energy[:, 2::4].shape) * 1e3
    cur = {"cost_uphmin": cost.ravel(), "slo_minutes": slo(nc).ravel(), "gco2": gco2(nc).ravel(),
           "energy_wmin": energy.ravel()}
    base = {"cost_uphmin": bcost.ravel(), "slo_minutes": slo(nb).ravel(), "gco2": gco2(nb).ravel(),
            "energy_wmin": benergy.ravel()}
    return cur, base


def counts(rows):
    """{objective: (less, equal, greater)} summed over the rows, and (dominates, dominated)."""
    out = {}
    for o, f in enumerate(("cost", "slo", "gco2", "energy")):
        less, greater = int(rows["obj"]["n_less"][:, o].sum()), int(rows["obj"]["n_greater"][:, o].sum())
        out[f] = (less, int(rows["pairs"].sum()) - less - greater, greater)
    return out, (int(rows["n_dominates"].sum()), int(rows["n_dominated"].sum()))
