"""numpy restatement of the sweep statistics (docs/SEMANTICS.md 6): per grid
and objective the sum, the nearest-rank quantile x(k) or the tail sum
x(k) + ... + x(n) of the sorted values, the checker of tests/test_gpu_sweep_stat.py."""
from __future__ import annotations

import numpy as np

FIELDS = ("cost_uphmin", "slo_minutes", "gco2", "energy_wmin")  # ccka_sweep_stat's objective order
SUM, QUANTILE, TAIL = 0, 1, 2


def rank(n: int, q_ppm: int) -> int:
    """Nearest rank k = max(1, ceil(q_ppm * n / 1e6)) in integers."""
    return max(1, (int(q_ppm) * int(n) + 999999) // 1000000)


def _one(x: np.ndarray, kind: int, q_ppm: int):
    if kind == SUM:
        return x.sum()
    xs = np.sort(x)
    k = rank(len(xs), q_ppm)
    xk = xs[k - 1]
    if kind == QUANTILE:
        return xk
    if xs.dtype.kind == "i":
        return xs[k - 1:].sum()  # exact
    gt = xs[xs > xk]
    m = (len(xs) - k + 1) - len(gt)
    return gt.sum() + m * xk


def grid_stat(res, grid_size: int, kinds, q_ppms, first_id: int = 0) -> dict:
    """The rows ccka_get_grid_stat returns for result columns `res` (a mapping
    with FIELDS); kinds / q_ppms: four each, in FIELDS order."""
    n = len(res["cost_uphmin"])
    assert n % grid_size == 0 and first_id % grid_size == 0
    ng = n // grid_size
    out = {
        "grid": np.arange(first_id // grid_size, first_id // grid_size + ng, dtype=np.int64),
        "scenarios": np.full(ng, grid_size, np.int64),
    }
    for f, kind, q in zip(FIELDS, kinds, q_ppms):
        col = np.asarray(res[f])
        col = col.astype(np.int64) if col.dtype.kind == "i" else col.astype(np.float64)
        rows = col.reshape(ng, grid_size)
        out[f] = np.array([_one(r, kind, q) for r in rows], dtype=col.dtype)
    return out
