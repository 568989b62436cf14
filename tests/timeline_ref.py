"""numpy restatement of the fleet timeline (docs/SEMANTICS.md 7): the rows
ccka_get_timeline returns for a [T][N] array of trajectory records, the checker
of tests/test_gpu_timeline.py. Integers only, so every value is exact."""
from __future__ import annotations

import numpy as np

from sweep_stat_ref import rank

NONE, REPLICAS, PENDING, NODES = 0, 1, 2, 3
SUMS = ("replicas", "pending", "nodes_spot", "nodes_od")
ROW_DTYPE = np.dtype([("grid", "<i8"), ("t0", "<i8"), ("samples", "<i8"), ("sum_replicas", "<i8"),
                      ("sum_pending", "<i8"), ("sum_nodes_spot", "<i8"), ("sum_nodes_od", "<i8"),
                      ("flag_count", "<i8", (8,)), ("max_replicas", "<i4"), ("max_pending", "<i4"),
                      ("max_nodes", "<i4"), ("min_nodes", "<i4"), ("q_value", "<i8")])


def world(profile: str, seed: int):
    """random_worlds.draw(profile, seed) with the batch moved to whole grids:
    the generator draws any first_id, a timeline needs a multiple of every
    grid size in use (here of the batch size, a different one per seed)."""
    import random_worlds as rw
    spec, sc, load = rw.draw(profile, seed)
    sc.first_id = sc.n * (1 + seed)
    return spec, sc, load


def n_rows(n: int, n_steps: int, grid_size: int, step_bucket: int, q_field: int = NONE, q_ppm: int = 0) -> int:
    """ccka_timeline_rows: the row count, or -1 where the call is CCKA_EINVAL."""
    if n < 1 or n_steps < 1 or grid_size < 1 or n % grid_size or step_bucket < 1:
        return -1
    if q_field not in (NONE, REPLICAS, PENDING, NODES) or (q_field != NONE and not 0 <= q_ppm <= 10**6):
        return -1
    if grid_size * min(step_bucket, n_steps) > 1 << 31:
        return -1
    rows = n // grid_size * -(-n_steps // step_bucket)
    return rows if rows <= 1 << 24 else -1


def field(recs: np.ndarray, q_field: int) -> np.ndarray:
    """The field a quantile ranks, as int64."""
    if q_field == NODES:
        return recs["nodes_spot"].astype(np.int64) + recs["nodes_od"].astype(np.int64)
    return recs["replicas" if q_field == REPLICAS else "pending"].astype(np.int64)


def timeline(recs: np.ndarray, grid_size: int, step_bucket: int = 1, q_field: int = NONE, q_ppm: int = 0,
             first_id: int = 0) -> np.ndarray:
    """Rows shaped (n_grids, n_buckets) for records `recs` [T][N]."""
    T, N = recs.shape
    assert n_rows(N, T, grid_size, step_bucket, q_field, q_ppm) >= 0 and first_id % grid_size == 0
    ng, nb = N // grid_size, -(-T // step_bucket)
    out = np.zeros((ng, nb), ROW_DTYPE)
    out["grid"] = (first_id // grid_size + np.arange(ng))[:, None]
    for b in range(nb):  # every grid's row of the bucket at once
        t0, t1 = b * step_bucket, min((b + 1) * step_bucket, T)
        x = recs[t0:t1].reshape(t1 - t0, ng, grid_size)
        o = out[:, b]
        o["t0"], o["samples"] = t0, (t1 - t0) * grid_size
        for f in SUMS:
            o["sum_" + f] = x[f].astype(np.int64).sum(axis=(0, 2))
        for bit in range(8):
            o["flag_count"][:, bit] = ((x["flags"] >> bit) & 1).astype(np.int64).sum(axis=(0, 2))
        nodes = field(x, NODES)
        o["max_replicas"], o["max_pending"] = x["replicas"].max(axis=(0, 2)), x["pending"].max(axis=(0, 2))
        o["max_nodes"], o["min_nodes"] = nodes.max(axis=(0, 2)), nodes.min(axis=(0, 2))
        if q_field != NONE:
            v = np.sort(field(x, q_field).transpose(1, 0, 2).reshape(ng, -1), axis=1)
            o["q_value"] = v[:, rank(v.shape[1], q_ppm) - 1]
    return out
