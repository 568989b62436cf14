"""Python handle on libccka.so (the HIP rollout engine) through its C ABI.

There is no CPU fallback: constructing an Engine without the built library or
without a GPU raises.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import abi
from .world import TRAJ_DTYPE, ScenarioSet, WorldSpec, alloc_results


GRID_DTYPE = np.dtype([("grid", "<i8"), ("scenarios", "<i8"), ("cost_uphmin", "<i8"),
                       ("slo_minutes", "<i8"), ("gco2", "<f8"), ("energy_wmin", "<f8")])


def _grid_array(a, n) -> np.ndarray:
    return np.frombuffer(bytes(a)[:n * C.sizeof(abi.GridStats)], GRID_DTYPE).copy()


class Engine:
    def __init__(self, device: int = 0, lib_path: str | None = None):
        self.lib = abi.load_engine(lib_path)
        abi.check_sizes(self.lib)
        self.ctx = C.c_void_p()
        abi.check(self.lib.ccka_open(C.byref(self.ctx), device), "ccka_open")
        self.n = 0
        self.T = 0
        self.D = 0

    def _chk(self, rc, what):
        abi.check(rc, what, self.lib, self.ctx)

    def close(self):
        if self.ctx:
            self.lib.ccka_close(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_world(self, spec: WorldSpec):
        w = spec.to_c()
        self._chk(self.lib.ccka_set_world(self.ctx, C.byref(w)), "ccka_set_world")
        self.T = spec.n_steps
        self.D = len(spec.deploys)

    def set_scenarios(self, sc: ScenarioSet):
        s = sc.to_c()
        self._chk(self.lib.ccka_set_scenarios(self.ctx, C.byref(s)), "ccka_set_scenarios")
        self.n = sc.n
        self.load_cols = sc.n_traces if sc.n_traces > 0 else sc.n

    def set_load(self, load: np.ndarray):
        a = np.ascontiguousarray(load, np.int32)
        self._chk(self.lib.ccka_set_load(self.ctx, a.ctypes.data_as(C.POINTER(C.c_int32)), a.size),
                  "ccka_set_load")

    def gen_load(self, gen: abi.TraceGen):
        self._chk(self.lib.ccka_gen_load(self.ctx, C.byref(gen)), "ccka_gen_load")

    def get_load(self) -> np.ndarray:
        a = np.zeros((self.T, self.D, self.load_cols), np.int32)
        self._chk(self.lib.ccka_get_load(self.ctx, a.ctypes.data_as(C.POINTER(C.c_int32)), a.size),
                  "ccka_get_load")
        return a

    def rollout(self, trajectory: bool = False):
        self._chk(self.lib.ccka_rollout(self.ctx, int(trajectory)), "ccka_rollout")

    def rollout_async(self, trajectory: bool = False):
        self._chk(self.lib.ccka_rollout_async(self.ctx, int(trajectory)), "ccka_rollout_async")

    def sync(self):
        self._chk(self.lib.ccka_sync(self.ctx), "ccka_sync")

    def kernel_ms(self) -> float:
        v = C.c_double()
        self._chk(self.lib.ccka_last_kernel_ms(self.ctx, C.byref(v)), "ccka_last_kernel_ms")
        return v.value

    def results(self) -> dict:
        arrays, r = alloc_results(self.n)
        self._chk(self.lib.ccka_get_results(self.ctx, C.byref(r)), "ccka_get_results")
        return arrays

    def trajectory(self) -> np.ndarray:
        a = np.zeros((self.T, self.n), TRAJ_DTYPE)
        self._chk(self.lib.ccka_get_trajectory(self.ctx, a.ctypes.data_as(C.POINTER(abi.TrajRec)),
                                               a.size), "ccka_get_trajectory")
        return a

    def trajectory_native(self):
        """(records, layout): the device records without a transpose, shaped
        [N][T] (abi.TRAJ_NT, the single-deployment engine) or [T][N]."""
        lay = C.c_int32()
        self._chk(self.lib.ccka_trajectory_layout(self.ctx, C.byref(lay)), "ccka_trajectory_layout")
        shape = (self.n, self.T) if lay.value == abi.TRAJ_NT else (self.T, self.n)
        a = np.zeros(shape, TRAJ_DTYPE)
        self._chk(self.lib.ccka_get_trajectory_native(self.ctx, a.ctypes.data_as(C.POINTER(abi.TrajRec)), a.size,
                                                      None), "ccka_get_trajectory_native")
        return a, lay.value

    @staticmethod
    def _grads():
        g = {k: np.zeros(v, np.float32) for k, v in abi.GRAD_SHAPES.items()}
        s = abi.MlpGrads(*[g[k].ctypes.data_as(C.POINTER(C.c_float)) for k in ("w1", "b1", "w2", "b2", "w3", "b3")])
        return g, s

    def policy_grad(self, seed: int, w_carbon: float = 0.0, w_slo: float = 0.0, baseline: bool = True):
        """One stochastic closed-loop rollout and the score-function gradient
        of E[J] (ccka_policy_grad): (grads dict, mean objective)."""
        g, s = self._grads()
        prm = abi.PgParams(seed, w_carbon, w_slo, int(bool(baseline)), 0)
        obj = C.c_double()
        self._chk(self.lib.ccka_policy_grad(self.ctx, C.byref(prm), C.byref(s), C.byref(obj)), "ccka_policy_grad")
        return g, obj.value

    def policy_samples(self):
        """(actions [T][N] uint8, coef [N] fp32) of the last policy_grad."""
        a = np.zeros((self.T, self.n), np.uint8)
        cf = np.zeros(self.n, np.float32)
        self._chk(self.lib.ccka_get_policy_samples(self.ctx, a.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                   cf.ctypes.data_as(C.POINTER(C.c_float)), a.size),
                  "ccka_get_policy_samples")
        return a, cf

    def mlp_backward(self, x_bits: np.ndarray, actions: np.ndarray, coef: np.ndarray):
        """Gradient of sum_m coef[m] log softmax(policy(x_m))[a_m] (ccka_mlp_backward)."""
        x = np.ascontiguousarray(x_bits, np.uint16)
        a = np.ascontiguousarray(actions, np.uint8)
        cf = np.ascontiguousarray(coef, np.float32)
        g, s = self._grads()
        self._chk(self.lib.ccka_mlp_backward(self.ctx, x.ctypes.data_as(C.POINTER(C.c_uint16)),
                                             a.ctypes.data_as(C.POINTER(C.c_uint8)),
                                             cf.ctypes.data_as(C.POINTER(C.c_float)), len(a), C.byref(s)),
                  "ccka_mlp_backward")
        return g

    def totals(self) -> abi.Totals:
        t = abi.Totals()
        self._chk(self.lib.ccka_get_totals(self.ctx, C.byref(t)), "ccka_get_totals")
        return t

    def set_detail(self, on: bool = True):
        """Record the per-pool / base-group / per-deployment breakdown
        (ccka_detail) in later rollouts (the summary path)."""
        self._chk(self.lib.ccka_set_detail(self.ctx, int(bool(on))), "ccka_set_detail")

    def detail(self) -> np.ndarray:
        a = np.zeros(self.n, abi.detail_dtype())
        self._chk(self.lib.ccka_get_detail(self.ctx, a.ctypes.data, a.size), "ccka_get_detail")
        return a

    # ---- closed-loop learned policy (config 5) ----
    def policy_rollout(self, trajectory: bool = False, record: bool = False):
        """ccka_policy_rollout: the MLP policy (mlp_set_weights) decides every
        step's HPA target and carbon weight from the scenario state."""
        self._chk(self.lib.ccka_policy_rollout(self.ctx, int(trajectory), int(record)), "ccka_policy_rollout")

    def policy_actions(self):
        """The recorded actions: (target [T][N] int16, carbon weight [T][N] float64)."""
        tg = np.zeros((self.T, self.n), np.int16)
        cw = np.zeros((self.T, self.n), np.float64)
        self._chk(self.lib.ccka_get_policy_actions(self.ctx, tg.ctypes.data, cw.ctypes.data, tg.size),
                  "ccka_get_policy_actions")
        return tg, cw

    def debug_policy_features(self, enable: bool = True):
        """Internal test hook: record the policy features of every step."""
        fn = self.lib.ccka_debug_policy_features
        fn.argtypes = [C.c_void_p, C.c_int32]
        self._chk(fn(self.ctx, int(enable)), "ccka_debug_policy_features")

    def debug_get_policy_features(self) -> np.ndarray:
        fn = self.lib.ccka_debug_get_policy_features
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        a = np.zeros((self.T + 1, self.n, 64), np.uint16)
        self._chk(fn(self.ctx, a.ctypes.data, a.size), "ccka_debug_get_policy_features")
        return a

    # ---- policy sweep (config 4) ----
    def grid_stats(self, grid_size: int) -> np.ndarray:
        ng = self.n // grid_size
        a = (abi.GridStats * ng)()
        self._chk(self.lib.ccka_get_grid_stats(self.ctx, C.c_int64(grid_size), a, C.c_int64(ng)),
                  "ccka_get_grid_stats")
        return _grid_array(a, ng)

    def grid_stat(self, grid_size: int, stat: abi.SweepStat) -> np.ndarray:
        """Per-grid rows with a chosen statistic per objective (abi.sweep_stat):
        a sum, a quantile or a tail sum in each objective's field."""
        ng = self.n // grid_size
        a = (abi.GridStats * ng)()
        self._chk(self.lib.ccka_get_grid_stat(self.ctx, C.c_int64(grid_size), C.byref(stat), a, C.c_int64(ng)),
                  "ccka_get_grid_stat")
        return _grid_array(a, ng)

    def pareto(self, grid_size: int, capacity: int | None = None, stat: abi.SweepStat | None = None) -> np.ndarray:
        """The cost / gCO2 / SLO frontier of the grids' sums, or with `stat` of
        their chosen statistics (ccka_pareto_frontier_stat)."""
        cap = capacity if capacity is not None else max(1, self.n // grid_size) * 8
        a = (abi.GridStats * cap)()
        n = C.c_int32()
        if stat is None:
            self._chk(self.lib.ccka_pareto_frontier(self.ctx, C.c_int64(grid_size), a, cap, C.byref(n)),
                      "ccka_pareto_frontier")
        else:
            self._chk(self.lib.ccka_pareto_frontier_stat(self.ctx, C.c_int64(grid_size), C.byref(stat), a, cap,
                                                         C.byref(n)), "ccka_pareto_frontier_stat")
        return _grid_array(a, n.value)

    def debug_grid_stat(self, cost, slo, gco2, energy, grid_size: int, stat: abi.SweepStat) -> np.ndarray:
        """Internal: grid_stat's kernel path on given result columns (int64,
        int32, float64, float64; whole grids of grid_size, grid ids from 0)."""
        cols = [np.ascontiguousarray(a, dt) for a, dt in
                ((cost, np.int64), (slo, np.int32), (gco2, np.float64), (energy, np.float64))]
        n = len(cols[0])
        assert all(a.shape == (n,) for a in cols)
        ng = n // max(1, grid_size)
        out = (abi.GridStats * max(1, ng))()
        fn = self.lib.ccka_debug_grid_stat
        fn.argtypes = [C.c_void_p] + [C.c_void_p] * 4 + [C.c_int64, C.c_int64, C.POINTER(abi.SweepStat), C.c_void_p]
        self._chk(fn(self.ctx, *[a.ctypes.data for a in cols], n, grid_size, C.byref(stat), out),
                  "ccka_debug_grid_stat")
        return _grid_array(out, ng)

    # ---- fleet timeline (docs/SEMANTICS.md 7) ----
    def timeline(self, grid_size: int, step_bucket: int = 1, q_field=0, q_ppm: int = 0) -> np.ndarray:
        """The last rollout's trajectory records reduced on the device per grid
        and bucket of step_bucket steps (ccka_get_timeline): a structured array
        (abi.timeline_dtype()) shaped (n_grids, n_buckets). q_field (abi.TL_* or
        its name) adds that field's nearest-rank quantile at q_ppm as q_value."""
        spec = abi.timeline_spec(grid_size, step_bucket, q_field, q_ppm)
        rows = self.lib.ccka_timeline_rows(self.n, self.T, C.byref(spec))
        out = np.zeros(max(rows, 1), abi.timeline_dtype())
        # rows < 0: the call names the rule that fails (or the missing trajectory)
        self._chk(self.lib.ccka_get_timeline(self.ctx, C.byref(spec), out.ctypes.data, max(rows, 0)),
                  "ccka_get_timeline")
        return out[:rows].reshape(self.n // grid_size, -1)

    def debug_timeline(self, recs, layout: int, grid_size: int, step_bucket: int = 1, q_field=0,
                       q_ppm: int = 0) -> np.ndarray:
        """Internal: timeline's kernel path on given records (TRAJ_DTYPE), shaped
        (T, N) for abi.TRAJ_TN or (N, T) for abi.TRAJ_NT; grid ids from 0."""
        a = np.ascontiguousarray(recs, TRAJ_DTYPE)
        assert a.ndim == 2 and layout in (abi.TRAJ_TN, abi.TRAJ_NT)
        n, steps = a.shape if layout == abi.TRAJ_NT else a.shape[::-1]
        spec = abi.timeline_spec(grid_size, step_bucket, q_field, q_ppm)
        rows = self.lib.ccka_timeline_rows(n, steps, C.byref(spec))
        out = np.zeros(max(rows, 1), abi.timeline_dtype())
        fn = self.lib.ccka_debug_timeline
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.POINTER(abi.TimelineSpec),
                       C.c_void_p]
        self._chk(fn(self.ctx, a.ctypes.data, n, steps, layout, C.byref(spec), out.ctypes.data),
                  "ccka_debug_timeline")
        return out[:rows].reshape(n // grid_size, -1)

    # ---- paired comparison (docs/SEMANTICS.md 8) ----
    def paired_capture(self, grid_size: int):
        """Keep the last rollout's batch as the snapshot later paired() calls
        compare against (ccka_paired_capture); it survives new worlds,
        scenarios, traces and rollouts until the next capture or import."""
        self._chk(self.lib.ccka_paired_capture(self.ctx, C.c_int64(grid_size)), "ccka_paired_capture")
        self._paired_gs = grid_size

    def paired(self, grid_size: int, base_grid: int = abi.PAIRED_SAME, stat: abi.SweepStat | None = None) -> np.ndarray:
        """One row (abi.paired_dtype()) per grid of the last rollout: its
        per-position deltas against grid base_grid of the snapshot, or with
        abi.PAIRED_SAME against the snapshot's grid of the same id; stat
        (abi.sweep_stat) adds a quantile or tail sum of the deltas per objective."""
        spec = abi.paired_spec(grid_size, base_grid, stat)
        ng = self.n // grid_size if grid_size > 0 else 0
        out = np.zeros(max(ng, 1), abi.paired_dtype())
        self._chk(self.lib.ccka_get_paired(self.ctx, C.byref(spec), out.ctypes.data, C.c_int64(ng)),
                  "ccka_get_paired")
        return out[:ng]

    def paired_export(self, grid: int) -> np.ndarray:
        """The snapshot's global grid `grid` as an int64 block [4][grid_size]
        (cost, SLO minutes, gCO2 ug, energy uW.min); the size is the last
        capture's or import's grid_size."""
        gs = getattr(self, "_paired_gs", 0)
        out = np.zeros((4, max(gs, 1)), np.int64)
        self._chk(self.lib.ccka_paired_export(self.ctx, C.c_int64(grid), out.ctypes.data, C.c_int64(4 * gs)),
                  "ccka_paired_export")
        return out

    def paired_import(self, grid_size: int, n_traces: int, grid: int, block: np.ndarray):
        """A one-grid snapshot (global grid id `grid`) from a paired_export block."""
        a = np.ascontiguousarray(block, np.int64)
        self._chk(self.lib.ccka_paired_import(self.ctx, C.c_int64(grid_size), C.c_int64(n_traces), C.c_int64(grid),
                                              a.ctypes.data, C.c_int64(a.size)), "ccka_paired_import")
        self._paired_gs = grid_size

    PAIRED_COLUMNS = (("cost_uphmin", np.int64), ("slo_minutes", np.int32), ("gco2", np.float64),
                      ("energy_wmin", np.float64))

    def debug_paired(self, cur, base, grid_size: int, base_grid: int = abi.PAIRED_SAME,
                     stat: abi.SweepStat | None = None) -> np.ndarray:
        """Internal: paired()'s two kernels on given result columns (mappings
        with PAIRED_COLUMNS; whole grids of grid_size, grid ids from 0 on both
        sides); the context's snapshot stays."""
        a = [np.ascontiguousarray(cur[k], dt) for k, dt in self.PAIRED_COLUMNS]
        b = [np.ascontiguousarray(base[k], dt) for k, dt in self.PAIRED_COLUMNS]
        n, nb = len(a[0]), len(b[0])
        assert all(x.shape == (n,) for x in a) and all(x.shape == (nb,) for x in b)
        spec = abi.paired_spec(grid_size, base_grid, stat)
        ng = n // max(1, grid_size)
        out = np.zeros(max(ng, 1), abi.paired_dtype())
        fn = self.lib.ccka_debug_paired
        fn.argtypes = [C.c_void_p] + [C.c_void_p] * 4 + [C.c_int64] + [C.c_void_p] * 4 + [C.c_int64,
                       C.POINTER(abi.PairedSpec), C.c_void_p]
        self._chk(fn(self.ctx, *[x.ctypes.data for x in a], n, *[x.ctypes.data for x in b], nb, C.byref(spec),
                     out.ctypes.data), "ccka_debug_paired")
        return out[:ng]

    # ---- paired bootstrap (docs/SEMANTICS.md 9) ----
    def paired_bootstrap(self, grid_size: int, base_grid: int = abi.PAIRED_SAME, replicates: int = 1000,
                         seed: int = 0, lo_ppm: int = 25000, hi_ppm: int = 975000) -> np.ndarray:
        """One row (abi.boot_dtype()) per grid of the last rollout: the paired
        bootstrap of its per-position deltas against the snapshot (baseline as
        paired()): the observed sums and, of `replicates` resampled sums per
        objective, the lo_ppm and hi_ppm quantiles and the sign and dominance
        counts (ccka_get_paired_bootstrap)."""
        spec = abi.boot_spec(grid_size, base_grid, replicates, seed, lo_ppm, hi_ppm)
        ng = self.n // grid_size if grid_size > 0 else 0
        out = np.zeros(max(ng, 1), abi.boot_dtype())
        self._chk(self.lib.ccka_get_paired_bootstrap(self.ctx, C.byref(spec), out.ctypes.data, C.c_int64(ng)),
                  "ccka_get_paired_bootstrap")
        return out[:ng]

    def debug_boot(self, cur, base, grid_size: int, base_grid: int = abi.PAIRED_SAME, replicates: int = 1000,
                   seed: int = 0, lo_ppm: int = 25000, hi_ppm: int = 975000) -> np.ndarray:
        """Internal: paired_bootstrap()'s kernels on given result columns, as
        debug_paired(); the context's snapshot stays."""
        a = [np.ascontiguousarray(cur[k], dt) for k, dt in self.PAIRED_COLUMNS]
        b = [np.ascontiguousarray(base[k], dt) for k, dt in self.PAIRED_COLUMNS]
        n, nb = len(a[0]), len(b[0])
        assert all(x.shape == (n,) for x in a) and all(x.shape == (nb,) for x in b)
        spec = abi.boot_spec(grid_size, base_grid, replicates, seed, lo_ppm, hi_ppm)
        ng = n // max(1, grid_size)
        out = np.zeros(max(ng, 1), abi.boot_dtype())
        fn = self.lib.ccka_debug_boot
        fn.argtypes = [C.c_void_p] + [C.c_void_p] * 4 + [C.c_int64] + [C.c_void_p] * 4 + [C.c_int64,
                       C.POINTER(abi.BootSpec), C.c_void_p]
        self._chk(fn(self.ctx, *[x.ctypes.data for x in a], n, *[x.ctypes.data for x in b], nb, C.byref(spec),
                     out.ctypes.data), "ccka_debug_boot")
        return out[:ng]

    def debug_boot_workspace(self, max_sums: int):
        """Internal: bound the replicate sums a bootstrap pass holds (0: the
        default); the rows do not depend on it."""
        fn = self.lib.ccka_debug_boot_workspace
        fn.argtypes = [C.c_void_p, C.c_int64]
        self._chk(fn(self.ctx, max_sums), "ccka_debug_boot_workspace")

    def debug_boot_limits(self):
        """Internal: (delta staging limit in positions per grid, grid-tile width) of the build."""
        fn = self.lib.ccka_debug_boot_limits
        fn.argtypes = [C.POINTER(C.c_int64)]
        out = (C.c_int64 * 2)()
        self._chk(fn(out), "ccka_debug_boot_limits")
        return int(out[0]), int(out[1])

    def debug_boot_ms(self, spec: abi.BootSpec, reps: int = 5, tile: int = 0, stage: int = -1):
        """Internal: device ms of (boot_delta_kernel, boot_sums_kernel,
        boot_select_kernel), each alone, for the last rollout against the
        snapshot; tile / stage select another grid-tile width / staging limit
        (0 / -1: the build's; stage 0: no LDS staging)."""
        fn = self.lib.ccka_debug_boot_ms
        fn.argtypes = [C.c_void_p, C.POINTER(abi.BootSpec), C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_double)]
        ms = (C.c_double * 3)()
        self._chk(fn(self.ctx, C.byref(spec), reps, tile, stage, ms), "ccka_debug_boot_ms")
        return tuple(ms)

    TOTALS_COLUMNS = (("cost_uphmin", np.int64), ("slo_minutes", np.int32), ("pending_pod_minutes", np.int64),
                      ("node_min_spot", np.int32), ("node_min_od", np.int32), ("launches", np.int32),
                      ("deletions", np.int32), ("energy_wmin", np.float64), ("gco2", np.float64))

    def debug_totals(self, cols: dict) -> abi.Totals:
        """Internal: ccka_get_totals' reduction on given result columns (a
        mapping with TOTALS_COLUMNS); raises CckaError on CCKA_EOVERFLOW."""
        a = [np.ascontiguousarray(cols[k], dt) for k, dt in self.TOTALS_COLUMNS]
        n = len(a[0])
        assert all(x.shape == (n,) for x in a)
        fn = self.lib.ccka_debug_totals
        fn.argtypes = [C.c_void_p] + [C.c_void_p] * 9 + [C.c_int64, C.POINTER(abi.Totals)]
        t = abi.Totals()
        self._chk(fn(self.ctx, *[x.ctypes.data for x in a], n, C.byref(t)), "ccka_debug_totals")
        return t

    def debug_traj_stage(self, records: int = 0):
        """Internal: staging capacity in records of trajectory()'s device
        transpose (0 = the default 4 Mi)."""
        fn = self.lib.ccka_debug_traj_stage
        fn.argtypes = [C.c_void_p, C.c_int64]
        self._chk(fn(self.ctx, records), "ccka_debug_traj_stage")

    def debug_trace_layout(self, trace: np.ndarray, dp: int = 0, lpw: int = 0, sentinel: int = 0x5EA7BEEF) -> np.ndarray:
        """Internal: the skewed schedule's [NL][T][DP] copy (dp > 0) or the
        single-deployment kernel's wave-tiled copy (dp == 0, lanes per wave
        lpw, D == 1) of a [T][D][NL] int32 trace: the whole output buffer,
        flat, filled with `sentinel` before the kernel ran."""
        a = np.ascontiguousarray(trace, np.int32)
        T, D, NL = a.shape
        cnt = NL * T * dp if dp else T * ((NL + lpw - 1) // max(1, lpw) * lpw)
        out = np.zeros(cnt, np.int32)
        fn = self.lib.ccka_debug_trace_layout
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                       C.c_void_p, C.c_int64]
        self._chk(fn(self.ctx, a.ctypes.data, T, D, NL, dp, lpw, sentinel, out.ctypes.data, cnt),
                  "ccka_debug_trace_layout")
        return out

    # ---- multi-GPU (RCCL over xGMI) ----
    def comm_init(self, uid: bytes | None = None, nranks: int = 1, rank: int = 0):
        """RCCL communicator of this context; uid = None creates a fresh id
        (one-rank communicator, or rank 0 before distributing it)."""
        buf = (C.c_uint8 * 128)()
        if uid is None:
            self._chk(self.lib.ccka_comm_unique_id(buf), "ccka_comm_unique_id")
        else:
            buf = (C.c_uint8 * 128).from_buffer_copy(uid)
        self._chk(self.lib.ccka_comm_init(self.ctx, buf, nranks, rank), "ccka_comm_init")

    def comm_info(self):
        n, r = C.c_int32(), C.c_int32()
        self._chk(self.lib.ccka_comm_info(self.ctx, C.byref(n), C.byref(r)), "ccka_comm_info")
        return n.value, r.value

    def allreduce_totals(self, t: abi.Totals) -> abi.Totals:
        out = abi.Totals.from_buffer_copy(t)
        self._chk(self.lib.ccka_allreduce_totals(self.ctx, C.byref(out)), "ccka_allreduce_totals")
        return out

    def debug_pareto_merge(self, gathered: np.ndarray, counts, capacity: int | None = None) -> np.ndarray:
        """Internal: the cross-rank merge of ccka_pareto_frontier on given
        exchange buffers (gathered: GRID_DTYPE [nranks][cap])."""
        g = np.ascontiguousarray(gathered, GRID_DTYPE)
        nranks, cap = g.shape
        cnt = np.ascontiguousarray(counts, np.int64)
        assert cnt.shape == (nranks,)
        outcap = capacity if capacity is not None else nranks * cap
        a = (abi.GridStats * outcap)()
        n = C.c_int32()
        fn = self.lib.ccka_debug_pareto_merge
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_int32,
                       C.POINTER(C.c_int32)]
        self._chk(fn(self.ctx, g.ctypes.data, cnt.ctypes.data, nranks, cap, a, outcap, C.byref(n)),
                  "ccka_debug_pareto_merge")
        return _grid_array(a, n.value)

    # ---- learned MLP policy (config 5) ----
    def mlp_set_weights(self, ws, bs):
        """ws: bf16 bit arrays (uint16) [in][out]; bs: float32 biases."""
        w = [np.ascontiguousarray(x, np.uint16) for x in ws]
        b = [np.ascontiguousarray(x, np.float32) for x in bs]
        u16 = C.POINTER(C.c_uint16)
        f32 = C.POINTER(C.c_float)
        self._chk(self.lib.ccka_mlp_set_weights(
            self.ctx, w[0].shape[0], w[0].shape[1], w[2].shape[1],
            w[0].ctypes.data_as(u16), b[0].ctypes.data_as(f32), w[1].ctypes.data_as(u16),
            b[1].ctypes.data_as(f32), w[2].ctypes.data_as(u16), b[2].ctypes.data_as(f32)),
            "ccka_mlp_set_weights")
        self.mlp_out = w[2].shape[1]

    def mlp_set_states(self, x: np.ndarray):
        a = np.ascontiguousarray(x, np.uint16)
        self._chk(self.lib.ccka_mlp_set_states(self.ctx, a.ctypes.data_as(C.POINTER(C.c_uint16)),
                                               C.c_int64(a.shape[0])), "ccka_mlp_set_states")
        self.mlp_n = a.shape[0]

    def mlp_gen_states(self, n: int, seed: int = 7):
        self._chk(self.lib.ccka_mlp_gen_states(self.ctx, C.c_int64(n), C.c_uint64(seed)),
                  "ccka_mlp_gen_states")
        self.mlp_n = n

    def mlp_forward(self):
        self._chk(self.lib.ccka_mlp_forward(self.ctx), "ccka_mlp_forward")

    def mlp_forward_async(self):
        self._chk(self.lib.ccka_mlp_forward_async(self.ctx), "ccka_mlp_forward_async")

    def mlp_actions(self) -> np.ndarray:
        y = np.zeros((self.mlp_n, getattr(self, "mlp_out", 8)), np.float32)
        self._chk(self.lib.ccka_mlp_get_actions(self.ctx, y.ctypes.data_as(C.POINTER(C.c_float)),
                                                C.c_int64(self.mlp_n)), "ccka_mlp_get_actions")
        return y

    def set_engine(self, mode: int):
        """Internal: 0 = automatic engine choice, 1 = general kernel only, 2 = the
        general kernel in lockstep (no lane-skewed schedule for several deployments)."""
        self.lib.ccka_debug_engine.argtypes = [C.c_void_p, C.c_int32]
        self._chk(self.lib.ccka_debug_engine(self.ctx, mode), "ccka_debug_engine")

    def last_engine(self):
        """Internal: (engine, table_ms) of the last rollout; engine 1 = general
        kernel, 2 = single-deployment kernel (rollout_d1.hip), 3 / 4 = the
        launched / fused closed loop, 5 = the general kernel on the lane-skewed
        schedule (rollout_sk.hip)."""
        e, ms = C.c_int32(), C.c_double()
        self._chk(self.lib.ccka_debug_last_engine(self.ctx, C.byref(e), C.byref(ms)),
                  "ccka_debug_last_engine")
        return e.value, ms.value

    PLAN_FIELDS = ("grid", "span", "all_hours", "hlen", "lds", "lclaims", "trace_mod",
                   "lds_tab", "nw", "nzi", "jt", "inst")

    def last_plan(self) -> dict:
        """Internal: the launch plan of the last rollout (ccka_debug_last_plan):
        workgroups, the general kernel's span / all_hours / hlen, dynamic LDS
        bytes, lane-local provisioning, shared traces, and the single-deployment
        kernel's lds_tab, NW, NZI, JT and instantiation (slots * 100 + pools);
        -1 where a field does not apply to the engine that ran."""
        fn = self.lib.ccka_debug_last_plan
        fn.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        out = (C.c_int32 * 12)()
        self._chk(fn(self.ctx, out), "ccka_debug_last_plan")
        return dict(zip(self.PLAN_FIELDS, out))

    def device_info(self):
        name = C.create_string_buffer(256)
        cus = C.c_int32()
        self._chk(self.lib.ccka_device_info(self.ctx, name, 256, C.byref(cus)), "ccka_device_info")
        return name.value.decode(), cus.value
