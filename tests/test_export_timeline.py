"""Fleet timeline export (ccka_host_export_timeline): the rows of a timeline as
Prometheus text exposition or CSV. Host code only: the rows here are the numpy
restatement's (tests/timeline_ref.py) over an oracle trajectory, which the GPU
rows equal field for field (tests/test_gpu_timeline.py)."""
import ctypes as C

import numpy as np
import pytest

import pyoracle as po
import timeline_ref as ref
from ccka import abi, configs
from ccka.host import EXPORT_CSV, EXPORT_PROMETHEUS, Host
from test_export import T0, parse, series

G, B, FIRST = 12, 45, 36
EVENTS = ("launch", "deletion", "slo_violation", "drift_deletion", "replacement_launch", "multi_consolidation")


@pytest.fixture(scope="module")
def run():
    spec = configs.config2_world(n_steps=200)
    spec.start_minute = 1400  # the day wraps inside the horizon
    sc = configs.hpa_scenarios(24)
    load = po.gen_load(configs.trace_gen(), spec.n_steps, 1, sc.n)
    _, tr = po.rollout(spec, sc, load, traj=True, threads=2)
    tr = tr.copy()
    tr["flags"][::7, ::5] |= 0x70 | 0x80 | 0x100  # bits 4..8 occur too
    tr["replicas"][3, 2] = -5                      # a signed value survives the text
    return spec, tr


def test_prometheus_values_are_the_row_fields(run):
    spec, tr = run
    sp = abi.timeline_spec(G, B, "nodes", 950000)
    rows = ref.timeline(tr, G, B, ref.NODES, 950000, first_id=FIRST)
    fam, s = parse(Host().export_timeline(spec.to_c(), sp, rows, EXPORT_PROMETHEUS, start_unix_ms=T0))
    assert set(fam.values()) == {"gauge"}
    assert set(fam) == {"ccka_fleet_samples", "ccka_fleet_replicas_sum", "ccka_fleet_pending_sum",
                        "ccka_fleet_nodes_sum", "ccka_fleet_replicas_max", "ccka_fleet_pending_max",
                        "ccka_fleet_nodes_max", "ccka_fleet_nodes_min", "ccka_fleet_step_events",
                        "ccka_fleet_policy_peak_samples", "ccka_fleet_quantile"}
    assert rows.shape == (2, 5) and rows["grid"][:, 0].tolist() == [3, 4]
    assert rows["sum_replicas"].min() < rows["sum_replicas"].max() and (rows["flag_count"][..., 7] > 0).any()
    for g in range(rows.shape[0]):
        r = rows[g]
        ts = [T0 + 60_000 * int(t) for t in r["t0"]]
        gid = int(r["grid"][0])

        def col(name, **lab):
            got = series(s, name, grid=gid, **lab)
            assert sorted(got) == ts, name  # one sample per bucket, at its first step
            return [int(got[x]) for x in ts]

        assert col("ccka_fleet_samples") == r["samples"].tolist()
        assert col("ccka_fleet_replicas_sum") == r["sum_replicas"].tolist()
        assert col("ccka_fleet_pending_sum") == r["sum_pending"].tolist()
        assert col("ccka_fleet_nodes_sum", capacity_type="spot") == r["sum_nodes_spot"].tolist()
        assert col("ccka_fleet_nodes_sum", capacity_type="on-demand") == r["sum_nodes_od"].tolist()
        assert col("ccka_fleet_replicas_max") == r["max_replicas"].tolist()
        assert col("ccka_fleet_pending_max") == r["max_pending"].tolist()
        assert col("ccka_fleet_nodes_max") == r["max_nodes"].tolist()
        assert col("ccka_fleet_nodes_min") == r["min_nodes"].tolist()
        for bit, ev in enumerate(EVENTS, start=1):
            assert col("ccka_fleet_step_events", event=ev) == r["flag_count"][:, bit].tolist(), ev
        assert col("ccka_fleet_policy_peak_samples") == r["flag_count"][:, 0].tolist()
        assert col("ccka_fleet_quantile", field="nodes", q_ppm=950000) == r["q_value"].tolist()
    # nothing else: every family has rows x its label values samples
    assert len(s) == rows.size * (10 + 1 + 6)


def test_quantile_series_only_when_asked(run):
    spec, tr = run
    h = Host()
    rows = ref.timeline(tr, G, B)
    fam, s = parse(h.export_timeline(spec.to_c(), abi.timeline_spec(G, B), rows))
    assert "ccka_fleet_quantile" not in fam and "ccka_fleet_samples" in fam
    assert min(k[2] for k in s) == 0  # start_unix_ms defaults to 0
    rows = ref.timeline(tr, G, B, ref.REPLICAS, 0)
    _, s = parse(h.export_timeline(spec.to_c(), abi.timeline_spec(G, B, "replicas", 0), rows))
    q = series(s, "ccka_fleet_quantile", grid=0, field="replicas", q_ppm=0)
    assert [int(q[t]) for t in sorted(q)] == rows["q_value"][0].tolist() and -5 in rows["q_value"][0]


def test_csv_rows(run):
    spec, tr = run
    rows = ref.timeline(tr, G, B, ref.PENDING, 500000, first_id=FIRST)
    txt = Host().export_timeline(spec.to_c(), abi.timeline_spec(G, B, "pending", 500000), rows, EXPORT_CSV)
    lines = txt.strip().split("\n")
    assert lines[0] == ("grid,t0,minute,samples,sum_replicas,sum_pending,sum_nodes_spot,sum_nodes_od,max_replicas,"
                        "max_pending,max_nodes,min_nodes,count_bit0,count_bit1,count_bit2,count_bit3,count_bit4,"
                        "count_bit5,count_bit6,count_bit7,q_value")
    assert len(lines) == 1 + rows.size
    for ln, r in zip(lines[1:], rows.ravel()):  # grid-major, as the rows
        v = [int(x) for x in ln.split(",")]
        assert v[:2] == [r["grid"], r["t0"]] and v[2] == (1400 + int(r["t0"])) % 1440
        assert v[3:8] == [r["samples"], r["sum_replicas"], r["sum_pending"], r["sum_nodes_spot"], r["sum_nodes_od"]]
        assert v[8:12] == [r["max_replicas"], r["max_pending"], r["max_nodes"], r["min_nodes"]]
        assert v[12:20] == r["flag_count"].tolist() and v[20] == r["q_value"]
    assert {int(ln.split(",")[2]) for ln in lines[1:]} == {1400, 5, 50, 95, 140}


def test_buffer_protocol_and_errors(run):
    spec, tr = run
    h = Host()
    w = spec.to_c()
    sp = abi.timeline_spec(G, B)
    rows = np.ascontiguousarray(ref.timeline(tr, G, B), abi.timeline_dtype()).ravel()
    need = C.c_int64(0)
    fn = h.L.ccka_host_export_timeline
    args = (h.h, EXPORT_CSV, C.byref(w), C.byref(sp), rows.ctypes.data, rows.size, 0)
    assert fn(*args, None, 0, C.byref(need)) != 0 and need.value > 16
    assert b"output buffer too small" in h.L.ccka_host_last_error(h.h)
    small = C.create_string_buffer(16)
    n1 = need.value
    assert fn(*args, small, 16, C.byref(need)) != 0 and need.value == n1
    exact = C.create_string_buffer(n1)
    assert fn(*args, exact, n1, C.byref(need)) == 0 and len(exact.value) == n1 - 1
    assert fn(*args, exact, n1 - 1, C.byref(need)) != 0
    # no rows: the header alone
    assert h.export_timeline(w, sp, rows[:0], EXPORT_CSV).count("\n") == 1
    with pytest.raises(abi.CckaError):
        h.export_timeline(w, sp, rows, 7)
    with pytest.raises(abi.CckaError):
        h.export_timeline(w, abi.timeline_spec(G, B, 4, 0), rows)
    assert fn(h.h, EXPORT_CSV, C.byref(w), None, rows.ctypes.data, rows.size, 0, exact, n1, C.byref(need)) == -1
