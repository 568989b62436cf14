"""The small kernels of csrc/util.hip on the GPU against the plain references
of tests/util_ref.py and the CPU oracle, at the shapes where they can go
wrong: the load generator on wide parameters (negative intermediates, both
clamps, every deployment, a changing high id word) and its parameter
validation, the totals reduction at its partial / chunk boundaries and on
every overflow rule, the trajectory read-back at every kind of step block, and
the two trace layouts on their whole output buffers, padding included."""
import dataclasses

import numpy as np
import pytest

import pyoracle as po
import util_ref as ur
from ccka import abi, configs
from ccka.world import ScenarioSet, deployment
from parity import run_engine

pytestmark = pytest.mark.gpu
SENTINEL = 0x5EA7BEEF


# ---- the load generator -----------------------------------------------------
def _gen_on_device(engine, gen, T, D, n, first_id, n_traces):
    spec = dataclasses.replace(configs.config2_world(n_steps=T), deploys=[deployment() for _ in range(D)])
    engine.set_world(spec)
    engine.set_scenarios(ScenarioSet(n, first_id, n_traces))
    engine.gen_load(gen)
    return engine.get_load()


@pytest.mark.parametrize("negative", [False, True], ids=["wide", "negative"])
@pytest.mark.parametrize("shape", ur.GEN_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_generator_on_wide_parameters(engine, shape, negative):
    # (that these cases reach both clamps and the truncating divisions of
    # negative dividends is asserted from the reference alone in test_util_ref.py)
    T, D, n, first_id, n_traces = shape
    want, _ = ur.gen_case(shape, negative)
    got = _gen_on_device(engine, ur.wide_gen(negative), T, D, n, first_id, n_traces)
    assert got.shape == want.shape == (T, D, n_traces or n)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} samples differ from SEMANTICS 4, first (t, d, i) {bad[:5].tolist()}"
    orc = po.gen_load(ur.wide_gen(negative), T, D, n_traces or n, 0 if n_traces else first_id)
    assert np.array_equal(got, orc)


def _gen(**kw):
    g = configs.trace_gen()
    for k, v in kw.items():
        setattr(g, k, v)
    return g


# one generator per rule of ccka_trace_gen's accepted set (include/ccka.h), and
# the reason ccka_last_error gives for it
REJECTED = {
    "base hi < lo": (_gen(base_lo=10, base_hi=9), "hi < lo"),
    "amp hi < lo": (_gen(amp_lo_pm=1, amp_hi_pm=0), "hi < lo"),
    "base width + 1 beyond int32": (_gen(base_lo=-1, base_hi=2**31 - 2), "width"),
    "amp width + 1 beyond int32": (_gen(base_lo=0, base_hi=1, amp_lo_pm=-2**30, amp_hi_pm=2**30), "width"),
    "burst_len < 0": (_gen(burst_len=-1), "burst_len < 0"),
    "bstart + burst_len wraps": (_gen(burst_len=2**31 - 1439), "bstart"),
    # 2^31 * (65536000 + 65536 * 2^17) = 2^31 * 8655470592 > 2^63
    "first product leaves int64": (_gen(base_lo=-2**31, base_hi=-2**31 + 9, amp_lo_pm=0, amp_hi_pm=2**17),
                                   r"base \* "),
    # V1 = 2e9 * 4, * (37837000 + 131072 * 2^20) > 2^63
    "second product leaves int64": (_gen(base_lo=0, base_hi=2 * 10**9, amp_lo_pm=0, amp_hi_pm=3000,
                                         noise_pm=-2**20), "noise"),
    # V2 = 3.57e10, * 2^31 > 2^63
    "burst product leaves int64": (_gen(base_lo=0, base_hi=2 * 10**9, amp_lo_pm=0, amp_hi_pm=3000, noise_pm=1000,
                                        burst_mult_pm=-2**31), "burst_mult"),
}


@pytest.mark.parametrize("why", sorted(REJECTED))
def test_generator_rejects_undefined_parameters(engine, why):
    engine.set_world(configs.config2_world(n_steps=4))
    engine.set_scenarios(ScenarioSet(8))
    gen, reason = REJECTED[why]
    with pytest.raises(abi.CckaError, match="EINVAL.*" + reason):
        engine.gen_load(gen)
    # the largest accepted burst_len, and the generator every workload uses
    engine.gen_load(_gen(burst_len=2**31 - 1 - 1439))
    engine.gen_load(configs.trace_gen())
    assert np.array_equal(engine.get_load(), po.gen_load(configs.trace_gen(), 4, 1, 8))


# ---- totals -------------------------------------------------------------------
def _totals_equal(t: abi.Totals, want: dict):
    for f, _ in t._fields_:
        got = getattr(t, f)
        if isinstance(got, float):
            assert got.hex() == float(want[f]).hex(), f
        else:
            assert got == want[f], (f, got, want[f])


def _oracle_totals(cols):
    """(abi.Totals or None, flagged) from the CPU oracle."""
    full = {name: np.zeros(len(cols["cost_uphmin"]), dt) for name, _, dt in abi.RESULT_FIELDS}
    for k, v in cols.items():
        full[k] = np.ascontiguousarray(v, full[k].dtype)
    try:
        return po.totals(full, len(cols["cost_uphmin"])), False
    except OverflowError:
        return None, True


# 262144: 1024 full partials; 262145: chunk 257, so the trailing workgroups' ranges are empty
@pytest.mark.parametrize("n", ur.TOTALS_N)
def test_totals_at_partial_boundaries(engine, n):
    cols = ur.random_columns(n)
    want, flagged = ur.totals(cols)
    assert not flagged
    got = engine.debug_totals(cols)
    _totals_equal(got, want)
    orc, oflag = _oracle_totals(cols)
    assert not oflag and bytes(got) == bytes(orc)


def test_totals_overflow_rules(engine):
    clean = ur.random_columns(1000, seed=1)
    clean_want, _ = ur.totals(clean)
    for name, cols, flagged in ur.totals_edge_cases():
        want, rflag = ur.totals(cols)
        orc, oflag = _oracle_totals(cols)
        assert rflag == oflag == flagged, name
        if flagged:
            with pytest.raises(abi.CckaError, match="EOVERFLOW"):
                engine.debug_totals(cols)
            # the flag word is rewritten by every call, not sticky
            _totals_equal(engine.debug_totals(clean), clean_want)
        else:
            got = engine.debug_totals(cols)
            _totals_equal(got, want)
            assert bytes(got) == bytes(orc), name


# ---- trajectory read-back -----------------------------------------------------
def _readbacks(engine, n, T, blocks):
    spec = configs.config2_world(n_steps=T)
    sc = configs.hpa_scenarios(n)
    try:
        engine.debug_traj_stage(0)
        _, first = run_engine(engine, spec, sc, gen=configs.trace_gen(), traj=True)  # default capacity: tc = T
        assert engine.last_engine()[0] == 2  # the single-deployment engine: [N][T] on the device
        native, lay = engine.trajectory_native()
        assert lay == abi.TRAJ_NT and native.shape == (n, T)
        assert np.array_equal(first, native.T)
        _, want = po.rollout(spec, sc, engine.get_load(), traj=True, threads=8)
        assert np.array_equal(first, want)
        # records that differ along both axes, or a misplaced block would go unseen
        assert (want["replicas"][1:] != want["replicas"][:-1]).any(axis=1).sum() > T // 4
        assert (want["replicas"][:, 1:] != want["replicas"][:, :-1]).any(axis=0).sum() > n // 2
        for tc in blocks:
            # tc steps per block whatever larger staging buffer the read-backs before left
            engine.debug_traj_stage(tc * n)
            got = engine.trajectory()
            bad = np.argwhere(got != want)
            assert bad.size == 0, f"tc {tc}: {len(bad)} records differ, first (t, i) {bad[:5].tolist()}"
    finally:
        engine.debug_traj_stage(0)


def test_trajectory_readback_at_every_block_size(engine):
    # 71 steps: blocks of 1, of less than / exactly / more than one 32-step
    # tile, a last block shorter than tc (all but 1 and 71), and the whole horizon
    _readbacks(engine, 203, 71, (1, 2, 31, 32, 33, 70, 71))


@pytest.mark.parametrize("n", [31, 33, 64])
def test_trajectory_readback_narrow_batches(engine, n):
    _readbacks(engine, n, 71, (33,))


# ---- trace layouts --------------------------------------------------------------
def _trace(T, D, NL):
    rng = np.random.default_rng([T, D, NL])
    a = rng.integers(-2**31, 2**31 - 1, (T, D, NL), dtype=np.int64, endpoint=True).astype(np.int32)
    a[a == SENTINEL] = 0  # so that a surviving sentinel is unambiguous
    return a


@pytest.mark.parametrize("dp", [2, 4, 8, 16])
def test_trace_nt_layout_whole_buffer(engine, dp):
    tt = 32 // dp  # steps per LDS tile
    for D in sorted({1, dp - 1, dp}):
        for T in sorted({1, tt - 1, tt, tt + 1, 67} - {0}):
            for NL in (1, 63, 64, 65, 130):
                trace = _trace(T, D, NL)
                got = engine.debug_trace_layout(trace, dp=dp, sentinel=SENTINEL)
                want = ur.trace_nt(trace, dp)
                assert not (got == SENTINEL).any(), (D, T, NL, "an element of the layout was not written")
                assert np.array_equal(got, want), (D, T, NL)
                assert not got.reshape(NL, T, dp)[:, :, D:].any(), (D, T, NL, "padding not zero")


@pytest.mark.parametrize("lpw", [1, 7, 23, 64])
def test_trace_tile_layout_whole_buffer(engine, lpw):
    for N in (1, 63, 64, 65, 997):
        for T in (1, 5):
            trace = _trace(T, 1, N)
            got = engine.debug_trace_layout(trace, lpw=lpw, sentinel=SENTINEL)
            # the lanes of the last wave past N keep the sentinel: the copy
            # writes the N * T defined elements and nothing else
            assert np.array_equal(got, ur.trace_tile(trace, lpw, SENTINEL)), (N, T)
            assert int((got == SENTINEL).sum()) == T * (-N % lpw), (N, T)
