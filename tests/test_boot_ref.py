"""CPU-side checks of the paired bootstrap (docs/SEMANTICS.md 9): the struct
sizes behind ccka_boot_sizes, the worked example of the text, the restated
Philox of this counter layout against the oracle's, properties of the indices,
the degenerate cases, wrapping and non-wrapping columns, and the activity floors
of the two sweeps tests/test_gpu_boot.py runs, computed with the CPU oracle
alone: a device row that came out all zero or all B could not pass there."""
import ctypes as C

import numpy as np
import pytest

import boot_ref as ref
import paired_ref
import pyoracle as po
from ccka import abi, configs
from test_paired_ref import BASE, GRID_LO, N_GRIDS, N_TRACES, T, _cols, cross_worlds, sweep_inputs

SEED = 0x123456789ABCDEF
B_SWEEP = 200


def test_struct_sizes_and_abi_version():
    assert [C.sizeof(s) for s in abi.BOOT_STRUCTS] == [40, 40, 208]
    assert abi.boot_dtype().itemsize == 208
    lib = abi.load_engine()
    buf = (C.c_int64 * 8)()
    assert lib.ccka_boot_sizes(buf, 8) == 3 and list(buf[:3]) == [40, 40, 208]
    assert lib.ccka_boot_sizes(buf, 2) == 2 and lib.ccka_boot_sizes(None, 3) == 0
    assert lib.ccka_abi_version() == 7 == abi.ABI_VERSION
    big = (C.c_int64 * 32)()
    assert lib.ccka_struct_sizes(big, 32) == 14 and lib.ccka_paired_sizes(big, 32) == 3
    abi.check_sizes(lib)
    sp = abi.boot_spec(48, 37, 200, (1 << 64) - 1, 1, 999999)
    assert (sp.grid_size, sp.base_grid, sp.seed, sp.replicates, sp.lo_ppm, sp.hi_ppm, sp._pad) == \
        (48, 37, (1 << 64) - 1, 200, 1, 999999, 0)
    d = abi.boot_spec(7)
    assert (d.base_grid, d.replicates, d.seed, d.lo_ppm, d.hi_ppm) == (abi.PAIRED_SAME, 1000, 0, 25000, 975000)


def test_worked_example_of_the_text():
    """Deltas [-2, 0, 5, 0], B = 3, seed 0: the index table of SEMANTICS 9."""
    base, cur = _cols([10, 20, 30, 40]), _cols([8, 20, 35, 40])
    b = ref.Boot(cur, base, 4)
    assert not b.ovf and b.p.d[0][0] == [-2, 0, 5, 0]
    idx = ref.indices(4, 3, 0)
    assert idx.tolist() == [[2, 3, 1, 1], [0, 3, 3, 1], [1, 1, 3, 1]]
    assert b.sums(3, 0)[0][0] == [5, -2, 0]
    lib = abi.load_engine()
    assert (lib.ccka_sweep_rank(3, 25000), lib.ccka_sweep_rank(3, 975000), lib.ccka_sweep_rank(3, 500000)) == (1, 3, 2)
    r = b.rows(3, 0)[0]
    c = r["obj"][0]
    assert (c["sum"], c["lo"], c["hi"], c["n_less"], c["n_greater"]) == (3, -2, 5, 1, 1)
    assert b.rows(3, 0, 500000, 500000)[0]["obj"][0]["lo"] == 0
    assert (r["grid"], r["base"], r["pairs"], r["replicates"], r["n_dominates"], r["n_dominated"]) == (0, 0, 4, 3, 1, 1)
    for o in (1, 2, 3):
        assert r["obj"][o].tolist() == (0,) * 5


def test_restated_philox_equals_the_oracle_for_this_counter_layout():
    out = (C.c_uint32 * 4)()
    fn = po.lib().ccka_oracle_philox
    for seed in (0, (1 << 64) - 1, SEED):
        k0, k1 = seed & ref.M32, seed >> 32
        for c0, r in ((0, 0), (1, 2), (624, 999), ((1 << 29) - 1, 65535)):
            fn(c0, r, 0, ref.TAG, k0, k1, out)
            got = [int(np.asarray(x).reshape(-1)[0]) for x in ref.philox(c0, r, 0, ref.TAG, k0, k1)]
            assert got == list(out), (seed, c0, r)
    # and the index rule on top of it, word by word
    n, B = 7, 3
    idx = ref.indices(n, B, SEED)
    for r in range(B):
        for i in range(n):
            fn(i // 4, r, 0, ref.TAG, SEED & ref.M32, SEED >> 32, out)
            assert idx[r, i] == (out[i % 4] * n) >> 32


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 257, 2500])
def test_indices_lie_in_range_and_ignore_the_tail_words(n):
    idx = ref.indices(n, 65, SEED)
    assert idx.shape == (65, n) and idx.min() >= 0 and idx.max() < n
    # words past n in the last call are discarded: a longer grid's first n draws use the same words
    w = ref.words(n, 65, SEED)
    assert np.array_equal(w, ref.words(n + 3, 65, SEED)[:, :n]) and int(w.max()) <= ref.M32
    assert np.array_equal(idx, (w.astype(object) * n // (1 << 32)).astype(np.int64))
    cnt = ref.counts(n, 65, SEED)
    assert cnt.sum(axis=1).tolist() == [n] * 65


def test_every_position_is_drawn():
    cnt = ref.counts(2500, 1000, 7)
    assert (cnt.sum(axis=0) > 0).all()
    assert len({tuple(r) for r in ref.indices(2500, 4, 7).tolist()}) == 4     # replicates differ
    assert not np.array_equal(ref.indices(2500, 1, 7), ref.indices(2500, 1, 8))


def test_degenerate_cases():
    cur, base = paired_ref._columns(1, 6, 6)
    b = ref.Boot(cur, base, 1)
    rows, S = b.rows(65, SEED), b.sums(65, SEED)
    for g in range(6):
        for o in range(4):
            d0 = b.p.d[g][o][0]
            assert S[g][o] == [d0] * 65                                     # n = 1: every S = d[0]
            ob = rows[g]["obj"][o]
            assert ob["sum"] == ob["lo"] == ob["hi"] == d0
            assert (ob["n_less"], ob["n_greater"]) == (65 * (d0 < 0), 65 * (d0 > 0))
    cur, _ = paired_ref._columns(257, 6, 6)
    z = ref.Boot(cur, cur, 257).rows(65, SEED)                              # a grid against itself
    assert not z["obj"].view(np.int64).any() and not z["n_dominates"].any() and not z["n_dominated"].any()
    assert (z["replicates"] == 65).all() and (z["pairs"] == 257).all() and z["grid"].tolist() == z["base"].tolist()


@pytest.mark.parametrize("g", [65, 257, 2500])
def test_wrapping_and_scaled_columns(g):
    cur, base = paired_ref._columns(g, 6, 6)
    b = ref.Boot(cur, base, g)
    assert not b.ovf
    cnt = ref.counts(g, 65, SEED)
    wraps = 0
    for per in b.p.d:
        for d in per:
            plain = ref.replicate_sums(d, cnt, wrapped=False)
            assert plain == [sum(int(c) * x for c, x in zip(row, d)) for row in cnt[:3].tolist()] + plain[3:]
            wraps += sum(paired_ref.wrap(s) != s for s in plain)
    assert wraps >= 1                                                       # some pattern's sums wrap
    assert not ref.no_wrap(b.p.rows())
    cur, base = ref.scaled_columns(g)
    for base_grid in (0, 1, ref.SAME):
        s = ref.Boot(cur, base, g, base_grid)
        assert not s.ovf and ref.no_wrap(s.p.rows())
        for per in s.p.d:
            for d in per:
                plain = ref.replicate_sums(d, cnt, wrapped=False)
                assert all(paired_ref.wrap(x) == x for x in plain)
    d = ref.Boot(cur, base, g).p.d
    assert set(d[3][0]) == {0} and len(set(d[5][0])) == 1 and len(set(d[4][0])) > 1   # the patterns survive the scaling


# ---- the activity floors of the two GPU sweeps -------------------------------
def same_world_floors(rows, what):
    """Cost intervals wholly below 0, wholly above and straddling it, and a
    dominance count strictly inside (0, B): each class at least once."""
    c = rows["obj"][:, 0]
    below, above = int((c["hi"] < 0).sum()), int((c["lo"] > 0).sum())
    straddle = int(((c["lo"] <= 0) & (c["hi"] >= 0) & (c["lo"] < c["hi"])).sum())
    inside = int(((rows["n_dominates"] > 0) & (rows["n_dominates"] < B_SWEEP)).sum())
    print(what, "below", below, "above", above, "straddle", straddle, "n_dominates inside (0, B)", inside)
    assert below >= 1 and above >= 1 and straddle >= 1 and inside >= 1, (what, below, above, straddle, inside)


def cross_world_floors(rows, what):
    """Every grid has replicate cost sums of both signs."""
    c = rows["obj"][:, 0]
    both = (c["n_less"] >= 1) & (c["n_greater"] >= 1)
    print(what, "grids with cost sums of both signs", int(both.sum()))
    assert both.all(), (what, c["n_less"], c["n_greater"])


def test_same_world_sweep_floors():
    sc, load = sweep_inputs()
    res, _ = po.rollout(configs.config2_world(n_steps=T), sc, load, threads=8)
    b = ref.Boot(res, res, N_TRACES, BASE, first_grid=GRID_LO, snap_first_grid=GRID_LO)
    assert not b.ovf
    rows = b.rows(B_SWEEP, SEED)
    same_world_floors(rows, "same world, baseline grid 37")
    assert not rows[BASE - GRID_LO]["obj"].view(np.int64).any()   # the baseline's own row
    assert np.array_equal(rows["obj"]["sum"], b.p.rows()["obj"]["sum"])


def test_cross_world_sweep_floors():
    sc, load = sweep_inputs()
    plain, disrupt = cross_worlds()
    r0, _ = po.rollout(plain, sc, load, threads=8)
    r1, _ = po.rollout(disrupt, sc, load, threads=8)
    b = ref.Boot(r1, r0, N_TRACES, first_grid=GRID_LO, snap_first_grid=GRID_LO)
    assert not b.ovf
    rows = b.rows(B_SWEEP, SEED)
    assert rows["grid"].tolist() == rows["base"].tolist() == list(range(GRID_LO, GRID_LO + N_GRIDS))
    cross_world_floors(rows, "drift + replace against plain, SAME")
