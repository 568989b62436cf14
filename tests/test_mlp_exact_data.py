"""Preconditions of the exact-arithmetic GPU tests (test_gpu_mlp.py,
test_gpu_pg.py), on the CPU: for every (seed, rows) those tests use,
mlp_ref.exact_case really is data on which the MLP forward and backward are
exact in bf16 operands and fp32 sums in any order, and it still exercises the
network (non-zero gradients, both ReLU branches, every action). Also the
helpers those tests lean on: the work-array decode against rb_off, the numpy
Philox against the oracle's, and the sampling restatement's edge rules."""
import numpy as np
import pytest

import mlp_ref
import pyoracle as po

CASES = sorted(set(mlp_ref.EXACT_CASES) | {(0, 1189)})


@pytest.mark.parametrize("seed,m", CASES)
def test_exact_case_preconditions(seed, m):
    c = mlp_ref.exact_case(seed, m)
    r = c["ref"]
    # every row's logits are equal: softmax is 1/8 whatever expf's last bits
    assert np.array_equal(r["y"], np.broadcast_to(r["y"][:, :1], r["y"].shape))
    assert np.abs(r["y"]).max() < 2 ** 24 and np.array_equal(r["y"], np.rint(r["y"]))
    # the hidden halves repeat on this data (what makes W3's halves cancel)
    assert np.array_equal(r["h1"][:, :128], r["h1"][:, 128:]) and np.array_equal(r["h2"][:, :128], r["h2"][:, 128:])
    # every MFMA operand is a bf16 value; rounding at the operand points is the identity
    for name in ("h1", "h2", "g", "dh2", "dh1"):
        assert mlp_ref.is_bf16(r[name]), name
    assert mlp_ref.is_bf16(c["x"]) and all(mlp_ref.is_bf16(w) for w in c["ws"])
    rr = mlp_ref.backward(c["x"], c["act"], c["coef"], c["ws"], c["bs"], round_bf16=True)
    for name, v in r.items():
        assert np.array_equal(v, rr[name]), name
    # order independence: every term of every sum is a multiple of `unit` and
    # sum |terms| / unit < 2^24, so each partial sum in any order is an fp32 value
    unit = c["unit"]
    ax, ah1, ah2 = np.abs(c["x"]).astype(np.float64), np.abs(r["h1"]), np.abs(r["h2"])
    ag, ad2, ad1 = np.abs(r["g"]), np.abs(r["dh2"]), np.abs(r["dh1"])
    for name in ("g", "dh2", "dh1"):
        assert np.array_equal(r[name] / unit, np.rint(r[name] / unit)), name
    sums = {"w1": ax.T @ ad1, "b1": ad1.sum(0), "w2": ah1.T @ ad2, "b2": ad2.sum(0), "w3": ah2.T @ ag, "b3": ag.sum(0)}
    for name, s in sums.items():
        assert s.max() / unit < 2 ** 24, (name, np.log2(s.max() / unit))
        assert np.array_equal(r[name].astype(np.float32).astype(np.float64), r[name]), name
    # the row-wise sums too (layers 1-3 forward, dH2 and dH1): integers / multiples of unit far below 2^24
    w1, w2, w3 = (np.abs(w).astype(np.float64) for w in c["ws"])
    assert max((ax @ w1).max(), (ah1 @ w2).max(), (ah2 @ w3).max()) + 3 < 2 ** 24
    assert max((ag @ w3.T).max(), (ad2 @ w2.T).max()) / unit < 2 ** 24
    # activity: the case still exercises the network
    act2 = (r["h2"] > 0).mean()
    assert 0.3 <= act2 <= 0.7, act2
    if m >= 31:
        assert (r["w1"] != 0).mean() >= 0.9 and (r["w2"] != 0).mean() >= 0.8
        assert len(np.unique(c["act"])) == 8
        assert (r["dh1"] != 0).mean() >= 0.25
    else:
        assert (r["dh1"] != 0).any() and (r["dh2"] != 0).any()


def test_exact_case_without_k_has_constant_logits():
    c = mlp_ref.exact_case(0, 1189, False)
    assert np.array_equal(c["ref"]["y"], np.broadcast_to(c["bs"][2].astype(np.float64), (1189, 8)))
    # with k the logits differ from row to row (a row permutation would show)
    assert len(np.unique(mlp_ref.exact_case(0, 1189)["ref"]["y"][:, 0])) > 8


_splits = mlp_ref.wgrad_splits


def test_exact_rows_include_an_empty_weight_gradient_split():
    """4,865 rows is among the exact cases because its last weight-gradient
    split starts at Mpad and owns no row (it must still write zero partials):
    the property from the code's own constants, so that a change of kPgSplits
    does not silently lose the case; no smaller row count has it."""
    assert 4865 in mlp_ref.PG_EXACT_ROWS
    mp = mlp_ref.mpad(4865)
    splits, chunk = _splits(mp)
    assert splits > 1 and (splits - 1) * chunk >= mp, (splits, chunk)
    for smaller in range(32, mp, 32):
        s, ch = _splits(smaller)
        assert (s - 1) * ch < smaller, smaller


def test_decode_work_is_rb_off():
    mp = 96
    rng = np.random.default_rng(0)
    arrays = {name: rng.integers(0, 65536, size=(mp, u)).astype(np.uint16) for name, u in mlp_ref.WORK_UNITS}
    buf = mlp_ref.encode_work(arrays, mp)
    got = mlp_ref.decode_work(np.concatenate([buf, np.zeros(7, np.uint16)]), mp)
    for name, _ in mlp_ref.WORK_UNITS:
        assert np.array_equal(got[name], arrays[name]), name
    # one element by the formula: unit 5, row 37 of h1T (256 units) behind xT
    assert buf[64 * mp + ((37 >> 4) * 256 + 5) * 16 + (37 & 15)] == arrays["h1"][37, 5]


def test_numpy_philox_is_the_oracles():
    ids = np.array([0, 1, 99, 2 ** 32 + 5, 2 ** 40 + 123], np.int64)
    for seed, t in ((9, 0), (2 ** 40 + 3, 29)):
        w0 = mlp_ref.philox(ids & 0xFFFFFFFF, ids >> 32, t, 0x5A3B1E7, seed & 0xFFFFFFFF, seed >> 32)[0]
        assert np.array_equal((w0 >> 8) / 16777216.0, po.policy_uniform(seed, ids, t))


def test_gen_states_restatement_shape_and_moments():
    x = mlp_ref.configs.from_bf16_bits(mlp_ref.gen_states(4096, 7))
    assert x.shape == (4096, 64) and abs(float(x.mean())) < 0.01 and 0.95 < float(x.std()) < 1.05


def test_sample_bins_edges():
    y = np.zeros((4, 8), np.float32)
    u = np.array([0.0, 0.125, 1.0 - 2.0 ** -24, 0.5 - 2.0 ** -24])
    b, near = mlp_ref.sample_bins(y, u)
    assert b.tolist() == [0, 1, 7, 3]  # u * sum == a partial sum goes to the next bin
    assert near.tolist() == [False, True, False, True]
    # one dominant logit: every other numerator underflows to 0, all draws land on it
    y = np.full((2, 8), -200.0, np.float32)
    y[:, 5] = 0.0
    assert mlp_ref.sample_bins(y, np.array([0.0, 1.0 - 2.0 ** -24]))[0].tolist() == [5, 5]
