"""CPU-side checks of the sweep statistics' ABI: ccka_sweep_rank (the nearest
rank of docs/SEMANTICS.md 6, integers only) against the integer formula, and
the abi.sweep_stat constructor."""
import pytest

from ccka import abi
from sweep_stat_ref import rank

NS = [1, 2, 47, 48, 1024, 10**9]
QS = [0, 1, 499999, 500000, 950000, 999999, 10**6]


@pytest.fixture(scope="module")
def lib():
    return abi.load_engine()


@pytest.mark.parametrize("n", NS)
def test_sweep_rank_is_the_integer_nearest_rank(lib, n):
    for q in QS:
        k = lib.ccka_sweep_rank(n, q)
        assert k == max(1, (q * n + 999999) // 1000000) == rank(n, q), (n, q)
        assert 1 <= k <= n
    assert lib.ccka_sweep_rank(n, 0) == 1 and lib.ccka_sweep_rank(n, 10**6) == n


def test_sweep_rank_rejects_bad_arguments(lib):
    for n in (0, -1, -(1 << 40)):
        assert lib.ccka_sweep_rank(n, 500000) == -1
    for q in (-1, 1000001, -(1 << 31)):
        assert lib.ccka_sweep_rank(1024, q) == -1


def test_sweep_stat_constructor():
    st = abi.sweep_stat(slo=("quantile", 950000), energy=("tail", 900000), gco2="sum")
    assert list(st.kind) == [abi.STAT_SUM, abi.STAT_QUANTILE, abi.STAT_SUM, abi.STAT_TAIL]
    assert list(st.q_ppm) == [0, 950000, 0, 900000]
    assert list(abi.sweep_stat().kind) == [0, 0, 0, 0]
    assert abi.STAT_OBJECTIVES == ("cost", "slo", "gco2", "energy")
