"""GPU numerics of the bf16 MFMA MLP control policy (BASELINE config 5)
against a plain PyTorch fp32 reference of the same op. The reference rounds the
hidden activations to bf16 exactly where the kernel does (the MFMA operands of
the next layer); accumulation is fp32 on both sides. Both standalone kernels
run: mlp16_kernel (the context's default) and mlp_kernel (the kernel of both
policy loops), chosen with ccka_debug_mlp_tile. On exact data (small integers;
mlp_ref.exact_case) the comparison is equality."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import mlp_ref
from ccka import configs

pytestmark = pytest.mark.gpu


def torch_ref(x_bits, ws_bits, bs):
    bf = lambda a: torch.from_numpy(configs.from_bf16_bits(a))  # noqa: E731
    x = bf(x_bits)
    w1, w2, w3 = (bf(w) for w in ws_bits)
    b1, b2, b3 = (torch.from_numpy(b) for b in bs)
    h1 = torch.relu(x @ w1 + b1).to(torch.bfloat16).float()
    h2 = torch.relu(h1 @ w2 + b2).to(torch.bfloat16).float()
    return (h2 @ w3 + b3).numpy()


@contextlib.contextmanager
def mlp_tile(engine, tile):
    """The standalone forward on mlp_kernel (32: v_mfma 32x32x16, the kernel of
    both policy loops) or mlp16_kernel (16: 16x16x32, the context's default)."""
    fn = engine.lib.ccka_debug_mlp_tile
    fn.argtypes = [C.c_void_p, C.c_int32]
    assert fn(engine.ctx, tile) == 0
    try:
        yield
    finally:
        assert fn(engine.ctx, 16) == 0


def run_forward(engine, x_bits, tile):
    engine.mlp_set_states(x_bits)
    with mlp_tile(engine, tile):
        engine.mlp_forward()
    return engine.mlp_actions()


# the edges of both tilings: mlp16_kernel runs four 16-state tiles per wave
# pass, mlp_kernel two 32-state tiles; then a ragged last tile, an odd number
# of tiles, and one full pass of a 256-CU grid plus a ragged tail
SIZES = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 129, 32 * 37 + 5, 32 * 38 + 7, 64 * 256 * 4 + 33]


@functools.lru_cache(maxsize=None)
def _integer_case(n):
    rng = np.random.default_rng(3)
    x = rng.integers(-1, 2, size=(n, 64)).astype(np.float32)
    w1 = rng.integers(-1, 2, size=(64, 256)).astype(np.float32)
    w2 = (rng.integers(-1, 2, size=(256, 256)) * (rng.random((256, 256)) < 0.02)).astype(np.float32)
    w3 = rng.integers(-2, 3, size=(256, 8)).astype(np.float32)
    bs = [rng.integers(-3, 4, size=k).astype(np.float32) for k in (256, 256, 8)]
    wb = [configs.to_bf16_bits(w) for w in (w1, w2, w3)]
    xb = configs.to_bf16_bits(x)
    return xb, wb, bs, torch_ref(xb, wb, bs)


@pytest.mark.parametrize("tile", [16, 32])
@pytest.mark.parametrize("n", SIZES)
def test_mlp_exact_integer_data(engine, n, tile):
    """Small integers: every product, sum and bf16 activation is exact, so any
    fragment-layout / k-order error shows up as an exact mismatch, on both
    standalone kernels and at the edges of both tilings."""
    xb, wb, bs, want = _integer_case(n)
    engine.mlp_set_weights(wb, bs)
    got = run_forward(engine, xb, tile)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("tile", [16, 32])
@pytest.mark.parametrize("k3", [False, True])
def test_mlp_exact_case_logits_cancel(engine, tile, k3):
    """mlp_ref.exact_case at 1,189 rows: W3's second half cancels the first on
    hidden halves that repeat, which holds only if the k-orders of layers 2 and
    3 agree. Without the per-unit offset k every output of every row is the
    constant b3; with it a row's 8 outputs are equal and the rows differ (a
    row permutation would show): the float64 reference, exactly."""
    c = mlp_ref.exact_case(0, 1189, k3)
    engine.mlp_set_weights([configs.to_bf16_bits(w) for w in c["ws"]], c["bs"])
    got = run_forward(engine, configs.to_bf16_bits(c["x"]), tile)
    if not k3:
        assert np.array_equal(got, np.broadcast_to(c["bs"][2], got.shape))
    assert np.array_equal(got, np.broadcast_to(got[:, :1], got.shape))
    assert np.array_equal(got, c["ref"]["y"].astype(np.float32))


def test_mlp_random_data_tolerance(engine):
    ws, bs = configs.mlp_weights(11)
    wb = [configs.to_bf16_bits(w) for w in ws]
    n = 20000
    xb = configs.to_bf16_bits(np.random.default_rng(7).standard_normal((n, 64)).astype(np.float32))
    engine.mlp_set_weights(wb, bs)
    engine.mlp_set_states(xb)
    engine.mlp_forward()
    got = engine.mlp_actions()
    want = torch_ref(xb, wb, bs)
    # fp32 accumulation order differs; a bf16 activation may round to the
    # neighbouring value when the sums differ in the last fp32 bit
    err = np.abs(got - want)
    assert err.max() <= 2e-2 * max(1.0, float(np.abs(want).max())), err.max()
    assert err.mean() <= 1e-3, err.mean()


def test_mlp_device_states(engine):
    """The device state generator against its numpy restatement
    (mlp_ref.gen_states; there is no getter for the states): the forward of
    the generated states equals the forward of the restated ones bit for bit
    (same bf16 bits in, same kernel), on both kernels, and the output really
    depends on the states."""
    ws, bs = configs.mlp_weights(11)
    engine.mlp_set_weights([configs.to_bf16_bits(w) for w in ws], bs)
    restated = mlp_ref.gen_states(4096, 7)
    for tile in (16, 32):
        engine.mlp_gen_states(4096, seed=7)
        with mlp_tile(engine, tile):
            engine.mlp_forward()
        y = engine.mlp_actions()
        assert np.isfinite(y).all() and y.std() > 0
        want = run_forward(engine, restated, tile)
        assert np.array_equal(y, want), tile
    other = run_forward(engine, mlp_ref.gen_states(4096, 8), 32)
    assert (other != want).mean() > 0.9
