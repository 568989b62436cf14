"""Differentiable control (BASELINE config 5, "differentiable-control rollout";
SEMANTICS 5): the score-function gradient of the closed loop's objective.

* The MLP backward (bf16 MFMA, fp32 accumulation) against PyTorch fp32
  autograd of the same forward (bf16-rounded activations with an identity
  gradient through the rounding, as the kernel's operands): the kernel also
  rounds g_y, dH2 and dH1 to bf16 for its MFMAs, so the tolerance is bf16's.
* ccka_policy_grad is that backward applied to the loop's own rows: the
  recorded features, sampled action bins and per-scenario factors reproduce its
  gradient bit for bit through ccka_mlp_backward; the rollout under the
  sampled actions is bit-exact against the CPU oracle; the sampled bins follow
  softmax(y) and the bin -> (target, carbon weight) table.
* On exact-arithmetic data (mlp_ref.exact_case) the six gradients and the six
  work arrays equal the float64 restatement element for element, chunked or
  not; on random data every hidden unit's gradient is checked on its own.
* Every sampled bin equals policy_sample restated in numpy.
* A few plain gradient steps lower the objective on config 2.
Parity of the sampled decisions themselves is unpinned (the reference has no
learned policy); the proposal's objective is the anchor
(CS218_Project_Proposal.pdf p.1, p.5)."""
import ctypes as C

import numpy as np
import pytest
import torch

import mlp_ref
import pyoracle as po
from ccka import configs
from parity import compare

pytestmark = pytest.mark.gpu


def torch_grads(x_bits, actions, coef, ws_bits, bs):
    """d/dW of sum_m coef[m] * log_softmax(policy(x_m))[a_m] in fp32 autograd."""
    bf = lambda a: torch.from_numpy(configs.from_bf16_bits(a))  # noqa: E731
    x = bf(x_bits)
    w = [bf(wb).clone().requires_grad_(True) for wb in ws_bits]
    b = [torch.from_numpy(np.asarray(v, np.float32)).clone().requires_grad_(True) for v in bs]

    def rnd(h):  # the kernel's bf16 operand, identity gradient
        return h + (h.to(torch.bfloat16).float() - h).detach()

    h1 = torch.relu(rnd(x @ w[0] + b[0]))
    h2 = torch.relu(rnd(h1 @ w[1] + b[1]))
    y = h2 @ w[2] + b[2]
    lp = torch.log_softmax(y, dim=1)
    a = torch.from_numpy(np.asarray(actions, np.int64))
    loss = (torch.from_numpy(np.asarray(coef, np.float32)) * lp[torch.arange(len(a)), a]).sum()
    loss.backward()
    return {"w1": w[0].grad.numpy(), "w2": w[1].grad.numpy(), "w3": w[2].grad.numpy(),
            "b1": b[0].grad.numpy(), "b2": b[1].grad.numpy(), "b3": b[2].grad.numpy()}


def rel_err(got, want):
    return float(np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-30))


@pytest.mark.parametrize("m", [1, 31, 32 * 37 + 5, 20000])
def test_mlp_backward_matches_torch_autograd(engine, m):
    rng = np.random.default_rng(m)
    ws, bs = configs.mlp_weights(11)
    wb = [configs.to_bf16_bits(w) for w in ws]
    engine.mlp_set_weights(wb, bs)
    x = configs.to_bf16_bits(rng.standard_normal((m, 64)).astype(np.float32))
    act = rng.integers(0, 8, size=m).astype(np.uint8)
    coef = rng.standard_normal(m).astype(np.float32) / m
    got = engine.mlp_backward(x, act, coef)
    want = torch_grads(x, act, coef, wb, bs)
    for k in want:
        assert got[k].shape == want[k].shape
        e = rel_err(got[k], want[k])
        assert e <= 2e-2, f"{k}: relative error {e:.3e}"


@pytest.mark.parametrize("chunk", [4096, 32 * 37])
def test_mlp_backward_row_chunks(engine, chunk):
    """Row chunks (the backward of N*T rows too many for one work buffer runs
    in chunks of 2^23 rows, each chunk's gradient added in chunk order): with a
    small chunk size forced, 20,000 rows in 5 / 17 chunks give the autograd
    gradient within the same bf16 tolerance and the unchunked kernel's within
    fp32 summation-order rounding; repeated runs are bit-identical."""
    import ctypes as C
    rng = np.random.default_rng(7)
    m = 20000
    ws, bs = configs.mlp_weights(11)
    wb = [configs.to_bf16_bits(w) for w in ws]
    engine.mlp_set_weights(wb, bs)
    x = configs.to_bf16_bits(rng.standard_normal((m, 64)).astype(np.float32))
    act = rng.integers(0, 8, size=m).astype(np.uint8)
    coef = rng.standard_normal(m).astype(np.float32) / m
    whole = engine.mlp_backward(x, act, coef)
    fn = engine.lib.ccka_debug_pg_chunk
    fn.argtypes = [C.c_void_p, C.c_int64]
    assert fn(engine.ctx, chunk) == 0
    try:
        got = engine.mlp_backward(x, act, coef)
        again = engine.mlp_backward(x, act, coef)
    finally:
        fn(engine.ctx, 0)
    want = torch_grads(x, act, coef, wb, bs)
    for k in want:
        assert rel_err(got[k], want[k]) <= 2e-2, k
        assert rel_err(got[k], whole[k]) <= 1e-5, k
        assert np.array_equal(got[k], again[k]), k


def test_mlp_backward_single_row_structure(engine):
    """One row with coef 1: every gradient is a rank-1 outer product; a
    fragment or k-order error would break it far beyond bf16 rounding."""
    ws, bs = configs.mlp_weights(5)
    wb = [configs.to_bf16_bits(w) for w in ws]
    engine.mlp_set_weights(wb, bs)
    x = configs.to_bf16_bits(np.random.default_rng(1).standard_normal((1, 64)).astype(np.float32))
    for a in (0, 3, 7):
        got = engine.mlp_backward(x, np.array([a], np.uint8), np.array([1.0], np.float32))
        want = torch_grads(x, [a], [1.0], wb, bs)
        for k in want:
            assert rel_err(got[k], want[k]) <= 2e-2, k
        # d/dy of log softmax sums to zero over the actions
        assert abs(float(got["b3"].sum())) <= 1e-2 * float(np.abs(got["b3"]).sum())


# ---------------------------------------------------------------------------
# Exact arithmetic (mlp_ref.exact_case): softmax is 1/8, every MFMA operand a
# bf16 value and every sum exact in any fp32 order (test_mlp_exact_data.py
# holds the preconditions on the CPU), so the gradients and every element of
# the work arrays equal the float64 reference. A dropped ragged tile, one
# wrong unit, a row block read twice or a chunk boundary off by a row is a
# mismatch here, not 1e-4 of an array norm.
# ---------------------------------------------------------------------------
def _pg_chunk(engine):
    fn = engine.lib.ccka_debug_pg_chunk
    fn.argtypes = [C.c_void_p, C.c_int64]
    return fn


def pg_work(engine, m):
    """The six work arrays of the last backward (of m rows), uint16 [Mpad][units]."""
    mp = mlp_ref.mpad(m)
    buf = np.zeros(mlp_ref.WORK_ROWS * mp, np.uint16)
    got = C.c_int64(-1)
    fn = engine.lib.ccka_debug_pg_work
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    assert fn(engine.ctx, buf.ctypes.data, buf.size, C.byref(got)) == 0
    assert got.value == mp  # the last backward's Mpad, not the buffer's capacity
    return mlp_ref.decode_work(buf, mp)


def exact_backward(engine, seed, m, coef=None):
    c = mlp_ref.exact_case(seed, m)
    engine.mlp_set_weights([configs.to_bf16_bits(w) for w in c["ws"]], c["bs"])
    return c, engine.mlp_backward(configs.to_bf16_bits(c["x"]), c["act"], c["coef"] if coef is None else coef)


def assert_exact(engine, seed, m):
    c, got = exact_backward(engine, seed, m)
    ref = c["ref"]
    for k in mlp_ref.GRADS:
        want = ref[k].astype(np.float32)  # exact: test_mlp_exact_data.py
        assert got[k].shape == want.shape
        bad = np.argwhere(got[k] != want)
        assert np.array_equal(got[k], want), f"m={m} d{k}: {len(bad)} entries differ, first {bad[:4].tolist()}"
    work = pg_work(engine, m)
    mp = mlp_ref.mpad(m)
    want_x = configs.to_bf16_bits(c["x"])
    for name, want in (("x", want_x), ("h1", mlp_ref.bits(ref["h1"])), ("h2", mlp_ref.bits(ref["h2"])),
                       ("g", mlp_ref.bits(ref["g"])), ("dh2", mlp_ref.bits(ref["dh2"])),
                       ("dh1", mlp_ref.bits(ref["dh1"]))):
        got_a = work[name]
        assert got_a.shape == (mp, want.shape[1])
        bad = np.argwhere(got_a[:m] != want)
        assert np.array_equal(got_a[:m], want), \
            f"m={m} {name}T: {len(bad)} elements differ, first (row, unit) {bad[:4].tolist()}"
    # the weight-gradient kernels sum over Mpad rows: the padding rows of their
    # B operands are zeros (0 * softmax may carry a minus sign: still a zero)
    for name in ("dh1", "dh2", "g"):
        assert not (work[name][m:] & 0x7FFF).any(), f"m={m} {name}T padding rows"
    assert not work["x"][m:].any()


@pytest.mark.parametrize("seed,m", mlp_ref.EXACT_CASES)
def test_mlp_backward_exact(engine, seed, m):
    """All six gradients and all six work arrays of the backward equal the
    float64 reference element for element (x, h1, h2, g, dH2, dH1 as bf16 bits),
    and the padding rows M..Mpad-1 of dh1T, dh2T and gyT are zero. Row counts:
    one row, around one 32-row tile, around 256 and 512 rows (the first split
    boundaries), a ragged middle size, 4,865 (an empty last split) and 20,000.
    The cases run in increasing size within the session's one context."""
    assert_exact(engine, seed, m)


def test_mlp_backward_exact_decreasing_sizes(engine):
    """The same cases from the largest down in one context: the work buffer
    only grows, so each backward runs inside a larger allocation with the
    previous case's rows beyond its own Mpad, and ccka_debug_pg_work must
    report this backward's Mpad for the arrays to be found at all."""
    for m in sorted(mlp_ref.PG_EXACT_ROWS, reverse=True):
        assert_exact(engine, 0, m)


@pytest.mark.parametrize("chunk", [4096, 32 * 37, 1000])
def test_mlp_backward_exact_row_chunks(engine, chunk):
    """20,000 exact rows in 5 / 17 / 20 chunks (the last chunk size no multiple
    of the 32-row tile: every chunk but the last then ends in padding rows)
    give the unchunked gradient and the float64 reference, bit for bit."""
    c, whole = exact_backward(engine, 0, 20000)
    fn = _pg_chunk(engine)
    assert fn(engine.ctx, chunk) == 0
    try:
        got = engine.mlp_backward(configs.to_bf16_bits(c["x"]), c["act"], c["coef"])
    finally:
        assert fn(engine.ctx, 0) == 0
    for k in mlp_ref.GRADS:
        assert np.array_equal(got[k], whole[k]), k
        assert np.array_equal(got[k], c["ref"][k].astype(np.float32)), k
    # the work arrays hold the last chunk: its rows, at its own Mpad
    last = 20000 - (20000 - 1) // chunk * chunk
    work = pg_work(engine, last)
    assert np.array_equal(work["x"][:last], configs.to_bf16_bits(c["x"])[20000 - last:])
    assert np.array_equal(work["dh1"][:last], mlp_ref.bits(c["ref"]["dh1"])[20000 - last:])


def test_mlp_backward_one_row_is_the_softmax_gradient(engine):
    """One row, coef 1: db3 is g itself, e_a - 1/8. A device expf(0) != 1 or
    an inexact 1/8 would show here (an arithmetic property, not a layout bug)."""
    c, got = exact_backward(engine, 0, 1, coef=np.ones(1, np.float32))
    want = np.full(8, -0.125, np.float32)
    want[c["act"][0]] = 0.875
    assert np.array_equal(got["b3"], want), got["b3"].tolist()
    assert np.array_equal(configs.from_bf16_bits(pg_work(engine, 1)["g"][0]), want)


# ---------------------------------------------------------------------------
# Random data, per hidden unit: the softmax itself and the masks at ordinary
# values, with a bound that one wrong unit cannot hide under.
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("m", [32 * 37 + 5, 20000])
def test_mlp_backward_per_unit_error(engine, m):
    """Relative L2 error of every hidden unit's column of dW1, dW2, db1, db2
    and row of dW3 against the float64 restatement that rounds to bf16 at the
    kernel's operand points. The allowance is computed here: 8 x the worst
    per-unit error of the same restatement run in fp32 on the CPU (PyTorch)
    against the float64 run; the factor covers bf16 operands that flip to a
    neighbour (2^-8 relative in one term) where two fp32 sums differ in the
    last bit.

    Measured on an MI355X, worst unit (CPU fp32 / kernel): 1,189 rows dW1
    8.8e-4 / 5.3e-4, dW2 1.1e-3 / 3.1e-4, dW3 5.2e-4 / 5.4e-4, db1 1.8e-1 /
    9.2e-3, db2 7.3e-3 / 2.7e-3; 20,000 rows dW1 4.0e-4 / 7.9e-4, dW2 3.1e-4 /
    4.3e-3, dW3 2.8e-4 / 2.3e-4, db1 5.6e-3 / 2.8e-2, db2 2.0e-2 / 5.4e-3. The
    worst unit of all is a bias gradient (one number per unit, a sum that
    nearly cancels), so the allowance is 1.4 and 0.16: loose for the weight
    gradients. A per-array allowance is not sound either: at 20,000 rows the
    kernel's dW2 column of unit 34 is 4.3e-3 off because ONE ReLU differs
    (row 2875: a bf16 flip in h1 moves the pre-activation of h2 across zero,
    which switches that row's whole term on), a step no multiple of the fp32
    run's error covers. What a wrong unit in the weight-gradient kernels
    cannot hide under is the second check: every gradient against the float64
    sums of the operands the kernels read themselves (the work arrays of this
    backward), per unit, relative to the column of sum |a| |b|. An fp32
    summation tree of depth d is within d 2^-23 of that scale whatever its
    order (bf16 products are exact in fp32; 2^-23 allows an MFMA that
    truncates); d = 16 terms per MFMA + the k-steps of a split + the splits.
    Measured: at most 2.8e-8 (dW3) against the bound 4.6e-6 at 1,189 rows and
    1.3e-5 at 20,000."""
    rng = np.random.default_rng(m)
    ws, bs = configs.mlp_weights(11)
    wb = [configs.to_bf16_bits(w) for w in ws]
    wr = [configs.from_bf16_bits(w) for w in wb]
    engine.mlp_set_weights(wb, bs)
    xb = configs.to_bf16_bits(rng.standard_normal((m, 64)).astype(np.float32))
    x = configs.from_bf16_bits(xb)
    act = rng.integers(0, 8, size=m).astype(np.uint8)
    coef = rng.standard_normal(m).astype(np.float32) / m
    got = engine.mlp_backward(xb, act, coef)
    work = pg_work(engine, m)
    ref = mlp_ref.backward(x, act, coef, wr, bs, round_bf16=True)
    cpu = mlp_ref.column_errors(mlp_ref.backward_f32(x, act, coef, wr, bs), ref)
    err = mlp_ref.column_errors(got, ref)
    cpu_worst = max(float(v.max()) for v in cpu.values())
    own = mlp_ref.own_operand_errors(got, work, m)
    splits, chunk = mlp_ref.wgrad_splits(mlp_ref.mpad(m))
    depth = 16 + chunk // 16 + splits
    for k in err:
        print(f"m={m} d{k}: worst per-unit error CPU fp32 {cpu[k].max():.3e} (unit {int(cpu[k].argmax())}), "
              f"kernel {err[k].max():.3e} (unit {int(err[k].argmax())})")
    for k in own:
        print(f"m={m} d{k}: against its own operands {own[k].max():.3e} (unit {int(own[k].argmax())}), "
              f"bound {depth} x 2^-23 = {depth * 2.0 ** -23:.3e}")
    assert cpu_worst > 0
    for k in err:
        assert err[k].max() <= 8 * cpu_worst, \
            f"d{k} unit {int(err[k].argmax())}: {err[k].max():.3e} > 8 x {cpu_worst:.3e}"
    for k in own:
        assert own[k].max() <= depth * 2.0 ** -23, f"d{k} unit {int(own[k].argmax())}: {own[k].max():.3e}"
    # the operands themselves: the same rows, and active / inactive as the reference
    # in all but a handful of the 256 x m ReLUs (each one a pre-activation next to zero)
    assert np.array_equal(work["x"][:m], xb)
    for name in ("h1", "h2"):
        toggled = np.argwhere((work[name][:m] != 0) != (ref[name] != 0))
        print(f"m={m} {name}: {len(toggled)} ReLUs differ from the reference {toggled[:4].tolist()}")


def _loop_case(n=1024, T=120):
    spec = configs.config2_world(n_steps=T)
    sc = configs.hpa_scenarios(n, first_id=7)
    load = po.gen_load(configs.trace_gen(5), T, 1, n, first_id=7)
    return spec, sc, load


def test_policy_grad_is_the_backward_of_its_own_rows(engine):
    spec, sc, load = _loop_case()
    ws, bs = configs.mlp_weights(11)
    wb = [configs.to_bf16_bits(w) for w in ws]
    engine.set_world(spec)
    engine.set_scenarios(sc)
    engine.set_load(load)
    engine.mlp_set_weights(wb, bs)
    g, obj = engine.policy_grad(seed=123, w_carbon=0.5, w_slo=0.01)
    act, coef = engine.policy_samples()
    feats = engine.debug_get_policy_features()
    tg, cw = engine.policy_actions()
    rg = engine.results()
    # the objective and the factors (J - mean J) / N from the results
    J = rg["cost_uphmin"] / 6e7 + 0.5 * rg["gco2"] * 1e-3 + 0.01 * rg["slo_minutes"]
    assert obj == pytest.approx(J.mean(), rel=1e-12)
    assert np.allclose(coef, ((J - J.mean()) / sc.n).astype(np.float32), rtol=1e-6, atol=1e-12)
    # the bin table: target 40 + 10 (a & 3) %, carbon weight a >> 2
    assert np.array_equal(tg, 40 + 10 * (act.astype(np.int16) & 3))
    assert np.array_equal(cw, (act >> 2).astype(np.float64))
    assert len(np.unique(act)) == 8
    # the same rows through the standalone backward: bit-identical gradient
    T, n = spec.n_steps, sc.n
    rows_x = feats[:T].reshape(T * n, 64)
    rows_c = np.tile(coef, T)
    g2 = engine.mlp_backward(rows_x, act.reshape(-1), rows_c)
    for k in g:
        assert np.array_equal(g[k], g2[k]), k
    # and within bf16 tolerance of PyTorch autograd on those rows
    want = torch_grads(rows_x, act.reshape(-1), rows_c, wb, bs)
    for k in want:
        assert rel_err(g[k], want[k]) <= 2e-2, k
    # the rollout under the sampled actions and every step's features: bit-exact
    # against the oracle
    rc, _, fc = po.rollout_policy(spec, sc, load, tg, cw, threads=16, features=True)
    compare(rg, rc)
    assert np.array_equal(feats, fc)


def test_policy_sampling_follows_softmax_and_seed(engine):
    from test_gpu_mlp import torch_ref
    spec, sc, load = _loop_case(n=4096, T=30)
    ws, bs = configs.mlp_weights(11)
    ws[2] = ws[2] * 4.0  # sharper logits: a non-uniform policy
    wb = [configs.to_bf16_bits(w) for w in ws]
    engine.set_world(spec)
    engine.set_scenarios(sc)
    engine.set_load(load)
    engine.mlp_set_weights(wb, bs)
    engine.policy_grad(seed=9)
    a1, _ = engine.policy_samples()
    feats = engine.debug_get_policy_features()
    engine.policy_grad(seed=9)
    a2, _ = engine.policy_samples()
    assert np.array_equal(a1, a2)  # counter-based: same seed, same samples
    engine.policy_grad(seed=10)
    a3, _ = engine.policy_samples()
    assert (a1 != a3).mean() > 0.2
    # empirical bin frequencies vs the mean softmax probabilities of the rows
    y = torch_ref(feats[:spec.n_steps].reshape(-1, 64), wb, bs)
    pr = torch.softmax(torch.from_numpy(y), dim=1).numpy()
    f = np.bincount(a1.reshape(-1), minlength=8) / a1.size
    assert np.abs(f - pr.mean(0)).max() < 0.01, (f, pr.mean(0))
    # each sample against the oracle's Philox draw: u lies in its bin of the
    # cumulative softmax (PyTorch's y may differ from the kernel's in the last
    # bits, so a draw within 1e-4 of a bin edge may land in the neighbour)
    for t in (0, spec.n_steps - 1):
        u = po.policy_uniform(9, sc.first_id + np.arange(sc.n), t)
        cum = np.cumsum(pr[t * sc.n:(t + 1) * sc.n], axis=1)
        a = a1[t].astype(np.int64)
        lo = np.where(a > 0, cum[np.arange(sc.n), np.maximum(a - 1, 0)], 0.0)
        hi = cum[np.arange(sc.n), a]
        inside = (u >= lo - 1e-4) & (u < hi + 1e-4)
        assert inside.all(), np.nonzero(~inside)[0][:10]
        assert ((u >= lo) & (u < hi)).mean() > 0.999


@pytest.mark.parametrize("chunk", [4096 + 32, 1000])
def test_policy_grad_row_chunks_per_scenario_factors(engine, chunk):
    """ccka_policy_grad's rows (t, i) take the factor of scenario i = row % N.
    With row chunks that do not divide N (512 scenarios x 40 steps in 5 / 21
    chunks) every chunk starts inside a step, so the factor index depends on
    the chunk's first row: the gradient equals, bit for bit, the standalone
    backward of the recorded rows with one factor per row under the same
    chunks, and both stay within fp32 summation order of the unchunked one."""
    spec, sc, load = _loop_case(n=512, T=40)
    assert sc.n % chunk and chunk % sc.n
    ws, bs = configs.mlp_weights(11)
    engine.set_world(spec)
    engine.set_scenarios(sc)
    engine.set_load(load)
    engine.mlp_set_weights([configs.to_bf16_bits(w) for w in ws], bs)
    whole, _ = engine.policy_grad(seed=5, w_carbon=0.5, w_slo=0.01)
    whole = {k: v.copy() for k, v in whole.items()}
    fn = _pg_chunk(engine)
    assert fn(engine.ctx, chunk) == 0
    try:
        g, _ = engine.policy_grad(seed=5, w_carbon=0.5, w_slo=0.01)
        act, coef = engine.policy_samples()
        feats = engine.debug_get_policy_features()
        T, n = spec.n_steps, sc.n
        rows_x = feats[:T].reshape(T * n, 64)
        g2 = engine.mlp_backward(rows_x, act.reshape(-1), np.tile(coef, T))
    finally:
        assert fn(engine.ctx, 0) == 0
    assert len(np.unique(coef)) > n // 2  # really one factor per scenario
    for k in g:
        assert np.array_equal(g[k], g2[k]), k
        assert rel_err(g[k], whole[k]) <= 1e-5, k
    # a factor taken from the wrong scenario is far outside that: the same rows
    # with the factors shifted by one scenario
    g3 = engine.mlp_backward(rows_x, act.reshape(-1), np.tile(np.roll(coef, 1), T))
    assert max(rel_err(g3[k], whole[k]) for k in g) > 0.1


def test_policy_sampling_equals_its_restatement(engine):
    """Every sampled bin of a 4,096 x 30 loop against policy_sample restated in
    numpy (mlp_ref.sample_bins) on the logits of mlp_kernel (the loop's MLP,
    bit for bit) and the oracle's Philox uniforms. Bins are equal except where
    u * sum lies within 1e-6 relative of a partial sum (the device expf against
    numpy's), and those are at most 0.1 % of the samples (expected: a 24-bit
    uniform against 7 edges 2e-6 wide, about 1.4e-5 per sample, 2 of 122,880).
    Measured on an MI355X: 0 of 122,880 within that distance, no bin differing."""
    from test_gpu_mlp import run_forward
    spec, sc, load = _loop_case(n=4096, T=30)
    ws, bs = configs.mlp_weights(11)
    ws[2] = ws[2] * 4.0  # sharper logits: a non-uniform policy
    engine.set_world(spec)
    engine.set_scenarios(sc)
    engine.set_load(load)
    engine.mlp_set_weights([configs.to_bf16_bits(w) for w in ws], bs)
    engine.policy_grad(seed=9)
    act, _ = engine.policy_samples()
    feats = engine.debug_get_policy_features()
    ids = sc.first_id + np.arange(sc.n)
    n_near = 0
    for t in range(spec.n_steps):
        y = run_forward(engine, feats[t], 32)
        want, near = mlp_ref.sample_bins(y, po.policy_uniform(9, ids, t))
        bad = (want != act[t]) & ~near
        assert not bad.any(), f"step {t}: scenarios {np.nonzero(bad)[0][:8].tolist()} sampled another bin"
        n_near += int(near.sum())
    print(f"samples within 1e-6 of a bin edge: {n_near} of {act.size}")
    assert n_near <= 1e-3 * act.size
    assert len(np.unique(act)) == 8


def test_gradient_steps_lower_the_objective(engine):
    """Plain gradient descent on E[J] (config 2, 2048 scenarios x 120 steps,
    cost + 0.02 $ per SLO-minute): the mean objective after a few steps is
    below the first one's."""
    spec, sc, load = _loop_case(n=2048, T=120)
    ws, bs = configs.mlp_weights(11)
    engine.set_world(spec)
    engine.set_scenarios(sc)
    engine.set_load(load)
    objs = []
    lr = 0.5
    for it in range(6):
        engine.mlp_set_weights([configs.to_bf16_bits(w) for w in ws], bs)
        g, obj = engine.policy_grad(seed=1000 + it, w_slo=0.02)
        objs.append(obj)
        ws = [ws[0] - lr * g["w1"], ws[1] - lr * g["w2"], ws[2] - lr * g["w3"]]
        bs = [bs[0] - lr * g["b1"], bs[1] - lr * g["b2"], bs[2] - lr * g["b3"]]
    assert min(objs[-2:]) < objs[0], objs
