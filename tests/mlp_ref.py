"""Plain references for the learned policy's kernels (SEMANTICS 5), shared by
test_mlp_exact_data.py (CPU), test_gpu_mlp.py, test_gpu_pg.py and
test_policy_rollout.py. Nothing here touches the GPU.

* forward / backward: the MLP 64 -> 256 -> 256 -> 8 and the score-function
  backward restated in numpy float64, optionally rounding to bf16 (nearest
  even) at exactly the kernels' MFMA operand points: h1, h2, g, dH2, dH1.
* backward_f32: the same restatement with fp32 arithmetic (PyTorch, CPU), the
  yardstick for what fp32 accumulation alone costs.
* decode_work: the backward's row-blocked work arrays (pg.hip, rb_off).
* exact_case: inputs on which the whole backward is exact in bf16 and fp32, so
  the GPU can be held to equality with the float64 reference.
* gen_states: mlp_gen_states_kernel restated (numpy Philox-4x32-10).
* sample_bins: policy_sample restated.
"""
import functools

import numpy as np

from ccka import configs

IN, HID, OUT = 64, 256, 8
WORK_UNITS = (("x", IN), ("h1", HID), ("h2", HID), ("dh1", HID), ("dh2", HID), ("g", OUT))
WORK_ROWS = sum(u for _, u in WORK_UNITS)  # bf16 elements per row of the work buffer
GRADS = ("w1", "b1", "w2", "b2", "w3", "b3")


def bf16_round(a):
    """Nearest-even rounding to bf16 (through fp32, as the kernels' fp32 sums are), as float64."""
    return configs.from_bf16_bits(configs.to_bf16_bits(np.asarray(a, np.float32))).astype(np.float64)


def is_bf16(a) -> bool:
    """Every element is a bf16 value: exact in fp32 with the low 16 bits zero."""
    a = np.asarray(a)
    f = np.ascontiguousarray(a, np.float32)
    return bool(np.array_equal(f.astype(np.float64), a.astype(np.float64)) and not (f.view(np.uint32) & 0xFFFF).any())


def bits(a) -> np.ndarray:
    """bf16 bit patterns of bf16-representable values, zeros as +0."""
    return configs.to_bf16_bits(np.asarray(a, np.float32) + np.float32(0.0))


def forward(x, ws, bs, round_bf16=True):
    """(h1, h2, y) in float64."""
    rnd = bf16_round if round_bf16 else (lambda a: a)
    x, (w1, w2, w3), (b1, b2, b3) = np.asarray(x, np.float64), [np.asarray(w, np.float64) for w in ws], \
        [np.asarray(b, np.float64) for b in bs]
    h1 = np.maximum(rnd(x @ w1 + b1), 0.0)
    h2 = np.maximum(rnd(h1 @ w2 + b2), 0.0)
    return h1, h2, h2 @ w3 + b3


def backward(x, act, coef, ws, bs, round_bf16=False):
    """Gradient of sum_m coef[m] log softmax(y_m)[act_m] in float64: a dict with
    h1, h2, y, g, dh2, dh1 ([rows][units]) and the six gradients w1 .. b3."""
    rnd = bf16_round if round_bf16 else (lambda a: a)
    x = np.asarray(x, np.float64)
    w1, w2, w3 = (np.asarray(w, np.float64) for w in ws)
    h1, h2, y = forward(x, ws, bs, round_bf16)
    e = np.exp(y - y.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    onehot = np.zeros_like(p)
    onehot[np.arange(len(x)), np.asarray(act, np.int64)] = 1.0
    g = rnd(np.asarray(coef, np.float64)[:, None] * (onehot - p))
    dh2 = rnd(np.where(h2 > 0, g @ w3.T, 0.0))
    dh1 = rnd(np.where(h1 > 0, dh2 @ w2.T, 0.0))
    return {"h1": h1, "h2": h2, "y": y, "g": g, "dh2": dh2, "dh1": dh1,
            "w1": x.T @ dh1, "b1": dh1.sum(0), "w2": h1.T @ dh2, "b2": dh2.sum(0), "w3": h2.T @ g, "b3": g.sum(0)}


def backward_f32(x, act, coef, ws, bs):
    """backward(round_bf16=True) with every product, sum and the softmax in
    fp32 (PyTorch on the CPU): the six gradients as float32 arrays."""
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))  # noqa: E731
    rnd = lambda a: a.to(torch.bfloat16).float()  # noqa: E731
    x, (w1, w2, w3), (b1, b2, b3) = t(x), [t(w) for w in ws], [t(b) for b in bs]
    h1 = torch.relu(rnd(x @ w1 + b1))
    h2 = torch.relu(rnd(h1 @ w2 + b2))
    p = torch.softmax(h2 @ w3 + b3, dim=1)
    onehot = torch.nn.functional.one_hot(torch.from_numpy(np.asarray(act, np.int64)), OUT).float()
    g = rnd(t(coef)[:, None] * (onehot - p))
    dh2 = rnd((g @ w3.T) * (h2 > 0))
    dh1 = rnd((dh2 @ w2.T) * (h1 > 0))
    out = {"w1": x.T @ dh1, "b1": dh1.sum(0), "w2": h1.T @ dh2, "b2": dh2.sum(0), "w3": h2.T @ g, "b3": g.sum(0)}
    return {k: v.numpy() for k, v in out.items()}


def column_errors(got, want):
    """Relative L2 error per hidden unit: per column of dW1, dW2, db1 and db2
    (the unit the gradient flows into), per row of dW3 (the unit it flows out
    of), so one wrong unit cannot hide in the array's norm. {name: [units]}."""
    out = {}
    for k in ("w1", "w2", "w3", "b1", "b2"):
        g, w = np.asarray(got[k], np.float64), np.asarray(want[k], np.float64)
        if k == "w3":
            g, w = g.T, w.T
        g, w = g.reshape(-1, g.shape[-1]), w.reshape(-1, w.shape[-1])
        out[k] = np.linalg.norm(g - w, axis=0) / np.maximum(np.linalg.norm(w, axis=0), 1e-300)
    return out


def mpad(m: int) -> int:
    """Rows of the work arrays of an m-row backward (pg_rows_kernel's 32-row tiles)."""
    return (m + 31) // 32 * 32


def wgrad_splits(mp):
    """(splits, rows per split) of the weight-gradient kernels on an Mpad-row
    chunk, re-derived from the sources' own constant and formulas (kPgSplits
    and pg_backward in abi_policy.cpp, the kernels' chunk in pg.hip)."""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(configs.__file__))), "csrc")
    src = open(os.path.join(csrc, "abi_policy.cpp")).read()
    k = int(re.search(r"kPgSplits\s*=\s*(\d+)\s*;", src).group(1))
    # the two formulas restated below, as the sources spell them
    assert "std::min<int64_t>(kPgSplits, Mpad / 256)" in src
    assert "(q.Mpad / 16 + q.splits - 1) / q.splits * 16" in open(os.path.join(csrc, "pg.hip")).read()
    splits = max(1, min(k, mp // 256))
    return splits, (mp // 16 + splits - 1) // splits * 16


def own_operand_errors(got, work, m):
    """The weight-gradient kernels against the float64 sums of the operands
    they read (the decoded work arrays of the same backward, rows 0..m-1): per
    hidden unit, the L2 norm of (got - sum) over the unit's column divided by
    the L2 norm of the column of sum |a| |b|, the scale an fp32 summation
    error is bounded by whatever the cancellation. {name: [units]} as
    column_errors, plus b3 per action."""
    f = {k: configs.from_bf16_bits(v[:m]).astype(np.float64) for k, v in work.items()}
    ones = np.ones((m, 1))
    out = {}
    for k, a, b in (("w1", f["x"], f["dh1"]), ("w2", f["h1"], f["dh2"]), ("w3", f["h2"], f["g"]),
                    ("b1", ones, f["dh1"]), ("b2", ones, f["dh2"]), ("b3", ones, f["g"])):
        d = np.asarray(got[k], np.float64).reshape(a.shape[1], b.shape[1]) - a.T @ b
        scale = np.abs(a).T @ np.abs(b)
        ax = 1 if k == "w3" else 0
        out[k] = np.linalg.norm(d, axis=ax) / np.maximum(np.linalg.norm(scale, axis=ax), 1e-300)
    return out


def decode_work(buf, mp):
    """The work buffer xT | h1T | h2T | dh1T | dh2T | gyT of a backward with
    Mpad = mp as six uint16 arrays [mp][units]: element (unit u, row m) of a
    U-unit array sits at ((m >> 4) * U + u) * 16 + (m & 15) (pg.hip, rb_off)."""
    buf = np.asarray(buf, np.uint16).reshape(-1)
    assert mp % 16 == 0 and buf.size >= WORK_ROWS * mp
    out, off = {}, 0
    for name, u in WORK_UNITS:
        out[name] = buf[off:off + u * mp].reshape(mp // 16, u, 16).transpose(0, 2, 1).reshape(mp, u).copy()
        off += u * mp
    return out


def encode_work(arrays, mp):
    """Inverse of decode_work, written from rb_off element by element (the
    layout's statement; test_mlp_exact_data checks the two against each other)."""
    buf = np.zeros(WORK_ROWS * mp, np.uint16)
    off = 0
    m = np.arange(mp)[:, None]
    for name, u in WORK_UNITS:
        idx = ((m >> 4) * u + np.arange(u)[None, :]) * 16 + (m & 15)
        buf[off + idx] = arrays[name]
        off += u * mp
    return buf


def _swap_rows(w):
    h = w.shape[0] // 2
    return np.concatenate([w[h:], w[:h]], axis=0)


def exact_weights(seed, k3=True):
    """The weights of exact_case(seed, .) (they do not depend on the row count)."""
    rng = np.random.default_rng([seed, 0xE7AC])
    w1h = rng.integers(-1, 2, size=(IN, HID // 2))
    b1h = rng.integers(-3, 4, size=HID // 2)
    w2h = rng.integers(-1, 2, size=(HID, HID // 2)) * (rng.random((HID, HID // 2)) < 0.03)
    b2h = rng.integers(-2, 3, size=HID // 2)
    w3h = rng.integers(-2, 3, size=(HID // 2, OUT))
    k = rng.integers(-1, 2, size=(HID // 2, 1)) * (1 if k3 else 0)
    b3 = np.full(OUT, rng.integers(-3, 4))
    ws = [np.concatenate([w1h, _swap_rows(w1h)], axis=1), np.concatenate([w2h, _swap_rows(w2h)], axis=1),
          np.concatenate([w3h, -w3h + k], axis=0)]
    bs = [np.concatenate([b1h, b1h]), np.concatenate([b2h, b2h]), b3]
    return [w.astype(np.float32) for w in ws], [b.astype(np.float32) for b in bs]


@functools.lru_cache(maxsize=None)
def exact_case(seed, m, k3=True):
    """Inputs on which forward and backward are exact in bf16 and fp32.

    x = [xh | xh] with xh in {-1, 0, 1}; W1 = [w1h | swap_rows(w1h)] and
    W2 = [w2h | swap_rows(w2h)] (3 % dense) with the biases repeated, so on this
    data h1[:, v + 128] = h1[:, v] and h2[:, u + 128] = h2[:, u] although the
    function is not symmetric; W3 = [w3h ; -w3h + k] (k a per-unit integer over
    all 8 actions; k3=False: k = 0) and b3 one constant, so a row's 8 logits
    are equal: softmax = 1/8 exactly, g = c (e_a - 1/8) with c = +-2^-j is a
    bf16 value, and dH2, dH1 and the gradients are small dyadic rationals whose
    sums are exact in any fp32 order (test_mlp_exact_data.py holds every
    precondition). Above 20,000 rows the coefficients are +-1 only.

    Returns a dict: x (float32 [m][64]), act (uint8), coef (float32), ws, bs
    (float32), unit (the smallest unit present in the backward's values) and
    ref (backward() in float64 without rounding). Treat it as read-only."""
    ws, bs = exact_weights(seed, k3)
    rng = np.random.default_rng([seed, m])
    xh = rng.integers(-1, 2, size=(m, IN // 2))
    x = np.concatenate([xh, xh], axis=1).astype(np.float32)
    act = rng.integers(0, OUT, size=m).astype(np.uint8)
    jmax = 2 if m <= 20000 else 0
    coef = (rng.choice([-1.0, 1.0], size=m) * 0.5 ** rng.integers(0, jmax + 1, size=m)).astype(np.float32)
    ref = backward(x, act, coef, ws, bs, round_bf16=False)
    case = {"x": x, "act": act, "coef": coef, "ws": ws, "bs": bs, "unit": 0.5 ** (jmax + 3), "ref": ref}
    for a in (x, act, coef, *ws, *bs, *ref.values()):
        a.setflags(write=False)
    return case


# the (seed, rows) of the GPU files' exact cases: test_mlp_exact_data.py checks the preconditions of each
PG_EXACT_ROWS = (1, 31, 32, 33, 255, 257, 511, 513, 1189, 4865, 20000)
EXACT_CASES = tuple((0, m) for m in PG_EXACT_ROWS) + ((1, 1189),)


def philox(c0, c1, c2, c3, k0, k1):
    """Philox-4x32-10 (SEMANTICS 4) on uint32 arrays: the four output words."""
    c = [np.asarray(v, np.uint64) & 0xFFFFFFFF for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(0xFFFFFFFF),
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(0xFFFFFFFF)]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def gen_states(n, seed):
    """mlp_gen_states_kernel (mlp.hip) restated: element e of the [n][64] states
    is the Irwin-Hall sum of the top 16 bits of Philox(e lo, e hi, 0x5EED,
    0x57A7E; seed) in fp32 (the four terms and the offset are exact, the
    scaling rounds once), rounded to bf16. uint16 [n][64]."""
    e = np.arange(n * IN, dtype=np.uint64)
    u = philox(e & np.uint64(0xFFFFFFFF), e >> np.uint64(32), 0x5EED, 0x57A7E, seed & 0xFFFFFFFF, seed >> 32)
    s = np.float32(0.0)
    for w in u:
        s = s + (w >> 16).astype(np.float32)
    v = (s - np.float32(131070.0)) * (np.float32(1.0) / np.float32(37837.0))
    return configs.to_bf16_bits(v).reshape(n, IN)


def sample_bins(y, u, rel=1e-6):
    """policy_sample (mlp_dev.h) restated on logits y [n][8] (fp32) and uniforms
    u [n] (k / 2^24): the softmax numerators exp(y - max) and their running sum
    in fp32, in action order; the bin is the first a with u * sum < p_0 + ... +
    p_a, the last one if there is none. Float64 is the arbiter of which samples
    an expf differing in the last bits could move: near[i] is set where u * sum
    lies within `rel` relative of one of the seven inner partial sums.
    (bins int64, near bool)."""
    y = np.asarray(y, np.float32)
    n = len(y)
    d = y - y.max(axis=1, keepdims=True)
    p = np.exp(d, dtype=np.float32)
    acc = np.zeros((n, OUT), np.float32)
    s = np.zeros(n, np.float32)
    for a in range(OUT):
        s = s + p[:, a]
        acc[:, a] = s
    uf = (np.asarray(u, np.float64) * 16777216.0).astype(np.float32) * np.float32(1.0 / 16777216.0) * s
    below = uf[:, None] < acc
    bins = np.where(below.any(axis=1), below.argmax(axis=1), OUT - 1)
    p64 = np.exp(d.astype(np.float64))
    acc64 = np.cumsum(p64, axis=1)
    us = np.asarray(u, np.float64) * acc64[:, -1]
    edges = acc64[:, :OUT - 1]  # (the total is no edge: above it the last action is taken anyway)
    near = (np.abs(us[:, None] - edges) <= rel * edges).any(axis=1)
    return bins.astype(np.int64), near
