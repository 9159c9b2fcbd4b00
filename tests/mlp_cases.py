"""The synthetic networks of the MLP shape tests (tests/test_gpu_mlp_shapes.py), shared with the CPU tests that pin the
oracle they are compared with (tests/test_mlp_shapes_host.py) and with the fixture generator
(tests/golden/make_mlp_golden.py).

The five shipped models are 18-58-58-256, 18-16-16-256, 7-16-16-224 (twice) and 18-64-64-256, all softsign, softsign,
linear: three of the eight compiled (K1S, H1T, H2T) instances of mlp_pair_kernel, one activation set, no generic
kernel.  CASES holds the smallest shapes that reach every other path of csrc/kernels_nn.hip:

  * every compiled instance, once with all hidden widths equal (what the reference's output_sgemm_flat can run, so the
    oracle is pinned to it bit for bit) and once with h1 != h2 and widths that are no multiple of the 16-unit tile;
    each with softsign, softsign, linear (the inlined activation set) and with a set taken by runtime code;
  * the generic kernel: 1, 2, 5 and 7 layers, hidden widths above 128;
  * three-layer networks that have a packed image but no compiled instance (rrtmgpnn_network_forward runs them on the
    generic kernel).

A case is reproducible from its seed alone: make_model(dims, acts, seed).  mlp_f64 is the independent check of the
oracle where the reference cannot run (unequal widths, one layer, tanh, gaussian): a float64 forward pass with a running
forward error bound of the float32 evaluation.
"""
import collections

import numpy as np

LINEAR, SOFTSIGN, RELU, SIGMOID, HARD_SIGMOID, TANH, GAUSSIAN = range(7)
ACT_NAMES = ("linear", "softsign", "relu", "sigmoid", "hard_sigmoid", "tanh", "gaussian")
# Lipschitz constants: max |f'| = 1 (linear, relu, softsign, tanh), 1/4 (sigmoid), 0.2 (hard_sigmoid),
# sqrt(2/e) = 0.858 (gaussian exp(-x^2))
LIPSCHITZ = (1.0, 1.0, 1.0, 0.25, 0.2, 1.0, 0.86)
SSL = (SOFTSIGN, SOFTSIGN, LINEAR)  # the shipped models' set: the ACTS == 1 instances (div_softsign)
ACTS0 = ((RELU, SIGMOID, HARD_SIGMOID), (SIGMOID, RELU, SOFTSIGN), (HARD_SIGMOID, LINEAR, RELU))  # ACTS == 0 sets
GTS = (GAUSSIAN, TANH, SIGMOID)
U = 2.0 ** -24  # float32 unit roundoff

# the compiled instances of mlp_pair_kernel (RRTMGPNN_MLP_SHAPES) and the LDS the packed image may take
MFMA_SHAPES = ((2, 1, 1), (2, 2, 2), (5, 1, 1), (5, 2, 2), (5, 3, 3), (5, 4, 4), (5, 5, 5), (5, 8, 8))
LDS_BYTES = 160 * 1024
MAX_INPUTS, MAX_MFMA_HIDDEN = 32, 128

Case = collections.namedtuple("Case", "name dims acts seed flat ref_ok path")


def act_f64(code, z):
    if code == SOFTSIGN:
        return z / (np.abs(z) + 1.0)
    if code == RELU:
        return np.maximum(0.0, z)
    if code == SIGMOID:
        return 1.0 / (1.0 + np.exp(-z))
    if code == HARD_SIGMOID:
        return np.maximum(0.0, np.minimum(1.0, 0.2 * z + 0.5))
    if code == TANH:
        return np.tanh(z)
    if code == GAUSSIAN:
        return np.exp(-z * z)
    return z


def gamma(k):
    return k * U / (1.0 - k * U)


def mlp_f64(model, x):
    """(y, err): the float64 forward pass of `model` on x (nbatch, nx), and a bound on |float32 evaluation - y|.

    Per layer with K inputs, for the float32 fmaf chain over k plus the bias add (K + 1 roundings; K + 2 leaves one
    u |z| for the activation's argument, see below):
        err_out = gamma(K + 2) (|W|^T |a| + |b|) + |W|^T err_in
    then through the activation: err_out * its Lipschitz constant + 4u |value| for the activation's own float32
    evaluation (an expf or tanhf within 2 ulp, an add and a division).  gaussian squares its argument first, which moves
    the value by at most u z^2 exp(-z^2) <= 0.43 u |z|: inside the spare u |z| of gamma(K + 2).
    A derived bound, not a tuned tolerance: an index or layout mistake is O(1) off."""
    dims = [int(v) for v in model["dims"]]
    a = np.asarray(x, np.float64).reshape(-1, dims[0])
    err = np.zeros_like(a)
    for n, code in enumerate(int(v) for v in model["activation"]):
        W = np.asarray(model["w%d" % (n + 1)], np.float64).reshape(dims[n], dims[n + 1])
        b = np.asarray(model["b%d" % (n + 1)], np.float64).ravel()
        z = a @ W + b
        e = gamma(dims[n] + 2) * (np.abs(a) @ np.abs(W) + np.abs(b)) + err @ np.abs(W)
        a = act_f64(code, z)
        err = LIPSCHITZ[code] * e + 4.0 * U * np.abs(a)
    return a, err


def make_model(dims, acts, seed, out_scaling=True):
    """The model dict the oracle, the reference harness and RrtmgpNetwork.from_arrays take: weights N(0, 1) / sqrt(fan
    in), biases N(0, 0.3), float32, from default_rng(seed).  The output scaling puts std * y + mean in about
    [0.2, 1.5] on inputs of [-0.2, 1.2] (mean 0.85, std 0.65 over 1.5 times the largest |y| of a 256-sample probe), so
    that pow8(.) * col_dry neither underflows nor overflows."""
    rng = np.random.default_rng(seed)
    dims = [int(d) for d in dims]
    m = {"dims": np.array(dims, np.int32), "activation": np.array(acts, np.int32),
         "input_min": np.zeros(dims[0], np.float32), "input_max": np.ones(dims[0], np.float32)}
    assert len(acts) == len(dims) - 1
    for n in range(1, len(dims)):
        m["w%d" % n] = (rng.standard_normal((dims[n - 1], dims[n])) / np.sqrt(dims[n - 1])).astype(np.float32)
        m["b%d" % n] = rng.normal(0.0, 0.3, dims[n]).astype(np.float32)
    if out_scaling:
        y, _ = mlp_f64(m, rng.uniform(-0.2, 1.2, (256, dims[0])).astype(np.float32))
        m["output_mean"] = np.full(dims[-1], 0.85, np.float32)
        m["output_std"] = (0.65 / (1.5 * np.abs(y).max(axis=0) + 1e-3)).astype(np.float32)
    return m


def inputs(dims, nbatch, seed):
    """x (nbatch, nx) uniform(-0.2, 1.2) with one row of zeros (the last, where there is more than one)."""
    x = np.random.default_rng(seed + 7919).uniform(-0.2, 1.2, (nbatch, int(dims[0]))).astype(np.float32)
    if nbatch > 1:
        x[-1] = 0.0
    return x


# ---- the pairs and single models of rrtmgpnn_predict_nn_lw / _sw (the last layer is linear there: output_sgemm_tau
# adds the bias and scales, "linear layer, no activation") ----
Pair = collections.namedtuple("Pair", "name mode ngpt a b acts_a acts_b path")
MIXED_A, MIXED_B = (RELU, SIGMOID, LINEAR), (HARD_SIGMOID, SOFTSIGN, LINEAR)


def _pairs():
    rows = [
        # LW pairs: absorption + Planck fraction
        ("lw", 36, (18, 58, 58), (18, 16, 16), (5, 4, 4, 5, 1, 1)),
        ("lw", 30, (18, 49, 64), (18, 3, 16), (5, 4, 4, 5, 1, 1)),
        ("lw", 32, (18, 65, 80), (18, 17, 32), (5, 5, 5, 5, 2, 2)),
        ("lw", 18, (18, 58, 58), (18, 32, 20), (5, 4, 4, 5, 2, 2)),
        # SW pairs: absorption + Rayleigh
        ("sw", 22, (7, 16, 16), (7, 9, 13), (2, 1, 1, 2, 1, 1)),
        ("sw", 32, (7, 20, 32), (7, 16, 16), (2, 2, 2, 2, 1, 1)),
        ("sw", 30, (8, 32, 17), (8, 17, 32), (2, 2, 2, 2, 2, 2)),
        # ssa == NULL: absorption alone (MLP_SW_ABS)
        ("sw_abs", 22, (7, 32, 32), None, (2, 2, 2, 0, 0, 0)),
        # nnets == 1: one model with 2 * ngpt outputs (MLP_LW_BOTH); ngpt 18: the group of four outputs 16..19 straddles
        # the tau / pfrac boundary
        ("lw_both", 18, (18, 58, 58), None, (5, 4, 4, 0, 0, 0)),
        ("lw_both", 20, (18, 64, 49), None, (5, 4, 4, 0, 0, 0)),
    ]
    out = []
    for mode, ngpt, a, b, path in rows:
        ny = 2 * ngpt if mode == "lw_both" else ngpt
        for tag, aa, ab in (("ssl", SSL, SSL), ("mixed", MIXED_A, MIXED_B)):
            name = "%s-g%d-%s%s-%s" % (mode, ngpt, "x".join(map(str, a)), "+" + "x".join(map(str, b)) if b else "", tag)
            out.append(Pair(name, mode, ngpt, a + (ny,), b + (ny,) if b else None, aa, ab, path))
    return tuple(out)


PAIRS = _pairs()
PAIR_NBATCH = (1, 17, 50)


def pair_models(p):
    seed = 5000 + PAIRS.index(p) * 2
    return make_model(p.a, p.acts_a, seed), (make_model(p.b, p.acts_b, seed + 1) if p.b else None)


def expected_path(dims):
    """The kernel rrtmgpnn_network_forward serves a network with, from the rules of pack_network and launch_mlp:
    ("mfma", K1S, H1T, H2T) or ("generic",)."""
    dims = [int(d) for d in dims]
    if len(dims) != 4 or dims[0] > MAX_INPUTS or max(dims[1:3]) > MAX_MFMA_HIDDEN:
        return ("generic",)
    k, h1, h2, ngt = (dims[0] + 3) // 4, (dims[1] + 15) // 16, (dims[2] + 15) // 16, (dims[3] + 15) // 16
    floats = h1 * k * 64 + h2 * h1 * 256 + ngt * h2 * 256 + 16 * (h1 + h2) + 48 * ngt  # img_layout
    if (k, h1, h2) in MFMA_SHAPES and 4 * floats <= LDS_BYTES:
        return ("mfma", k, h1, h2)
    return ("generic",)


def is_flat(dims):
    return len(set(int(d) for d in dims[1:-1])) <= 1


def reference_can_run(dims, acts):
    """output_sgemm_flat: all hidden widths equal ("assumes a flat network"), at least two layers (one layer crashes
    the harness), activations linear..hard_sigmoid (set_activation leaves bias_and_activation null for tanh and
    gaussian)."""
    return is_flat(dims) and len(dims) - 1 >= 2 and all(0 <= a <= HARD_SIGMOID for a in acts)


def mfma(k, h1, h2):
    return ("mfma", k, h1, h2)


GENERIC = ("generic",)

# (instance, flat dims, dims with h1 != h2)
MFMA_TABLE = (
    ((2, 1, 1), (7, 16, 16, 224), (5, 9, 13, 23)),
    ((2, 2, 2), (8, 32, 32, 36), (8, 17, 32, 36)),
    ((5, 1, 1), (18, 16, 16, 256), (17, 3, 16, 20)),
    ((5, 2, 2), (20, 32, 32, 64), (20, 32, 17, 64)),
    ((5, 3, 3), (18, 33, 33, 50), (18, 33, 48, 50)),
    ((5, 4, 4), (18, 58, 58, 256), (18, 49, 64, 130)),
    ((5, 5, 5), (19, 80, 80, 250), (19, 80, 65, 250)),
    ((5, 8, 8), (18, 128, 128, 40), (18, 128, 113, 40)),
)
GENERIC_TABLE = (
    ((4, 6), (TANH,)),
    ((4, 8, 6), (RELU, SIGMOID)),
    ((32, 64, 64, 64, 64, 10), (SOFTSIGN, RELU, HARD_SIGMOID, SIGMOID, LINEAR)),
    ((18, 58, 58, 58, 58, 58, 58, 256), (RELU, SOFTSIGN, SIGMOID, HARD_SIGMOID, SOFTSIGN, RELU, LINEAR)),
    ((18, 256, 256, 40), (SIGMOID, SOFTSIGN, LINEAR)),
    ((18, 256, 200, 40), (GAUSSIAN, TANH, RELU)),
)
# three layers and a packed image, but no compiled instance: nx of 9..16 and of 1..4, unequal tile counts, an image
# over 160 KiB of LDS
NO_INSTANCE_TABLE = (
    ((9, 100, 100, 30), SSL),
    ((3, 16, 16, 5), (RELU, SIGMOID, HARD_SIGMOID)),
    ((18, 96, 16, 8), (TANH, GAUSSIAN, LINEAR)),
    ((18, 128, 128, 256), SSL),
)
GTS_ROWS = ((5, 3, 3), (5, 8, 8))  # the h1 != h2 cases that also run gaussian, tanh, sigmoid


def _name(dims, acts):
    return "-".join(str(d) for d in dims) + ":" + ",".join(ACT_NAMES[a] for a in acts)


def _build():
    cases = []

    def add(dims, acts, path):
        cases.append(Case(_name(dims, acts), tuple(dims), tuple(acts), 1000 + len(cases), is_flat(dims),
                          reference_can_run(dims, acts), path))

    i = 0
    for inst, flat, uneq in MFMA_TABLE:
        for dims in (flat, uneq):
            add(dims, SSL, mfma(*inst))
            add(dims, ACTS0[i % len(ACTS0)], mfma(*inst))
            i += 1
        if inst in GTS_ROWS:
            add(uneq, GTS, mfma(*inst))
    for dims, acts in GENERIC_TABLE + NO_INSTANCE_TABLE:
        add(dims, acts, GENERIC)
    return tuple(cases)


CASES = _build()
BY_NAME = {c.name: c for c in CASES}
MFMA_CASES = tuple(c for c in CASES if c.path != GENERIC)
GENERIC_CASES = tuple(c for c in CASES if c.path == GENERIC and (c.dims, c.acts) in GENERIC_TABLE)
NO_INSTANCE_CASES = tuple(c for c in CASES if (c.dims, c.acts) in NO_INSTANCE_TABLE)
REF_CASES = tuple(c for c in CASES if c.ref_ok)
NBATCH = 17          # the batch of the fixture and of the host comparisons
NBATCH_LARGE = 1500


def model_of(case, out_scaling=True):
    return make_model(case.dims, case.acts, case.seed, out_scaling)


def ulp_distance(a, b):
    """Largest distance in float32 ulps between two arrays of finite values (for a finding's record)."""
    def key(v):
        i = np.ascontiguousarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return int(np.abs(key(a) - key(b)).max()) if np.size(a) else 0
