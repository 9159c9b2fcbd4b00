"""CPU: what the GPU MLP shape tests (tests/test_gpu_mlp_shapes.py) compare with is itself pinned.

  * Oracle.mlp lies inside mlp_f64's running float32 error bound on every case of tests/mlp_cases.py -- the only
    independent check where the reference cannot run (unequal hidden widths, one layer, tanh, gaussian);
  * Oracle.mlp equals the reference's network_type%output_sgemm_flat (MKL sgemm) bit for bit on every case the
    reference can run, at nbatch 17 and 1500 (where oracle/_ref is built), and equals the recorded outputs of that
    library in tests/golden/mlp_shapes.npz everywhere;
  * the reference's sgemm gives each sample the same bits wherever it stands in a batch of 17 (nbatch == 1 is another
    code path of the BLAS and differs by up to tens of ulp: DESIGN.md section 4; not asserted, it is the BLAS's).
"""
import os

import numpy as np
import pytest

import mlp_cases as M

HERE = os.path.dirname(os.path.abspath(__file__))
REF_SO = os.path.join(os.path.dirname(HERE), "oracle", "_ref", "librrtmgp_ref.so")
GOLD = os.path.join(HERE, "golden", "mlp_shapes.npz")
needs_ref = pytest.mark.skipif(not os.path.exists(REF_SO), reason="reference oracle not built (oracle/Makefile.ref)")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def ref():
    import oracle as O
    return O.Reference()


def test_case_table_is_what_the_issue_lists():
    names = [c.name for c in M.CASES]
    assert len(set(names)) == len(names)
    assert len(M.MFMA_CASES) == 8 * 2 * 2 + 2 and len(M.GENERIC_CASES) == 6 and len(M.NO_INSTANCE_CASES) == 4
    assert {c.path[1:] for c in M.MFMA_CASES} == set(M.MFMA_SHAPES)
    for c in M.CASES:
        assert c.path == M.expected_path(c.dims), c.name
        assert c.flat == M.is_flat(c.dims) and c.ref_ok == M.reference_can_run(c.dims, c.acts), c.name
    for inst in M.MFMA_SHAPES:  # per instance: flat and h1 != h2, the inlined set and a runtime set
        rows = [c for c in M.MFMA_CASES if c.path[1:] == inst]
        assert {(c.flat, c.acts == M.SSL) for c in rows} == {(f, s) for f in (True, False) for s in (True, False)}
    used = {a for c in M.CASES for a in c.acts}
    assert used == set(range(7))
    # every no-instance case has a packed image (3 layers, nx <= 32, hidden <= 128) and still no kernel
    for c in M.NO_INSTANCE_CASES:
        assert len(c.dims) == 4 and c.dims[0] <= M.MAX_INPUTS and max(c.dims[1:3]) <= M.MAX_MFMA_HIDDEN


def test_make_model_is_reproducible_and_scaled():
    c = M.BY_NAME["18-49-64-130:softsign,softsign,linear"]
    a, b = M.model_of(c), M.model_of(c)
    assert sorted(a) == sorted(b)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])
        assert a[k].dtype in (np.float32, np.int32)
    assert a["w2"].shape == (49, 64) and a["b3"].shape == (130,)
    y, _ = M.mlp_f64(a, M.inputs(c.dims, 200, 5))
    t = a["output_std"] * y + a["output_mean"]
    assert 0.2 - 0.15 < t.min() and t.max() < 1.5 + 0.15  # "about": unseen samples may pass the probe's largest |y|


def test_error_bound_is_small_and_sees_a_swapped_unit():
    """The bound is of float32 rounding size, far below what an index mistake moves the outputs by."""
    c = M.BY_NAME["18-49-64-130:softsign,softsign,linear"]
    m = M.model_of(c)
    x = M.inputs(c.dims, M.NBATCH, c.seed)
    y, err = M.mlp_f64(m, x)
    assert err.max() < 1e-3
    wrong = dict(m, b1=m["b1"][::-1].copy())
    y2, _ = M.mlp_f64(wrong, x)
    assert (np.abs(y2 - y) > 100 * err).mean() > 0.9


@pytest.mark.parametrize("case", M.CASES, ids=lambda c: c.name)
def test_oracle_within_f64_bound(orc, case):
    m = M.model_of(case)
    x = M.inputs(case.dims, M.NBATCH, case.seed)
    y, err = M.mlp_f64(m, x)
    got = orc.mlp(m, x)
    assert got.shape == y.shape and np.isfinite(got).all()
    d = np.abs(got.astype(np.float64) - y)
    print("%s: max |oracle - f64| %.3g, bound there %.3g, worst ratio %.3g"
          % (case.name, d.max(), err.ravel()[d.argmax()], (d / np.maximum(err, 1e-300)).max()))
    assert (d <= err).all()


@needs_ref
@pytest.mark.parametrize("nbatch", [M.NBATCH, M.NBATCH_LARGE])
@pytest.mark.parametrize("case", M.REF_CASES, ids=lambda c: c.name)
def test_oracle_bitwise_vs_reference(orc, ref, case, nbatch):
    m = M.model_of(case)
    x = M.inputs(case.dims, nbatch, case.seed)
    want = ref.mlp(m, x)
    got = orc.mlp(m, x)
    print("%s nbatch %d: max ulp distance %d" % (case.name, nbatch, M.ulp_distance(got, want)))
    np.testing.assert_array_equal(bits(got), bits(want))


def test_oracle_bitwise_vs_reference_fixture(orc):
    """tests/golden/mlp_shapes.npz: the reference library's outputs at nbatch 17 (tests/golden/make_mlp_golden.py);
    what pins the oracle on these shapes where oracle/_ref is absent."""
    gold = np.load(GOLD)
    assert sorted(gold["names"].tolist()) == sorted(c.name for c in M.REF_CASES)
    for name, seed in zip(gold["names"].tolist(), gold["seeds"].tolist()):
        case = M.BY_NAME[name]
        assert case.seed == seed and int(gold["nbatch"]) == M.NBATCH
        got = orc.mlp(M.model_of(case), M.inputs(case.dims, M.NBATCH, case.seed))
        np.testing.assert_array_equal(bits(got), bits(gold["y:" + name]), err_msg=name)


@needs_ref
@pytest.mark.parametrize("name", ["18-58-58-256:softsign,softsign,linear", "8-32-32-36:hard_sigmoid,linear,relu",
                                  "32-64-64-64-64-10:softsign,relu,hard_sigmoid,sigmoid,linear"])
def test_reference_sample_bits_do_not_depend_on_the_column(ref, name):
    """A sample's outputs from a batch of 17 are the same bits in whichever column it stands: 17 evaluations with the
    columns rotated.  (The ascending-k order of the oracle is what the BLAS gives for nbatch >= 2.)"""
    case = M.BY_NAME[name]
    m = M.model_of(case)
    x = M.inputs(case.dims, M.NBATCH, case.seed)
    want = ref.mlp(m, x)
    for shift in range(1, M.NBATCH):
        perm = np.roll(np.arange(M.NBATCH), shift)
        got = ref.mlp(m, np.ascontiguousarray(x[perm]))
        np.testing.assert_array_equal(bits(got), bits(want[perm]), err_msg="shift %d" % shift)


def test_lw_both_straddle_indices():
    """The expected split of a single model's 2*ngpt outputs, as the GPU test forms it (Oracle.both_post): output g of
    [ngpt, 2 ngpt) is pfrac[g - ngpt].  With ngpt = 18 the group of four outputs 16..19 holds tau 16, 17 and pfrac 0, 1:
    an index that forgets `- ngpt` would put them at pfrac 18, 19 (the next sample's tau region is never theirs)."""
    import oracle as O
    orc = O.Oracle()
    ngpt, nb = 18, 3
    y = np.arange(nb * 2 * ngpt, dtype=np.float32).reshape(nb, 2 * ngpt) / 64
    m = {"output_mean": np.zeros(2 * ngpt, np.float32), "output_std": np.ones(2 * ngpt, np.float32)}
    tau, pf = orc.both_post(m, y, np.ones(nb, np.float32))
    np.testing.assert_array_equal(pf, y[:, ngpt:] ** 2)
    t2 = y[:, :ngpt] * y[:, :ngpt]
    t4 = t2 * t2
    np.testing.assert_array_equal(tau, t4 * t4)
    # the mutated index: g instead of g - ngpt, flat offset s * ngpt + g
    g = np.arange(ngpt, 2 * ngpt)
    right = (np.arange(nb)[:, None] * ngpt + (g - ngpt)[None, :]).ravel()
    wrong = (np.arange(nb)[:, None] * ngpt + g[None, :]).ravel()
    assert not np.intersect1d(right[:2], wrong[:2]).size and (wrong != right).all()
