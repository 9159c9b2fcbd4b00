"""GPU: McICA cloud sampling with in-kernel random numbers (Philox4x32-10, counter-based, seeded), bit for bit.

* rrtmgpnn_mcica_randoms against the numpy restatement tests/philox_ref.py;
* the seeded mask kernels (bytes, bits, both) against the array entries run on rrtmgpnn_mcica_randoms' output, against
  tests/mcica_ref.py on the restated numbers, and against its packed form;
* a column's numbers depend on its global index only: 7 columns in one call against calls on [0, 3) and [3, 7);
* argument errors and the class layer's messages;
* ClearSkyStep(mcica={"seed": ...}) against the array route on the restated numbers and the composed oracle, a captured
  step replayed after set_mcica_seed, two half steps against the whole, fused=False, the refusals and the unchanged
  call lists of steps without a seed.
Cases and their non-vacuity: tests/mcica_seeded_cases.py (asserted on the CPU by tests/test_mcica_seeded_host.py)."""
import numpy as np
import pytest

import mcica_ref as M
import mcica_seeded_cases as C
import philox_ref as P

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
ERR_ARGUMENT = 1


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def T(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)


def _randoms_gpu(dev, seed, stream, col0, ngpt, nlay, ncol):
    from rrtmgpnn import cloud_sampling as cs
    r = torch.full((ncol, nlay, ngpt), float("nan"), device=dev)  # poisoned: every element must be written
    assert cs.mcica_randoms(seed, stream, col0, r) == ""
    torch.cuda.synchronize()
    return r


def _outputs(dev, ncol, nlay, ngpt, want_bytes, want_bits):
    """Poisoned outputs: every element must be written (the packed words' unused high bits with zeros)."""
    mb = torch.full((ncol, nlay, ngpt), 7, dtype=torch.uint8, device=dev) if want_bytes else None
    bits = torch.full((ncol, nlay, (ngpt + 31) // 32), -1, dtype=torch.int32, device=dev) if want_bits else None
    return mb, bits


def _np(mb, bits):
    torch.cuda.synchronize()
    return (None if mb is None else mb.cpu().numpy(), None if bits is None else bits.cpu().numpy().view(np.uint32))


def _seeded_gpu(dev, seed, stream, col0, ngpt, cf, ov, want_bytes=True, want_bits=True):
    from rrtmgpnn import cloud_sampling as cs
    ncol, nlay = cf.shape
    mb, bits = _outputs(dev, ncol, nlay, ngpt, want_bytes, want_bits)
    if ov is None:
        e = cs.sampled_mask_max_ran_seeded(seed, stream, col0, T(cf, dev), mb, bits, ngpt=ngpt)
    else:
        e = cs.sampled_mask_exp_ran_seeded(seed, stream, col0, T(cf, dev), T(ov, dev), mb, bits, ngpt=ngpt)
    assert e == ""
    return _np(mb, bits)


def _array_gpu(dev, r, cf, ov):
    from rrtmgpnn import cloud_sampling as cs
    ncol, nlay, ngpt = r.shape
    mb, bits = _outputs(dev, ncol, nlay, ngpt, True, True)
    if ov is None:
        e = cs.sampled_mask_max_ran(r, T(cf, dev), mb, bits)
    else:
        e = cs.sampled_mask_exp_ran(r, T(cf, dev), T(ov, dev), mb, bits)
    assert e == ""
    return _np(mb, bits)


@pytest.mark.parametrize("shape", C.CASES, ids=lambda s: "g%d-l%d" % s)
def test_mcica_randoms_match_restatement(dev, shape):
    ngpt, nlay = shape
    for ncol, col0, seed in C.combos():
        got = _randoms_gpu(dev, seed, C.STREAM, col0, ngpt, nlay, ncol).cpu().numpy()
        want = P.randoms(seed, C.STREAM, col0, ngpt, nlay, ncol)
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=str((ncol, col0, seed)))


@pytest.mark.parametrize("overlap", ["max_ran", "exp_ran"])
@pytest.mark.parametrize("shape", C.CASES, ids=lambda s: "g%d-l%d" % s)
def test_seeded_masks(dev, shape, overlap):
    ngpt, nlay = shape
    cloudy_elems = []
    for ncol, col0, seed in C.combos():
        cf, ov = C.inputs(ngpt, nlay, ncol)
        ov = ov if overlap == "exp_ran" else None
        what = str((ncol, col0, seed))
        want = C.want_mask(seed, col0, ngpt, cf, ov)  # mcica_ref.sampled_mask on philox_ref.randoms
        want_bits = M.pack_bits(want)
        # non-vacuity (tests/mcica_seeded_cases.py)
        if ngpt > 1:
            assert M.non_vacuity(want, M.bands(ngpt))[2] >= 1, what
        cloudy_elems.append(want[cf > 0].ravel())
        # the array entries on mcica_randoms' output
        arr_b, arr_w = _array_gpu(dev, _randoms_gpu(dev, seed, C.STREAM, col0, ngpt, nlay, ncol), cf, ov)
        np.testing.assert_array_equal(arr_b, want.astype(np.uint8), err_msg=what)
        np.testing.assert_array_equal(arr_w, want_bits, err_msg=what)
        for outputs in ("bytes", "bits", "both"):
            mb, bits = _seeded_gpu(dev, seed, C.STREAM, col0, ngpt, cf, ov, outputs != "bits", outputs != "bytes")
            assert (mb is None) == (outputs == "bits") and (bits is None) == (outputs == "bytes")
            if mb is not None:
                np.testing.assert_array_equal(mb, arr_b, err_msg=what + outputs)
                np.testing.assert_array_equal(mb, want.astype(np.uint8), err_msg=what + outputs)
            if bits is not None:
                np.testing.assert_array_equal(bits, arr_w, err_msg=what + outputs)
                np.testing.assert_array_equal(bits, want_bits, err_msg=what + outputs)
    e = np.concatenate(cloudy_elems)
    assert e.any() and not e.all()


@pytest.mark.parametrize("overlap", ["max_ran", "exp_ran"])
def test_decomposition_on_the_device(dev, overlap):
    """7 columns in one call equal calls on [0, 3) and [3, 7) with col0 = 3 (ngpt 40: a partial last word; 5 layers: a
    partial last group)."""
    ngpt, nlay, seed = 40, 5, C.SEEDS[1]
    _, cf, ov = M.build(ngpt, nlay, 7, 7)
    ov = ov if overlap == "exp_ran" else None
    whole = _seeded_gpu(dev, seed, C.STREAM, 0, ngpt, cf, ov)
    want = C.want_mask(seed, 0, ngpt, cf, ov)
    assert want[3:].any() and not want[cf > 0].all()
    np.testing.assert_array_equal(whole[0], want.astype(np.uint8))
    r = _randoms_gpu(dev, seed, C.STREAM, 0, ngpt, nlay, 7).cpu().numpy()
    for lo, hi in ((0, 3), (3, 7)):
        o = None if ov is None else ov[lo:hi]
        part = _seeded_gpu(dev, seed, C.STREAM, lo, ngpt, cf[lo:hi], o)
        np.testing.assert_array_equal(part[0], whole[0][lo:hi])
        np.testing.assert_array_equal(part[1], whole[1][lo:hi])
        rp = _randoms_gpu(dev, seed, C.STREAM, lo, ngpt, nlay, hi - lo).cpu().numpy()
        np.testing.assert_array_equal(rp.view(np.uint32), r[lo:hi].view(np.uint32))


def _last_error():
    from rrtmgpnn import _lib
    return _lib.lib().rrtmgpnn_last_error().decode()


def test_argument_errors(dev):
    from rrtmgpnn import _lib
    from rrtmgpnn.api import context
    L, ctx = _lib.lib(), context(0).h
    ngpt, nlay, ncol = 40, 5, 3
    rng = torch.zeros(4, dtype=torch.int32, device=dev)
    cf = T(np.full((ncol, nlay), 0.5), dev)
    ov = T(np.zeros((ncol, nlay - 1)), dev)
    mb = torch.zeros((ncol, nlay, ngpt), dtype=torch.uint8, device=dev)
    bits = torch.zeros((ncol, nlay, 2), dtype=torch.int32, device=dev)
    r = torch.zeros((ncol, nlay, ngpt), device=dev)
    p = lambda t: t.data_ptr()  # noqa: E731
    assert L.rrtmgpnn_mcica_rng_set(ctx, 1, 2, 3, p(rng)) == 0
    torch.cuda.synchronize()
    assert rng.cpu().numpy().view(np.uint32).tolist() == [1, 0, 2, 3]
    assert L.rrtmgpnn_mcica_rng_set(ctx, (5 << 32) | 6, 0xFFFFFFFF, 2 ** 32 - 2, p(rng)) == 0
    assert rng.cpu().numpy().view(np.uint32).tolist() == [6, 5, 0xFFFFFFFF, 2 ** 32 - 2]
    # NULL rng
    assert L.rrtmgpnn_mcica_rng_set(ctx, 1, 2, 3, None) == ERR_ARGUMENT and "rng is NULL" in _last_error()
    assert L.rrtmgpnn_mcica_randoms(ctx, ngpt, nlay, ncol, None, p(r)) == ERR_ARGUMENT and "rng is NULL" in _last_error()
    assert L.rrtmgpnn_sampled_mask_max_ran_seeded(ctx, ngpt, nlay, ncol, None, p(cf), p(mb), p(bits)) == ERR_ARGUMENT
    assert "sampled_mask_max_ran_seeded: rng is NULL" in _last_error()
    assert L.rrtmgpnn_sampled_mask_exp_ran_seeded(ctx, ngpt, nlay, ncol, None, p(cf), p(ov), p(mb), p(bits)) \
        == ERR_ARGUMENT
    assert "sampled_mask_exp_ran_seeded: rng is NULL" in _last_error()
    # both outputs NULL
    assert L.rrtmgpnn_sampled_mask_max_ran_seeded(ctx, ngpt, nlay, ncol, p(rng), p(cf), None, None) == ERR_ARGUMENT
    assert "neither cloud_mask nor mask_bits" in _last_error()
    assert L.rrtmgpnn_sampled_mask_exp_ran_seeded(ctx, ngpt, nlay, ncol, p(rng), p(cf), p(ov), None, None) \
        == ERR_ARGUMENT
    assert "neither cloud_mask nor mask_bits" in _last_error()
    # negative (and zero g-point / layer) extents; a missing overlap_param above one layer; NULL arrays
    for ext in ((-1, nlay, ncol), (ngpt, -1, ncol), (ngpt, nlay, -1), (0, nlay, ncol), (ngpt, 0, ncol)):
        assert L.rrtmgpnn_sampled_mask_max_ran_seeded(ctx, *ext, p(rng), p(cf), p(mb), p(bits)) == ERR_ARGUMENT, ext
        assert "bad argument" in _last_error()
        assert L.rrtmgpnn_sampled_mask_exp_ran_seeded(ctx, *ext, p(rng), p(cf), p(ov), p(mb), p(bits)) == ERR_ARGUMENT
        assert L.rrtmgpnn_mcica_randoms(ctx, *ext, p(rng), p(r)) == ERR_ARGUMENT, ext
    assert L.rrtmgpnn_sampled_mask_exp_ran_seeded(ctx, ngpt, nlay, ncol, p(rng), p(cf), None, p(mb), None) == ERR_ARGUMENT
    assert L.rrtmgpnn_sampled_mask_max_ran_seeded(ctx, ngpt, nlay, ncol, p(rng), None, p(mb), None) == ERR_ARGUMENT
    assert L.rrtmgpnn_mcica_randoms(ctx, ngpt, nlay, ncol, p(rng), None) == ERR_ARGUMENT
    # no columns: OK, nothing launched; one layer: overlap_param may be NULL
    assert L.rrtmgpnn_sampled_mask_max_ran_seeded(ctx, ngpt, nlay, 0, p(rng), p(cf), p(mb), p(bits)) == 0
    assert L.rrtmgpnn_mcica_randoms(ctx, ngpt, nlay, 0, p(rng), p(r)) == 0
    assert L.rrtmgpnn_sampled_mask_exp_ran_seeded(ctx, ngpt, 1, ncol, p(rng), p(cf), None, p(mb), p(bits)) == 0
    torch.cuda.synchronize()


def test_class_layer_messages(dev):
    """The checks and the reference's messages of the array functions, (seed, stream, col0) in place of randoms."""
    from rrtmgpnn import api, cloud_sampling as cs
    _, cf, ov = (T(a, dev) for a in M.build(40, 7, 3, 1))
    mb = torch.zeros((3, 7, 40), dtype=torch.uint8, device=dev)
    bits = torch.zeros((3, 7, 2), dtype=torch.int32, device=dev)
    pre = "sampled_mask_max_ran: "
    s = (11, 0, 0)
    assert cs.sampled_mask_max_ran_seeded(*s, cf, mb[:2]) == \
        pre + "sizes of randoms(ngpt,nlay,ncol) and cloud_mask(ncol,nlay,ngpt) are inconsistent"
    assert cs.sampled_mask_exp_ran_seeded(*s, cf, ov, mb[:, :6]) == \
        pre + "sizes of randoms(ngpt,nlay,ncol) and cloud_mask(ncol,nlay,ngpt) are inconsistent"
    assert cs.sampled_mask_exp_ran_seeded(*s, cf, ov[:, :4], mb) == \
        pre + "sizes of randoms(ngpt,nlay,ncol) and overlap_param(ncol,nlay-1) are inconsistent"
    assert cs.sampled_mask_max_ran_seeded(*s, cf) != ""           # no output at all
    assert cs.sampled_mask_max_ran_seeded(*s, cf, None, bits) != ""   # bits alone need ngpt
    assert cs.sampled_mask_max_ran_seeded(*s, cf, None, bits, ngpt=40) == ""
    assert cs.sampled_mask_max_ran_seeded(*s, cf, mb, bits[:, :, :1]) != ""
    assert cs.mcica_randoms(*s, torch.zeros((3, 7), device=dev)) != ""
    api.rte_config_checks(True)
    try:
        hi, lo = cf.clone(), cf.clone()
        hi[1, 2], lo[0, 0] = 1.5, -0.1
        for bad in (hi, lo):
            assert cs.sampled_mask_max_ran_seeded(*s, bad, mb) == pre + "cloud fraction values out of range [0,1]"
            assert cs.sampled_mask_exp_ran_seeded(*s, bad, ov, mb) == pre + "cloud fraction values out of range [0,1]"
        for v in (1.25, -1.25):
            bad = ov.clone()
            bad[2, 3] = v
            assert cs.sampled_mask_exp_ran_seeded(*s, cf, bad, mb) == pre + "overlap_param values out of range [-1,1]"
        assert cs.sampled_mask_exp_ran_seeded(*s, cf, ov, mb) == ""
    finally:
        api.rte_config_checks(False)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------
# ClearSkyStep(mcica={"seed": ...}): 36 RFMIP columns, the all-sky recipe's clouds with a cloud fraction per layer
SEED_A, SEED_B = 20261019, (3 << 32) | 77


def _fluxes(step):
    step.step()
    torch.cuda.synchronize()
    return step.fluxes()


def _same(got, want, use, what=""):
    np.testing.assert_array_equal(got["lw_up"], want["lw_up"], err_msg=what)
    np.testing.assert_array_equal(got["lw_dn"], want["lw_dn"], err_msg=what)
    for k in ("sw_up", "sw_dn", "sw_dir"):
        np.testing.assert_array_equal(got[k][use], want[k][use], err_msg=what + k)


@pytest.fixture(scope="module", params=["max_ran", "exp_ran"])
def step_case(request, dev, rfmip):
    """The problem, its clouds and the seeded fused step's fluxes for SEED_A and SEED_B (never modified)."""
    from conftest import subset
    from rrtmgpnn import data
    from rrtmgpnn.pipeline import ClearSkyStep
    prob = subset(rfmip, np.arange(0, 1800, 50))
    ncol, nlay = prob["ncol"], prob["nlay"]
    assert ncol == 36
    clouds = data.allsky_clouds(prob, data.load_cloud_optics("lw"))
    cloudy = (clouds[0] > 0) | (clouds[1] > 0)
    assert cloudy.any()
    rng = np.random.default_rng(51)
    cf = np.where(cloudy, rng.uniform(0.2, 0.9, cloudy.shape), 0).astype(np.float32)
    ov = rng.uniform(-1, 1, (ncol, nlay - 1)).astype(np.float32) if request.param == "exp_ran" else None
    c = {"prob": prob, "clouds": clouds, "cf": cf, "ov": ov, "use": prob["usecol"], "ncol": ncol, "nlay": nlay,
         "ng_lw": data.load_kdist("lw")["ngpt"], "ng_sw": data.load_kdist("sw")["ngpt"]}
    for name, seed in (("a", SEED_A), ("b", SEED_B)):
        s = ClearSkyStep(prob, device=0, clouds=clouds, mcica={"cloud_frac": cf, "overlap_param": ov, "seed": seed})
        c[name] = _fluxes(s)
        if name == "a":
            c["names"] = [n for n, _, _ in s.calls]
            assert not hasattr(s, "randoms_lw") or s.randoms_lw is None  # no randoms buffers
        s.close()
    return c


def test_step_seeded_equals_array_route_and_oracle(step_case, orc):
    from rrtmgpnn.pipeline import ClearSkyStep
    c = step_case
    r_lw = P.randoms(SEED_A, 0, 0, c["ng_lw"], c["nlay"], c["ncol"])  # stream_lw 0, stream_sw 1, col0 0: the defaults
    r_sw = P.randoms(SEED_A, 1, 0, c["ng_sw"], c["nlay"], c["ncol"])
    arr = ClearSkyStep(c["prob"], device=0, clouds=c["clouds"],
                       mcica={"cloud_frac": c["cf"], "overlap_param": c["ov"], "randoms_lw": r_lw, "randoms_sw": r_sw})
    _same(c["a"], _fluxes(arr), c["use"], "array route ")
    arr.close()
    _same(c["a"], M.step_oracle(orc, c["prob"], c["clouds"], c["cf"], c["ov"], r_lw, r_sw), c["use"], "oracle ")
    assert (c["a"]["lw_dn"] != c["b"]["lw_dn"]).any() and (c["a"]["sw_dn"] != c["b"]["sw_dn"]).any()


def test_step_replay_reads_the_device_words(step_case):
    """A captured step replayed after set_mcica_seed gives the fluxes of a fresh step built with that seed."""
    from rrtmgpnn.pipeline import ClearSkyStep
    c = step_case
    s = ClearSkyStep(c["prob"], device=0, clouds=c["clouds"],
                     mcica={"cloud_frac": c["cf"], "overlap_param": c["ov"], "seed": SEED_A})
    s.step()
    torch.cuda.synchronize()
    s.capture()
    for t in (s.lw_up, s.lw_dn, s.sw_up, s.sw_dn, s.sw_dir):
        t.fill_(float("nan"))
    s.replay()
    torch.cuda.synchronize()
    _same(s.fluxes(), c["a"], c["use"], "replay ")
    s.set_mcica_seed(seed=SEED_B)
    s.replay()
    torch.cuda.synchronize()
    _same(s.fluxes(), c["b"], c["use"], "replay after set_mcica_seed ")
    s.close()


def test_step_halves_reproduce_the_whole(step_case):
    from conftest import subset
    from rrtmgpnn.pipeline import ClearSkyStep
    c = step_case
    for lo, hi in ((0, 18), (18, 36)):
        idx = np.arange(lo, hi)
        prob = subset(c["prob"], idx)
        clouds = tuple(a[idx] for a in c["clouds"])
        mc = {"cloud_frac": c["cf"][idx], "overlap_param": None if c["ov"] is None else c["ov"][idx], "seed": SEED_A,
              "col0": lo}
        s = ClearSkyStep(prob, device=0, clouds=clouds, mcica=mc)
        got = _fluxes(s)
        s.close()
        _same(got, {k: v[idx] for k, v in c["a"].items()}, prob["usecol"], "columns %d..%d " % (lo, hi))


def test_step_unfused_equals_fused(step_case):
    from rrtmgpnn.pipeline import ClearSkyStep
    c = step_case
    s = ClearSkyStep(c["prob"], device=0, clouds=c["clouds"], fused=False,
                     mcica={"cloud_frac": c["cf"], "overlap_param": c["ov"], "seed": SEED_A})
    names = [n for n, _, _ in s.calls]
    assert names.index("mcica_randoms_lw") == names.index("mcica_mask_lw") - 1
    assert names.index("mcica_randoms_sw") == names.index("mcica_mask_sw") - 1
    _same(_fluxes(s), c["a"], c["use"], "unfused ")
    s.close()


FUSED_ARRAY = ["cloud_optics_sw", "delta_scale_sw", "mcica_mask_sw", "predict_nn_sw", "cloud_optics_lw", "mcica_mask_lw",
               "predict_nn_lw", "lw_mask", "lw_solver", "sw_mask", "sw_solver"]
UNFUSED_ARRAY = ["get_col_dry", "sw_boundary", "nn_inputs_lw", "predict_nn_lw", "cloud_optics_lw", "mcica_mask_lw",
                 "draw_samples_lw", "increment_lw", "planck_source", "expand_emis", "lw_solver", "nn_inputs_sw",
                 "predict_nn_sw", "cloud_optics_sw", "delta_scale_sw", "mcica_mask_sw", "draw_samples_sw",
                 "increment_sw", "sw_solver"]
FUSED_OVERCAST = ["cloud_optics_sw", "delta_scale_sw", "predict_nn_sw", "cloud_optics_lw", "predict_nn_lw", "lw_solver",
                  "sw_solver"]


def test_step_refusals_and_unchanged_call_lists(step_case):
    from conftest import subset
    from rrtmgpnn import _lib
    from rrtmgpnn.pipeline import ClearSkyStep
    c = step_case
    idx = np.arange(4)
    prob = subset(c["prob"], idx)
    clouds = tuple(a[idx] for a in c["clouds"])
    nlay = c["nlay"]
    base = {"cloud_frac": c["cf"][idx], "overlap_param": None if c["ov"] is None else c["ov"][idx]}
    r_lw, r_sw = np.zeros((4, nlay, c["ng_lw"]), np.float32), np.zeros((4, nlay, c["ng_sw"]), np.float32)
    for extra in ({"randoms_lw": r_lw}, {"randoms_sw": r_sw}, {"randoms_lw": r_lw, "randoms_sw": r_sw}):
        with pytest.raises(ValueError, match="seed"):
            ClearSkyStep(prob, device=0, clouds=clouds, mcica=dict(base, seed=1, **extra))
    s = ClearSkyStep(prob, device=0, clouds=clouds, mcica=dict(base, seed=1))
    with pytest.raises(ValueError, match="seeded"):
        s.mcica_randoms()
    # the seeded fused list is the array route's, name for name, on the _seeded entries
    assert [n for n, _, _ in s.calls] == FUSED_ARRAY == c["names"]
    L = _lib.lib()
    seeded = (L.rrtmgpnn_sampled_mask_max_ran_seeded, L.rrtmgpnn_sampled_mask_exp_ran_seeded)
    assert all(f in seeded for n, f, _ in s.calls if n.startswith("mcica_mask_"))
    s.close()
    # without a seed: the parent's lists, and the array entries
    arr = dict(base, randoms_lw=r_lw, randoms_sw=r_sw)
    for fused, want in ((True, FUSED_ARRAY), (False, UNFUSED_ARRAY)):
        s = ClearSkyStep(prob, device=0, clouds=clouds, mcica=arr, fused=fused)
        assert [n for n, _, _ in s.calls] == want
        assert not any(f in seeded for _, f, _ in s.calls)
        with pytest.raises(ValueError, match="seed"):
            s.set_mcica_seed(seed=2)
        s.close()
    s = ClearSkyStep(prob, device=0, clouds=clouds)
    assert [n for n, _, _ in s.calls] == FUSED_OVERCAST
    with pytest.raises(ValueError):
        s.set_mcica_seed(seed=2)
    s.close()
