"""CPU: the step-level GPU tests compare the SW fluxes of night columns (usecol false, solved with mu0 = 1) with the
oracle's raw rte_sw output (zero_unused=False).  That comparison is vacuous on a problem without night columns: every
problem and column sample those tests use must contain some, and day columns too.  Also: zero_unused=True is
zero_unused=False with the night columns' up and down fluxes set to zero, nothing else."""
import numpy as np

from conftest import subset


def _has_both(usecol, what):
    usecol = np.asarray(usecol)
    assert (~usecol).any(), what + ": no night column"
    assert usecol.any(), what + ": no day column"


def test_step_test_problems_contain_night_columns(rfmip):
    from rrtmgpnn import data, shard
    import test_gpu_fullsize as FS
    _has_both(rfmip["usecol"], "RFMIP (C3)")
    # C4 and C5 as tests/test_gpu_fullsize.py samples them; usecol does not depend on the layer count (a column's RFMIP
    # site is drawn first from its block's random stream), so two layers suffice here
    c4 = data.synthetic_problem(10000, 2, seed=20251015)
    _has_both(c4["usecol"][FS._sample(10000, 400)], "C4 sample")
    c5 = data.synthetic_problem(125000, 2, seed=20251015)
    np.testing.assert_array_equal(c5["usecol"][:10000], c4["usecol"])
    _has_both(c5["usecol"][FS._sample(125000, 500)], "C5 sample")
    lo, hi = shard.column_range(1000000, 1, 3)
    g = data.synthetic_problem(hi - lo, 2, seed=20251015, col0=lo)
    _has_both(g["usecol"][FS._sample(hi - lo, 300)], "C5 global rank sample")
    # the pipeline-shape problems of tests/test_gpu_parity.py with more than a handful of columns
    _has_both(data.synthetic_problem(50, 137, seed=137)["usecol"], "synthetic 50 x 137")


def test_zero_unused_only_zeroes_night_up_and_down(orc, rfmip):
    from rrtmgpnn import data
    prob = subset(rfmip, np.arange(3, 1800, 45))
    _has_both(prob["usecol"], "subset")
    models = [data.load_model("sw_abs"), data.load_model("sw_ray")]
    kd = data.load_kdist("sw")
    up, dn, dr, _ = orc.clear_sky_sw(prob, models, kd)
    ru, rd, rr, _ = orc.clear_sky_sw(prob, models, kd, zero_unused=False)
    night = ~prob["usecol"]
    assert (ru[night] != 0).any() and (rd[night] != 0).any()  # the raw output of a night column is a solved column
    assert not up[night].any() and not dn[night].any()
    np.testing.assert_array_equal(up[~night], ru[~night])
    np.testing.assert_array_equal(dn[~night], rd[~night])
    np.testing.assert_array_equal(dr, rr)
    co = data.load_cloud_optics("sw")
    clouds = data.allsky_clouds(prob, data.load_cloud_optics("lw"))
    up, dn, dr, _ = orc.all_sky_sw(prob, models, kd, co, clouds)
    ru, rd, rr, _ = orc.all_sky_sw(prob, models, kd, co, clouds, zero_unused=False)
    assert (ru[night] != 0).any() and not up[night].any() and not dn[night].any()
    np.testing.assert_array_equal(up[~night], ru[~night])
    np.testing.assert_array_equal(dn[~night], rd[~night])
    np.testing.assert_array_equal(dr, rr)
