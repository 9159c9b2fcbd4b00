"""GPU: bench.py's split between a plain run and --full, through the command line.  A plain run prints the headline
keys alone (bench.PLAIN_KEYS: none of the --full blocks ran, since each block's result is a key of the line); --full
prints those and every block (bench.FULL_KEYS), with the blocks it was not told to skip filled in.  --steps and
--warmup are the line's, and --dump-outputs writes the same fluxes, bit for bit, in both modes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _bench(tmp_path, name, *extra):
    d = str(tmp_path / name)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--settle-s", "0.05", "--dump-outputs", d, *extra], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout  # ONE JSON line
    return json.loads(lines[0]), {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return _bench(tmp_path_factory.mktemp("bench"), "plain")


def test_plain_run_prints_the_headline_keys_alone(plain):
    import bench
    line, _ = plain
    assert set(line) == set(bench.PLAIN_KEYS)
    assert not set(line) & set(bench.FULL_KEYS)
    assert line["full"] is False and line["steps"] == 3 and line["warmup"] == 1
    assert line["unit"] == "columns/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["ms_per_step"] > 0
    # value is the columns of the timed steps over their time: 1800 columns per ms_per_step (both rounded in the line)
    assert line["value"] == pytest.approx(1800 / (line["ms_per_step"] * 1e-3), rel=1e-3)


def test_full_run_adds_every_block_and_dumps_the_same_fluxes(plain, tmp_path):
    import bench
    # the two long blocks (1e6-column c5_global, the CPU baseline) are switched off by their own options: their keys stay
    line, dump = _bench(tmp_path, "full", "--full", "--c5-steps", "0", "--no-cpu-baseline")
    assert set(line) == set(bench.PLAIN_KEYS) | set(bench.FULL_KEYS)
    assert line["full"] is True and line["steps"] == 3
    for k in ("ms_per_step_unsettled", "value_unsettled", "roofline", "stages_ms", "stages_overlapped_ms",
              "stage_roofline", "host_resident", "block_stream"):
        assert line[k], k  # measured at N = 1
    assert line["c5_global"] is None and line["cpu_baseline"] is None  # switched off above
    assert line["gather_ms"] is None and line["gather_check"] is None and line["end_to_end"] is None  # N > 1 only
    assert set(line["stages_ms"]) == {"predict_nn_lw", "predict_nn_sw", "lw_solver", "sw_solver"}
    pline, pdump = plain
    assert pline["dump_outputs"]["arrays"] == list(bench.FLUX_NAMES) == line["dump_outputs"]["arrays"]
    assert sorted(dump) == sorted(pdump) == sorted(bench.FLUX_NAMES)
    for k in bench.FLUX_NAMES:
        assert pdump[k].dtype == np.float32 and pdump[k].shape == (1800, 61)
        np.testing.assert_array_equal(pdump[k].view(np.uint32), dump[k].view(np.uint32), err_msg=k)
