"""bench.py's plain run (the headline alone) and its --dump-outputs files.  Everything else the benchmark measures runs only
with --full (tests/test_gpu_round2.py, tests/test_gpu_round3.py, tests/test_gpu_parity.py cover that line)."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
FULL_ONLY = ("other_precision", "extra_Mpx_s", "host_pipeline", "host_us_per_apply", "cpu_baseline", "strong")


def test_plain_run_leaves_every_other_measurement_to_full():
    import bench
    a = bench.parse_args(["--steps", "7"])
    assert a.steps == 7 and not a.full
    assert a.no_cpu_baseline and a.no_extra and a.no_strong and a.no_host_cost and a.no_stats and a.no_other
    assert a.pipeline == "hbm"
    f = bench.parse_args(["--full"])
    assert not (f.no_cpu_baseline or f.no_extra or f.no_strong or f.no_host_cost or f.no_stats or f.no_other)
    assert f.pipeline == "auto"


def test_dump_sample_is_fixed_and_bounded():
    import bench
    assert bench.dump_index((1, 1080, 1920), 1) is None
    a, b = bench.dump_index((256, 2160, 3840), 0), bench.dump_index((256, 2160, 3840), 0)
    assert np.array_equal(a, b) and len(a) == bench.DUMP_VALUES and np.all(np.diff(a) >= 0) and a[-1] < 256 * 2160 * 3840
    assert 3 * bench.DUMP_VALUES * 4 <= 64 << 20


@pytest.mark.gpu
def test_plain_line_and_dumped_outputs_match_the_oracle(orc, tmp_path):
    """One UHD yuv420p10le frame: the luma plane is above the dump limit (seeded sample), the chroma planes are written
    whole; every dumped code equals the oracle's on the same seeded input."""
    import bench
    from lut_renderer_amd import cube, frames
    res = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--steps", "3", "--warmup", "1", "--frames", "1",
                          "--dump-outputs", str(tmp_path / "out")], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    d = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][0])
    for key in ("metric", "value", "unit", "steps", "warmup", "ms_per_step", "higher_is_better", "dtype", "config", "roofline"):
        assert key in d, key
    assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["value"] > 0 and d["dtype"] == "f32"
    assert not any(k in d for k in FULL_ONLY) and d["config"]["lds_window"] is None

    lut = cube.read_cube(cube.write_cube(tmp_path / "log709_33.cube", cube.log709_lattice(33), title="log709 33"))
    src = frames.make_yuv("natural", 3840, 2160, 10, 1, 1, k=0)
    k = orc.yuv_constants("bt709", "tv", "bt709", "tv", 10, 10, 10, 4)
    want = orc.apply_yuv(lut.table, lut.scale, "tetrahedral", k, 10, 10, 10, 1, 1, src, nthreads=16)
    for i, name in enumerate(("y", "cb", "cr")):
        got = np.load(tmp_path / "out" / f"{name}.npy")
        assert got.dtype == np.float32
        w = want[i][None].astype(np.float32)
        idx = bench.dump_index(w.shape, i)
        assert np.array_equal(got, w if idx is None else w.reshape(-1)[idx]), name
