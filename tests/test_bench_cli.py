"""bench.py's command line: a plain run measures the headline and nothing else, --full adds the other legs to the same line."""
import json

import pytest

import bench

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus")
# what only a --full run carries at N = 1 (the last three need minutes: the GPU test below takes them out with the --skip-* options)
FULL_CHEAP = ("timed_region_repeats", "roofline", "roofline_operator", "kernels_us", "op_algorithmic_GBps")
FULL_LONG = ("roofline_large", "cpu_baseline", "cpu_baseline_all_cores", "extra")
# every function of bench.py that a leg outside the headline goes through
LEGS = ("spread", "kernel_profile", "event_overhead_us", "stream_probe", "dense_legs", "large_frame_leg", "cpu_baseline_voxel",
        "cpu_allcore_voxel", "extras", "iou_leg", "nms_leg", "iou3d_leg")


def test_full_is_an_option_and_off_by_default():
    ap = bench.build_parser()
    assert ap.parse_args(["--gpus", "1", "--steps", "3", "--warmup", "1"]).full is False
    assert ap.parse_args(["--gpus", "1", "--steps", "3", "--warmup", "1", "--full"]).full is True
    for name in LEGS:
        assert callable(getattr(bench, name)), name


def _line(capsys, argv):
    bench.main(argv)
    lines = [x for x in capsys.readouterr().out.splitlines() if x.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone(capsys, monkeypatch, tmp_path):
    def forbidden(name):
        def f(*a, **k):
            raise AssertionError("a plain run went into bench.%s" % name)
        return f
    for name in LEGS:
        monkeypatch.setattr(bench, name, forbidden(name))
    line = _line(capsys, ["--gpus", "1", "--steps", "3", "--warmup", "1", "--points", "50000", "--dump-outputs", str(tmp_path)])
    for k in HEADLINE:
        assert k in line, k
    for k in FULL_CHEAP + FULL_LONG:
        assert k not in line, k
    assert line["metric"] == "voxelize_mpoints_per_s" and line["unit"] == "Mpoints/s" and line["dtype"] == "f32"
    assert line["higher_is_better"] is True and (line["steps"], line["warmup"], line["n_gpus"]) == (3, 1, 1)
    assert line["value"] > 0 and line["ms_per_step"] > 0
    # value and ms_per_step are the same region: 50000 points per step
    assert line["value"] == pytest.approx(50000 / (line["ms_per_step"] * 1e-3) / 1e6, rel=1e-2)
    import numpy as np
    assert np.load(tmp_path / "coords.npy").shape[0] == line["voxels"]
    assert np.load(tmp_path / "voxels.npy").shape[:2] == (line["voxels"], 32)


@pytest.mark.gpu
def test_full_run_adds_the_legs_to_the_same_line(capsys):
    line = _line(capsys, ["--gpus", "1", "--steps", "3", "--warmup", "1", "--points", "100000", "--full",
                          "--skip-large", "--skip-cpu", "--skip-extra"])
    for k in HEADLINE + FULL_CHEAP:
        assert k in line, k
    for k in FULL_LONG:
        assert k not in line, k
    assert line["timed_region_repeats"]["reps"] == 5
    assert line["roofline"]["kernel"] in line["kernels_us"]
    assert line["roofline"]["event_overhead_us"] > 0
