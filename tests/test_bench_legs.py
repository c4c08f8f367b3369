"""bench.py's --full on the CPU: a plain run measures the headline alone; --full adds the secondary measurements, each still
subject to its --no-* switch and to the configuration it applies to."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ALL = ["roofline", "with_backbone", "exact_f32_error", "criterion", "cpu_baseline"]


def test_plain_run_has_no_secondary_legs():
    import bench
    for argv in ([], ["--gpus", "1", "--steps", "20", "--warmup", "5"], ["--config", "c4"], ["--loss", "criterion"],
                 ["--dump-outputs", "out"], ["--quick-cpu-baseline"]):
        a = bench.parse_args(argv)
        assert not a.full
        for world, dtype in ((1, "f32"), (1, "bf16"), (2, "f32")):
            assert bench.secondary_legs(a, world, dtype) == [], (argv, world, dtype)


def test_full_runs_every_leg_in_order():
    import bench
    assert bench.secondary_legs(bench.parse_args(["--full"]), 1, "f32") == ALL
    assert bench.secondary_legs(bench.parse_args(["--full", "--steps", "20", "--warmup", "5"]), 1, "f32") == ALL


def test_full_keeps_the_switches_and_the_configurations():
    import bench
    legs = lambda argv, world=1, dtype="f32": bench.secondary_legs(bench.parse_args(["--full"] + argv), world, dtype)  # noqa: E731
    for flag, name in (("--no-roofline", "roofline"), ("--no-backbone-leg", "with_backbone"), ("--no-exact-leg", "exact_f32_error"),
                       ("--no-criterion-leg", "criterion"), ("--no-cpu-baseline", "cpu_baseline")):
        assert legs([flag]) == [x for x in ALL if x != name], flag
    assert legs(["--no-cpu-baseline", "--no-criterion-leg", "--no-exact-leg", "--no-backbone-leg", "--no-roofline"]) == []
    assert legs(["--config", "c4"], dtype="bf16") == ["roofline", "criterion", "cpu_baseline"]   # backbone: C2 only; exact: f32 only
    assert legs(["--config", "c5"]) == ["roofline", "exact_f32_error", "criterion", "cpu_baseline"]
    assert legs(["--loss", "criterion"]) == ["roofline", "with_backbone", "cpu_baseline"]       # the step IS the criterion step
    assert legs([], world=2) == ["roofline"]                                                     # several ranks: rank 0's micro-benchmark


def test_help_names_full():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--full" in r.stdout
