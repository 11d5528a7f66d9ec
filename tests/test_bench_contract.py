"""The bench.py output contract, checked on the lines committed under profiles/ (produced by bench.py, today `--full`, on an
MI355X; no GPU needed here): every key the driver and the judge read is present and well-formed."""
import json
import os

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", ["r01_final_bench_default.json", "r01_int8_bench.json", "r02_bench_default.json",
                                  "r02_bench_cpu_full_protocol.json", "r03_bench_default.json"])
def test_committed_bench_lines_follow_the_contract(name):
    d = json.loads(open(os.path.join(REPO, "profiles", name)).read().strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["unit"] == "frames/s" and d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None
    assert d["n_gpus"] == 1 and d["value"] > 0 and abs(d["value"] * d["ms_per_step"] / 1e3 - 1.0) < 0.02
    assert "workload" in d["config"] and "model" not in d["config"] and d["data"].startswith("synthetic")
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel"):
        assert k in r, k
    assert r["bound"] in ("hbm", "mfma") and r["unit"] == ("GB/s" if r["bound"] == "hbm" else "TFLOP/s")
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3 and 0 < r["frac"] < 1
    assert r["traffic"] is None or r["traffic"] >= 0.9 * r["algorithmic_bytes_per_launch"]
    c = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c, k
    assert c["kind"] in ("port", "reference") and c["cores"] >= 1 and 0 < c["value"] < d["value"]
    if name.startswith("r03"):          # round 3: traffic measured for the new dominant kernel, the in-product dispatcher beside the headline,
        # the bounded CPU protocol ending in one unscaled frame at the workload size
        assert d["roofline"]["kernel"].startswith("conv_prw") and d["roofline"]["traffic"] > d["roofline"]["algorithmic_bytes_per_launch"]
        disp = d["dispatcher_host_fed"]
        assert disp["worker_exit_codes"] == [0] and abs(disp["value"] / d["value_pcie_inclusive"] - 1.0) <= 0.03
        assert [(r["size"], r["warmup"], r["timed_frames"]) for r in c["runs"]] == [("960x540", 5, 20), ("1920x1080", 1, 5), ("3840x2160", 0, 1)]
        assert "scaled" not in c["sample"] and d["p99_ms"] >= d["p50_ms"]
    if name.startswith("r02") or name.startswith("r03"):          # round-2 protocol: ring-inclusive value, 1 % low, eager-CPU baseline per stage
        assert d["one_percent_low_fps"] <= 1000.0 / d["p50_ms"] * 1.001 and d["value_device_only"] > 0 and "pinned host" in d["metric"]
        assert c["cores"] <= c["physical_cores_available"] and c["cpu_model"] and c["backend"].startswith("PyTorch CPU eager")
        for r in c["runs"]:
            assert {"size", "warmup", "timed_frames", "pre_ms", "run_ms", "post_ms", "frames_per_s"} <= set(r)
        if c["protocol"] == "full":
            assert [(r["size"], r["warmup"], r["timed_frames"]) for r in c["runs"]] == [("960x540", 5, 20), ("1920x1080", 5, 20), ("3840x2160", 0, 2)]
        assert d["roofline"]["traffic_source"].startswith("profiles/pmc_traffic")


def test_bench_defaults_are_the_headline_configuration():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench", os.path.join(REPO, "bench.py"))
    src = open(os.path.join(REPO, "bench.py")).read()
    assert spec is not None
    for needle in ('"--gpus", type=int, default=1', '"--height", type=int, default=2160', '"--width", type=int, default=3840'):
        assert needle in src, needle


def test_bench_leaves_every_other_leg_to_full():
    """A plain `bench.py --gpus 1 --steps K --warmup W` runs only what `value` needs; `--full` (off by default) adds the other
    legs, and `--layers`, which prints the roofline leg's profile, asks for it."""
    import bench
    assert bench.parse(["--gpus", "1", "--steps", "3", "--warmup", "1"]).full is False
    assert bench.parse(["--full", "--layers"]).full is True
    with pytest.raises(SystemExit):
        bench.parse(["--layers"])


def test_bench_self_launches_its_ranks(tmp_path):
    """`python bench.py --gpus 2` with no WORLD_SIZE in the environment starts two ranks itself (torch.distributed.run in a
    child process) and relays rank 0's line with n_gpus = 2.  HDRTV_BENCH_RANK_STUB=1 replaces the GPU work of a rank by the
    rendezvous / barrier / max-over-ranks skeleton (gloo), so this runs without a GPU."""
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env["HDRTV_BENCH_RANK_STUB"] = "1"
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["max_over_ranks"] == 2.0
    assert "torch.distributed.run" in r.stderr and "--nproc-per-node=2" in r.stderr


def test_committed_counter_figures_are_reported_only_for_the_code_they_were_measured_on():
    """bench.py's `roofline.traffic` comes from a committed rocprofv3 --pmc file: it must carry the library's build stamp, and a
    figure is printed only when the stamp matches the loaded library or the kernel's own source (and the shared headers) hash as
    they did at measurement time; otherwise `traffic` is null and `traffic_note` says why."""
    import bench
    doc = {"build_id": "aaaaaaaaaaaa", "sources": {"conv3x3_prw.hip": "111", "common.h": "222", "launchers.h": "333", "le_rows.hip": "444"}}
    same = {"conv3x3_prw.hip": "111", "common.h": "222", "launchers.h": "333", "le_rows.hip": "changed"}
    t, why = bench.traffic_for("conv_prw<pool>", 123, doc, "profiles/x.json", build_id=lambda: "aaaaaaaaaaaa", source_hash=same.__getitem__)
    assert (t, why) == (123, None)
    t, why = bench.traffic_for("conv_prw<pool>", 123, doc, "profiles/x.json", build_id=lambda: "bbbbbbbbbbbb", source_hash=same.__getitem__)
    assert t == 123 and "unchanged" in why
    t, why = bench.traffic_for("le_tail_rows", 123, doc, "profiles/x.json", build_id=lambda: "bbbbbbbbbbbb", source_hash=same.__getitem__)
    assert t is None and "le_rows.hip differs" in why
    t, why = bench.traffic_for("conv_prw<pool>", 123, {"kernels": {}}, "profiles/x.json", build_id=lambda: "bbbbbbbbbbbb", source_hash=same.__getitem__)
    assert t is None and "no build stamp" in why
    assert bench.traffic_for("conv_prw8_i8<ps>", 1, doc, "p", build_id=lambda: "b", source_hash=lambda f: "zzz")[0] is None


def test_library_version_carries_a_build_stamp():
    from hdrtv_mi355x import lib
    bid = lib.build_id()
    assert len(bid) == 12 and all(c in "0123456789abcdef" for c in bid), bid
    assert lib.source_hash("common.h") and len(lib.source_hash("common.h")) == 12
