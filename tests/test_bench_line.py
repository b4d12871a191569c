"""The ONE line bench.py prints for the driver: short enough to be parsed (round 5's 22 KB line was not), valid JSON, carrying the
contract's keys, `roofline` and `cpu_baseline`.  Fed with the full record of a real run (profiles/r05, 22 KB) and with a record whose
free-text fields have grown out of hand.  The timing contract it mirrors: one number per run,
[REF roman/align/submap_align.py:155-157]."""
import json
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, ROOT)

FULL = os.path.join(ROOT, "profiles", "r05", "bench_line_driver_flags_20steps.json")
CONTRACT = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "config", "roofline", "cpu_baseline", "timed_region_s", "p50_latency_ms")


def _full():
    with open(FULL) as fh:
        return json.load(fh)


def test_headline_of_a_real_record_is_short_valid_and_complete():
    import bench
    full = _full()
    assert len(json.dumps(full)) > 20000                              # the record that the driver could not parse
    text = bench.headline(full)
    assert len(text) < bench.HEADLINE_MAX_BYTES == 4096 and "\n" not in text
    line = json.loads(text)
    for k in CONTRACT:
        assert k in line, k
    assert line["value"] == pytest.approx(full["value"], rel=1e-5) and line["ms_per_step"] == pytest.approx(full["ms_per_step"], rel=1e-5)
    assert line["config"]["workload"].startswith("config 3") and "model" not in line["config"]
    r = line["roofline"]
    for k in ("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] == "hbm" and r["frac"] == pytest.approx(r["achieved"] / r["peak"], rel=1e-4)
    assert {"k_count", "k_cos"} <= set(r["kernels"]) and "frac" in r["step"] and "frac" in r["isolated"]
    c = line["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample", "identical_to_gpu"):
        assert k in c, k
    assert c["kind"] == "port" and line["vs_baseline"] is None and line["higher_is_better"] is True


def test_headline_stays_short_whatever_the_notes_grow_to():
    import bench
    full = _full()
    full["config"]["workload"] = "w" * 3000
    full["cpu_baseline"]["sample"] = "s" * 3000
    full["p50_note"] = "n" * 5000
    full["side_legs_error"] = "e" * 9000
    full["ranks"] = {"ms_per_step_by_rank": [1.234567] * 64}
    text = bench.headline(full)
    assert len(text) < bench.HEADLINE_MAX_BYTES
    line = json.loads(text)
    assert line["value"] == pytest.approx(full["value"], rel=1e-5) and "roofline" in line and "cpu_baseline" in line


def test_emit_prints_the_headline_last_and_alone(tmp_path, capsys, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    bench.emit(_full())
    out = capsys.readouterr().out
    lines = [l for l in out.splitlines() if l.strip()]
    assert len(lines) == 1 and len(lines[0]) < 4096                   # stdout: the one line; everything else went to the side file / stderr
    line = json.loads(lines[0])
    extras = json.load(open(tmp_path / "bench_extras.json"))
    assert line["extras"] == "bench_extras.json" and "caller" in extras and "decision_sensitivity" in extras


def test_live_traffic_reports_why_when_there_is_no_profiler(monkeypatch):
    """roofline.traffic is measured by re-running the main measurement under rocprofv3 --pmc (bench.live_traffic); without the tool the
    bench says so and quotes the committed pass instead — it never loses the line over it."""
    import shutil
    import bench
    monkeypatch.setattr(shutil, "which", lambda name: None)
    tb, why = bench.live_traffic()
    assert tb is None and "rocprofv3" in why


def _fake_measure(tmp_steps=7):
    """A measure() record over CPU output sets: 3 sets, a step of two calls (4 + 3 problems), `tmp_steps` steps timed — the
    last step's calls are numbers 12 and 13, i.e. output sets 0 and 1; set 2 holds the step before."""
    import types
    import numpy as np
    import torch
    from roman_amd.align.pipeline import OutputSet
    sets = [OutputSet(4, 5, "cpu") for _ in range(3)]
    for k, s in enumerate(sets):
        s.n[:] = torch.tensor([1, 2, 3, 0]) + k
        s.assoc[:] = 10 * k + 1
        s.T[:] = float(k)
        s.status[:] = k
    S = types.SimpleNamespace(sets=sets, nset=3, loop=types.SimpleNamespace(call_no=2 * tmp_steps))
    return types.SimpleNamespace(stream_=S, calls=[np.arange(4), np.arange(4, 7)], total_per_step=7, steps=tmp_steps, warmup=1, dt=0.5,
                                 scaling="weak", wl_text="config 3: test", CB=4, skipped=0, rank_ms=[1.0])


def test_dump_outputs_writes_the_last_steps_results(tmp_path):
    import numpy as np
    import bench
    bench.dump_outputs(str(tmp_path), _fake_measure())
    got = {p.stem: np.load(p) for p in tmp_path.glob("*.npy")}
    assert {"problem", "assoc", "n_assoc", "T", "status", "stats_score", "stats_n_pass"} <= set(got)
    assert all(v.dtype == np.float64 for v in got.values())
    assert got["problem"].tolist() == list(range(7))
    assert got["status"].tolist() == [0.0] * 4 + [1.0] * 3                       # call 12 -> set 0, call 13 -> set 1
    assert got["n_assoc"].tolist() == [1, 2, 3, 0, 2, 3, 4]
    a = got["assoc"]
    assert a.shape == (7, 5, 2) and np.all(got["T"][4:] == 1.0) and got["T"].shape == (7, 16)
    for r in range(7):                                                            # rows past the count are -1, the others the set's
        k = int(got["n_assoc"][r])
        assert np.all(a[r, :k] == (1.0 if r < 4 else 11.0)) and np.all(a[r, k:] == -1.0)


def test_plain_line_carries_the_headline_keys():
    import types
    import bench
    M = _fake_measure(tmp_steps=8)
    args = types.SimpleNamespace(n=200, m=200, d=512, method="semanticgrav", pipeline=3)
    text = bench.plain_line(args, M, 1)
    line = json.loads(text)
    assert "\n" not in text and len(text) < bench.HEADLINE_MAX_BYTES
    assert line["metric"] == bench.METRIC and line["dtype"] == bench.DTYPE and line["unit"] == "alignments/s"
    assert line["higher_is_better"] is True and line["steps"] == 8
    assert line["ms_per_step"] == pytest.approx(0.5 / 8 * 1e3, rel=1e-5) and line["value"] == pytest.approx(7 * 8 / 0.5, rel=1e-5)


def test_full_is_off_by_default(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 3
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "x"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "x"


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_what_they_computed(tmp_path, orc):
    """`bench.py --gpus 1 --steps 3 --warmup 1 --dump-outputs DIR` in a fresh process: one line, the steps asked for, and the
    last step's associations are the oracle's for the first problems of config 3."""
    import subprocess
    import numpy as np
    from roman_amd import synth
    from roman_amd.align import SubmapAlignParams
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                          "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0 and line["skipped_in_timed_steps"] == 0
    assert "roofline" not in line and "cpu_baseline" not in line
    got = {p.stem: np.load(p) for p in tmp_path.glob("*.npy")}
    assert got["problem"].tolist() == list(range(256)) and np.all(got["status"] == 0)
    reg = SubmapAlignParams(method="semanticgrav", semantics_dim=512).get_object_registration()
    for b in range(2):
        pr = synth.make_pair(200, 200, 512, 3000 + b)
        ref = orc.register(reg._abi_params(), reg.pack(pr.map1), reg.pack(pr.map2))
        k = int(got["n_assoc"][b])
        assert np.array_equal(got["assoc"][b, :k].astype(np.int64), ref["assoc"].astype(np.int64)), b
