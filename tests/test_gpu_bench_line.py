"""-m gpu: the bench.py --full line (N = 1) — ONE compact JSON line (< 6 KB, the LAST line of stdout, so
that the driver's parser keeps it whole: round 4's 21 KB line came back `parsed: null`) whose `roofline` carries every BASELINE GPU
config as flat scalars (`frac_c3` ...) and in `per_config` (+ the README scene, the scope `draw`, the non-integer-exponent
variant, the tolerance-mode rows and the reference's own published protocol `readme_loop`), the unprimed figure beside the
primed one, the render-side multi-GPU term measured on this GPU, whose `cpu_baseline` is measured in the same run, and whose
PMC constants are either those of THIS tree's kernels or flagged stale.  The full records are in bench_details.json."""
import json
import os
import subprocess
import sys

import numpy as np

import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_default_line_is_short_last_and_carries_every_config():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "SRZ_BENCH_FORCE_LAUNCHER")}
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--full", "--steps", "3", "--warmup", "1", "--cpu-budget-s", "2"],
                       capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    nonempty = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert nonempty and nonempty[-1].startswith('{"metric"'), r.stdout[-500:]          # nothing follows the line on stdout
    assert sum(ln.startswith('{"metric"') for ln in nonempty) == 1
    line = nonempty[-1]
    assert len(line) < 6000, len(line)
    d = json.loads(line)
    assert d["metric"] == "frames_per_sec" and d["unit"] == "frames/s" and d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["dtype"] == "f32" and d["vs_baseline"] is None
    assert d["config"]["workload"] == "spot_texture_1024" and d["config"]["frames_per_step"] == 256
    # the arguments taken literally (W warm-up steps from idle, K timed) beside the steady-state figure
    assert d["value"] > 0 and d["value_unprimed"] > 0 and d["ms_per_step_unprimed"] > 0 and d["priming_steps"] >= 19
    roof = d["roofline"]
    assert roof["bound"] == "hbm" and roof["peak"] == 8000.0 and 0.2 < roof["frac"] < 1.0 and abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-3
    assert 0.1 < roof["frac_unprimed"] < 1.0
    # the fraction against BOTH peaks: 8.0 TB/s spec and the 6.29 TB/s measured copy
    assert roof["peak_measured"] == 6290.0 and abs(roof["frac_measured"] - roof["achieved"] / 6290.0) < 1e-3 and roof["frac"] < roof["frac_measured"] < 1.3
    assert (roof["traffic"] is None) == bool(roof.get("traffic_stale"))          # fresh counters, or flagged — never silently old ones
    for k in ("c3", "c4", "c5"):                                                  # flat scalars: what the driver's parser keeps
        assert 0.05 < roof["frac_" + k] < 1.0 and roof["fps_" + k] > 0
        assert abs(roof["frac_measured_" + k] - roof["frac_" + k] * 8000.0 / 6290.0) < 2e-3
    pc = roof["per_config"]
    for w in ("c3", "c4", "c5", "readme", "c2_p7.5", "c2:draw", "c2:approx", "c3:approx", "c4:approx", "c5:approx"):
        assert "error" not in pc[w], pc[w]
        assert pc[w]["fps"] > 0 and 0.05 < pc[w]["frac"] < 1.0 and pc[w]["us"][2] > 0
    loop = pc["readme:readme_loop"]
    assert "error" not in loop, loop
    p10, med, p90 = loop["draw_ms_p10_med_p90"]
    assert 0 < p10 <= med <= p90 < 5.0 and loop["frames"] == 1000 and loop["ref_published_draw_ms"] == 17.06
    em = roof["multi_gpu_emulated"]
    assert "error" not in em, em
    for n in (2, 4, 8):
        e = em["c2"][f"N{n}"]
        assert len(e["ms"]) == n and min(e["ms"]) > 0 and 1.0 <= e["max_over_mean"] < 2.0
        assert e["pred_ms"]["planes"] >= e["pred_ms"]["bgr8"] >= max(e["ms"]) * 0.999
    assert len(em["c4"]["N8"]["ms"]) == 8 and len(em["c5"]["N8"]["ms"]) == 8
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["value"] > 0 and cb["cores"] >= 1 and cb["unit"] == "frames/s" and 0 < len(cb["sample"]) <= 200
    full = json.load(open(os.path.join(REPO, "bench_details.json")))
    assert any(e.get("scope") == "readme_loop" for e in full["configs"]) and len(full["configs"]) >= 11
    assert abs(full["value"] - d["value"]) <= 1e-4 * full["value"]


def test_plain_line_times_the_headline_only_and_dumps_the_same_outputs_every_run(tmp_path, orc):
    """without --full: exactly --steps timed steps of the headline, the contract's keys, none of what --full adds; --dump-outputs
    writes the seeded sample of the last step's framebuffer, bit-identical from run to run (same arguments, same inputs), and
    the sampled pixels are those of the frames their indices name (checked against the CPU oracle as smoke() checks a frame)"""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "SRZ_BENCH_FORCE_LAUNCHER")}
    dumps = []
    for run in ("a", "b"):
        out = tmp_path / run
        r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2",
                            "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, r.stderr[-3000:]
        nonempty = [ln for ln in r.stdout.splitlines() if ln.strip()]
        assert nonempty and nonempty[-1].startswith('{"metric"'), r.stdout[-500:]
        d = json.loads(nonempty[-1])
        assert d["metric"] == "frames_per_sec" and d["unit"] == "frames/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
        assert d["steps"] == 4 and d["warmup"] == 2 and d["roofline"]["launches_timed"] == 4 * d["roofline"]["lanes"]
        assert d["ms_per_step"] > 0 and abs(d["value"] - d["config"]["frames_per_step"] / d["ms_per_step"] * 1e3) <= 1e-3 * d["value"]
        assert "cpu_baseline" not in d and d["value_unprimed"] is None and not d["roofline"]["per_config"]
        assert "multi_gpu_emulated" not in d["roofline"] and d["roofline"]["frac"] is None   # (its bytes need --full's counting pass)
        files = sorted(p.name for p in out.iterdir())
        assert files == ["framebuffer_sample.npy", "framebuffer_sample_index.npy", "framebuffer_sample_nonfinite.npy"], files
        assert sum(p.stat().st_size for p in out.iterdir()) <= 64 << 20
        s, c, i = (np.load(out / f"framebuffer_sample{x}.npy") for x in ("", "_nonfinite", "_index"))
        assert s.dtype == c.dtype == np.float32 and s.shape == c.shape == (1 << 20, 4) and i.dtype == np.float64 and i.shape == (1 << 20,)
        assert np.isfinite(s).all() and np.isfinite(c).all() and np.isfinite(i).all()
        cov = c[:, 0] == 0                                                       # z of an uncovered pixel is +inf: code 1
        assert 0.02 < cov.mean() < 0.5 and set(np.unique(c[:, 0])) <= {0.0, 1.0} and (c[:, 1:] == 0).all()   # the spot covers part of every frame
        dumps.append((s, c, i))
    for a, b in zip(*dumps):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    # batch frame f is the workload's frame f % 36 (bench.Case); the sample's first and last frames against the oracle
    from srz import scenes as pscenes
    wl = pscenes.WORKLOADS["spot_texture_1024"]()
    s, c, i = dumps[0]
    k = i.astype(np.int64)
    fi, px = k // (1024 * 1024), k % (1024 * 1024)
    for f in sorted({int(fi[0]), int(fi[-1])}):
        frame = wl.frame(f % 36)
        for slot, tex in enumerate(wl.texture_arrays):
            orc.texture_set(slot, tex)
        rc, ref, _ = orc.draw(frame)
        assert rc == 0
        m = fi == f
        z = ref[0].reshape(-1)[px[m]]
        cov = np.isfinite(z)
        assert m.sum() > 1000 and np.array_equal(c[m, 0] == 1, ~cov) and (c[m, 0][cov] == 0).all()
        assert np.array_equal(s[m, 0][cov].view(np.uint32), z[cov].view(np.uint32)), f      # z bit-exact
        col = np.stack([p.reshape(-1)[px[m]] for p in ref[1:]], axis=1)
        d = np.abs(s[m, 1:] - col)
        assert float(d.max()) <= 1e-3 and int((d > 0).sum()) <= max(1, int(1e-5 * cov.sum())), (f, float(d.max()))
