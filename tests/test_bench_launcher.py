"""bench.py started plainly with --gpus N > 1 is its own launcher (reference layout:
train1.py:152-171 spawns one worker per GPU).  On CPU: two gloo ranks drive bench.py's OWN launcher,
rendezvous, DistributedSampler-equal sharding, FlatDataParallel wrap, step loop, fences, max-over-ranks
timing and JSON line with the plain-torch stand-in model (--selftest-cpu; the HIP model cannot run without
a GPU and there is no CPU fallback).  On the GPU box: the same launcher with the real HIP model, two ranks
sharing the one card (gloo, host-staged collectives)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(args, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, BENCH] + args, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, f"expected ONE JSON line on stdout, got {len(lines)}:\n{r.stdout[-2000:]}"
    return json.loads(lines[0])


@pytest.mark.parametrize("mtype", ["vaetf", "scavaetf"])
def test_plain_gpus2_spawns_two_ranks_cpu(mtype):
    out = _run(["--gpus", "2", "--steps", "4", "--warmup", "1", "--batch", "8", "--model-type", mtype,
                "--selftest-cpu", "--full"])
    assert out["n_gpus"] == 2 and out["ranks"] == 2 and out["launcher"] == "self-spawn"
    assert out["backend"] == "gloo" and out["steps"] == 4 and out["warmup"] == 1
    assert out["config"]["global_batch"] == 16 and out["config"]["parallelism"] == "dp2"
    assert out["scaling"] == "weak" and out["ms_per_step"] > 0
    assert abs(out["value"] - 16 * 4 / (out["ms_per_step"] * 4e-3)) / out["value"] < 1e-2
    assert "self-test" in out["metric"]              # can never be mistaken for a benchmark line
    # the multi-rank report of the line (what a first run on real GPUs is read by): both ranks seen and named,
    # the gradient exchange counted per backward pass, parameters bit-identical across ranks, the overlap-off A/B leg
    mr = out["multi_rank"]
    assert mr["ranks_seen"] == 2 and [i["rank"] for i in mr["identities"]] == [0, 1]
    assert len({i["pid"] for i in mr["identities"]}) == 2
    assert mr["parameter_checksum_max_minus_min"] == 0
    ex = mr["exchange_rank0"]
    assert ex["backward_passes"] == 4 and ex["buckets"] >= 1
    assert abs(ex["buckets_in_backward_per_pass"] + ex["buckets_at_finalize_per_pass"] - ex["buckets"]) < 1e-6
    assert ex["exposed_wait_ms_median"] is not None and mr["exposed_wait_ms_max_over_ranks"] >= 0
    assert len(mr["host_ms_per_step"]) == 2 and all(h > 0 for h in mr["host_ms_per_step"])
    assert mr["same_step_overlap_off"]["ms_per_step"] > 0


# what the line carries only under --full (every further leg and check after the timed steps)
FULL_ONLY = {"fixed_len_80", "every_decoder_row", "same_step_fp32_mfma_gemms", "trainer_loop", "model_types", "decode",
             "multi_rank", "box", "cpu_baseline"}


def test_plain_gpus2_carries_the_headline_only_cpu():
    out = _run(["--gpus", "2", "--steps", "2", "--warmup", "1", "--batch", "8", "--selftest-cpu"])
    assert out["ranks"] == 2 and out["steps"] == 2 and out["ms_per_step"] > 0
    assert not FULL_ONLY & set(out)


def test_single_rank_cpu_selftest_and_world_mismatch():
    out = _run(["--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "8", "--selftest-cpu"])
    assert out["n_gpus"] == 1 and out["launcher"] == "single process"
    env = dict(os.environ, WORLD_SIZE="3", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--selftest-cpu"], env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode != 0 and "does not match" in r.stderr


def test_dead_rank_fails_the_launch():
    """a worker that dies must take the launch down (non-zero exit), not leave the others in a collective"""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env["GCT_BENCH_SELFTEST_DIE"] = "1"
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "2", "--warmup", "1", "--batch", "8",
                        "--selftest-cpu"], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 3 and not [l for l in r.stdout.splitlines() if l.startswith("{")]


def _load_dump(d):
    import numpy as np
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def test_dump_outputs_cpu_selftest_is_repeatable(tmp_path):
    """--dump-outputs writes the last timed step's outputs, float32 / float64 only; the same arguments give the same
    inputs, so two runs write the same arrays, and the loss written is the one the line reports for the last step."""
    import numpy as np
    dumps = []
    for run in ("a", "b"):
        d = str(tmp_path / run)
        out = _run(["--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "8", "--selftest-cpu", "--dump-outputs", d])
        assert out["steps"] == 3 and out["ms_per_step"] > 0
        dumps.append(_load_dump(d))
        assert sorted(out["dumped_outputs"]) == sorted(dumps[-1])
    a, b = dumps
    assert {"loss", "logits", "parameters", "gradients"} <= set(a) and a.keys() == b.keys()
    for n in a:
        assert a[n].dtype in (np.float32, np.float64) and np.isfinite(a[n]).all(), n
        assert np.array_equal(a[n], b[n]), n
    assert sum(v.nbytes for v in a.values()) <= 64 * 2 ** 20
    assert abs(float(a["loss"]) / 8 - out["final_loss_per_sample"]) < 1e-3


@pytest.mark.gpu
def test_dump_outputs_real_model(tmp_path):
    import numpy as np
    d = str(tmp_path / "dump")
    out = _run(["--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "8", "--model-type", "pvaetf", "--tiny",
                "--no-alt-mode", "--no-fixed-len-leg", "--dump-outputs", d], timeout=900)
    got = _load_dump(d)
    assert set(got) == {"loss", "logits", "mu", "logvar", "prop", "parameters", "gradients"}
    for n, v in got.items():
        assert v.dtype in (np.float32, np.float64) and np.isfinite(v).all(), n
    assert got["logits"].ndim == 3 and got["logits"].shape[0] == 8 and np.abs(got["gradients"]).max() > 0
    assert abs(float(got["loss"]) / 8 - out["final_loss_per_sample"]) < 1e-3 * abs(out["final_loss_per_sample"]) + 1e-4


@pytest.mark.gpu
def test_plain_run_real_model_carries_the_headline_only():
    out = _run(["--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "8", "--tiny"], timeout=900)
    assert out["metric"].startswith("SMILES/sec training step (vaetf") and out["steps"] == 2 and out["ms_per_step"] > 0
    assert "roofline" in out and "host" in out
    assert not FULL_ONLY & set(out)


@pytest.mark.gpu
def test_plain_gpus2_real_model_shared_gpu():
    out = _run(["--gpus", "2", "--steps", "3", "--warmup", "2", "--batch", "8", "--model-type", "scavaetf",
                "--tiny", "--share-gpu", "--no-alt-mode", "--full"], timeout=900)
    assert out["ranks"] == 2 and out["launcher"] == "self-spawn" and out["n_gpus"] == 2
    assert out["metric"].startswith("SMILES/sec training step (scavaetf")
    assert out["roofline"] is None or "kernel" in out["roofline"]
    assert out["fixed_len_80"]["ms_per_step"] > 0
    assert out["final_loss_per_sample"] == out["final_loss_per_sample"]      # not NaN
    mr = out["multi_rank"]
    assert mr["ranks_seen"] == 2 and mr["parameter_checksum_max_minus_min"] == 0
    ex = mr["exchange_rank0"]
    # per-layer buckets leave from inside the trunk backward once the dead set is known (after the first pass)
    assert ex["buckets_in_backward_per_pass"] > 0 and ex["exposed_wait_ms_median"] is not None


def test_replay_switch_children_never_raise():
    """bench.py's slow-replay diagnosis starts child processes; without a GPU (or past its time budget) it must come
    back with one record per runtime switch -- an error text or 'skipped' -- and never raise into the bench line."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    recs = mod.replay_switch_children(budget_s=-1.0)          # budget already spent: nothing is started
    assert len(recs) == 5 and all(r.get("skipped") == "time budget" and "env" in r for r in recs)
