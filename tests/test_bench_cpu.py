"""CPU dry-runs of bench.py — the same path the driver runs on MI355X,
with llama-tiny on the fp32 reference ops and gloo collectives."""
import json
import os
import random
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_bench(env_extra, args):
    env = dict(os.environ)
    env.update(env_extra)
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--device", "cpu",
           "--model", "llama-tiny", "--kv-pages", "64", "--decode-batch", "4",
           "--prompt-len", "16", "--decode-steps", "4"] + args
    return subprocess.run(cmd, capture_output=True, text=True, env=env,
                          cwd=REPO, timeout=600)


def _parse_json_line(stdout):
    for line in stdout.splitlines():
        line = line.strip()
        if line.startswith("{"):
            return json.loads(line)
    raise AssertionError(f"no JSON line in output:\n{stdout}")


def test_bench_single_process():
    r = _run_bench({}, ["--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--full"])
    assert r.returncode == 0, r.stderr[-4000:]
    out = _parse_json_line(r.stdout)
    assert out["n_gpus"] == 1
    assert out["steps"] == 2
    assert out["ms_per_step"] > 0
    assert out["higher_is_better"] is False
    assert out["value"] > 0
    assert out["config"]["rollout_ms_p50"] > 0
    assert out["config"]["decode_tokens_per_s"] > 0
    assert out["config"]["parallelism"] == "tp1"


def test_bench_plain_run_dumps_reproducible_outputs(tmp_path):
    """A plain run measures the headline only (no decode figures), and
    --dump-outputs writes float32 arrays that are identical from run to
    run with the same arguments."""
    import numpy as np

    dumps = []
    for name in ("a", "b"):
        d = tmp_path / name
        r = _run_bench({}, ["--gpus", "1", "--steps", "2", "--warmup", "0",
                            "--dump-outputs", str(d)])
        assert r.returncode == 0, r.stderr[-4000:]
        out = _parse_json_line(r.stdout)
        assert out["steps"] == 2
        assert out["ms_per_step"] > 0
        assert out["config"]["decode_tokens_per_s"] is None
        dumps.append({p.name: np.load(p) for p in sorted(d.glob("*.npy"))})
    a, b = dumps
    assert set(a) == set(b) == {"warmup_k_cache.npy", "warmup_v_cache.npy",
                                "qkv_weight_sample.npy",
                                "lm_head_weight_sample.npy"}
    for name, arr in a.items():
        assert arr.dtype == np.float32
        assert np.isfinite(arr).all()
        assert np.array_equal(arr, b[name]), name
    # the warmup wrote 5 positions (4 prompt + 1 decoded) of the page in
    # every layer; the rest of the page is still the zero-initialised pool
    k = a["warmup_k_cache.npy"]                # [L, Hkv, page, D]
    assert (np.abs(k[:, :, :5]).max(axis=(0, 1, 3)) > 0).all()
    assert not k[:, :, 5:].any()
    assert sum(arr.nbytes for arr in a.values()) <= 64 * 2 ** 20


def test_dump_outputs_holds_its_size_budget(tmp_path):
    """An array over its share of the byte budget is replaced by a fixed
    seeded sample, so the limit holds for any model size."""
    import numpy as np
    import torch

    sys.path.insert(0, REPO)
    import bench

    assert bench.DUMP_BUDGET_BYTES == 64 * 2 ** 20
    outs = {"big": torch.arange(1000, dtype=torch.bfloat16),
            "small": torch.ones(10)}
    for name in ("a", "b"):
        bench.dump_outputs(outs, str(tmp_path / name), budget_bytes=400)
    big = np.load(tmp_path / "a" / "big.npy")
    small = np.load(tmp_path / "a" / "small.npy")
    assert big.dtype == small.dtype == np.float32
    assert big.shape == (50,) and small.shape == (10,)
    assert big.nbytes + small.nbytes <= 400
    assert np.isin(big, outs["big"].float().numpy()).all()
    assert np.array_equal(big, np.load(tmp_path / "b" / "big.npy"))


def _two_rank_attempt(port, timeout=240):
    procs = []
    for rank in range(2):
        env = {"RANK": str(rank), "WORLD_SIZE": "2",
               "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port),
               "LOCAL_RANK": str(rank)}
        p_env = dict(os.environ)
        p_env.update(env)
        cmd = [sys.executable, os.path.join(REPO, "bench.py"),
               "--device", "cpu", "--model", "llama-tiny", "--kv-pages", "64",
               "--decode-batch", "4", "--prompt-len", "16",
               "--decode-steps", "4", "--gpus", "2", "--steps", "1",
               "--warmup", "0", "--full"]
        procs.append(subprocess.Popen(cmd, stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True,
                                      env=p_env, cwd=REPO))
    outs = []
    try:
        for p in procs:
            stdout, stderr = p.communicate(timeout=timeout)
            assert p.returncode == 0, stderr[-4000:]
            outs.append(stdout)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    return outs


def test_bench_two_rank_gloo():
    """Two ranks over gloo — the distributed path the driver exercises with
    torch.distributed.run on the GPU box.  OS-assigned rendezvous port
    (conftest.free_port) instead of the old random+retry pattern."""
    from conftest import free_port
    outs = _two_rank_attempt(free_port())
    out = _parse_json_line(outs[0])
    assert out["n_gpus"] == 2
    assert out["config"]["parallelism"] == "tp2"
    assert out["value"] > 0


def test_bench_four_rank_gloo():
    """4-rank gloo dry-run of the driver's N=4 launch shape (TP=4 over
    the collective runtime; llama-tiny4 divides 4 kv heads)."""
    from conftest import free_port

    for attempt in range(1):
        port = free_port()
        procs = []
        for rank in range(4):
            p_env = dict(os.environ)
            p_env.update({"RANK": str(rank), "WORLD_SIZE": "4",
                          "MASTER_ADDR": "127.0.0.1",
                          "MASTER_PORT": str(port),
                          "LOCAL_RANK": str(rank)})
            cmd = [sys.executable, os.path.join(REPO, "bench.py"),
                   "--device", "cpu", "--model", "llama-tiny4",
                   "--kv-pages", "64", "--decode-batch", "4",
                   "--prompt-len", "16", "--decode-steps", "2",
                   "--gpus", "4", "--steps", "1", "--warmup", "0",
                   "--full"]
            procs.append(subprocess.Popen(cmd, stdout=subprocess.PIPE,
                                          stderr=subprocess.PIPE, text=True,
                                          env=p_env, cwd=REPO))
        try:
            outs = []
            ok = True
            for p in procs:
                stdout, stderr = p.communicate(timeout=300)
                if p.returncode != 0:
                    ok = False
                    last_err = stderr[-3000:]
                outs.append(stdout)
            if ok:
                out = _parse_json_line(outs[0])
                assert out["n_gpus"] == 4
                assert out["config"]["parallelism"] == "tp4"
                assert out["value"] > 0
                return
        except subprocess.TimeoutExpired:
            last_err = "timeout"
        finally:
            for p in procs:
                if p.poll() is None:
                    p.kill()
    raise AssertionError(f"4-rank bench failed 3 attempts: {last_err}")
