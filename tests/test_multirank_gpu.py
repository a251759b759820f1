"""Multi-rank engine paths ON THE GPU.

RCCL refuses two ranks on one device ("Duplicate GPU detected", RCCL
2.26.6 — probe log profiles/r02_multirank_probe.md), and the gpurun box
is an SR-IOV virtual function whose compute partition (CPX) is
host-controlled, so one physical MI355X cannot present multiple RCCL
devices.  These tests therefore run the full multi-rank engine path —
sharded weights, HIP kernels, TP all-reduce / all-gather, KV handoff —
with collectives host-staged over gloo (lws_amd.parallel.tp
ParallelState.staged).  On a node with >= world GPUs the same code paths
select RCCL automatically (init_distributed backend auto-pick), which is
what the driver's 8-GPU SCALE run exercises.
"""
import json
import multiprocessing as mp
import os
import subprocess
import sys

import pytest
import torch

from conftest import free_port
from test_engine import _clean_worker_exit

gpu = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _env_for(rank, world, port):
    return {
        "RANK": str(rank), "WORLD_SIZE": str(world),
        "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port),
        "LOCAL_RANK": str(rank),
    }


def _tp_gpu_worker(rank, world, port, q):
    os.environ.update(_env_for(rank, world, port))
    from lws_amd.parallel.tp import init_distributed, parallel_state

    init_distributed(device="cuda:0")   # backend auto: gloo on 1-GPU box
    import lws_amd.ops as ops
    ops.require_native()                 # HIP extension must be live
    from lws_amd.serving.engine import Engine, EngineConfig

    cfg = EngineConfig(model="llama-tiny", kv_pages=64, device="cuda:0",
                       seed=7, tp_rank=rank, tp_world=world,
                       max_model_len=512)
    eng = Engine(cfg)
    eng.load()
    prompt = [5, 17, 250, 3]
    out = eng.generate([prompt], max_new_tokens=3)[0]
    eng2 = Engine(EngineConfig(model="llama-tiny", kv_pages=64,
                               device="cuda:0", seed=7, tp_rank=rank,
                               tp_world=world, max_model_len=512))
    eng2.load()
    out2 = eng2.generate([prompt + out[:2]], max_new_tokens=1)[0]
    q.put((rank, out, out2, parallel_state().staged))
    _clean_worker_exit(q)


def _run_ranks(target, world, extra=()):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=target, args=(r, world, port, q) + tuple(extra))
             for r in range(world)]
    for p in procs:
        p.start()
    results = {}
    try:
        for _ in range(world):
            item = q.get(timeout=600)
            results[item[0]] = item[1:]
    finally:
        for p in procs:
            p.join(timeout=120)
            if p.is_alive():
                p.terminate()
    assert all(p.exitcode == 0 for p in procs), \
        [f"rank exit {p.exitcode}" for p in procs]
    return results


@gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")
def test_tp2_engine_consistency_gpu():
    """TP=2, both shards on one MI355X, HIP kernels + staged collectives:
    ranks agree on tokens and decode is consistent with prefill."""
    results = _run_ranks(_tp_gpu_worker, 2)
    assert results[0][0] == results[1][0], "ranks disagree on tokens"
    out, out2, staged = results[0]
    assert out2[0] == out[2], "TP decode/prefill inconsistency"
    if torch.cuda.device_count() < 2:
        assert staged, "expected host-staged collectives on a 1-GPU box"


def _handoff_gpu_worker(rank, world, port, q):
    os.environ.update(_env_for(rank, world, port))
    from lws_amd.parallel.tp import init_distributed

    init_distributed(device="cuda:0")
    import lws_amd.ops as ops
    ops.require_native()
    from lws_amd.serving.engine import Engine, EngineConfig
    from lws_amd.serving.handoff import recv_kv, send_kv

    cfg = EngineConfig(model="llama-tiny", kv_pages=64, device="cuda:0",
                       seed=11, max_model_len=512)
    eng = Engine(cfg)
    eng.load()
    prompt = [9, 3, 77, 200, 5]
    if rank == 0:   # prefill role
        sid = eng.add_request(prompt)
        eng.step()                       # prefill + first token
        first = eng.sequences[sid].token_ids[-1]
        send_kv(eng, sid, dst=1)
        q.put((rank, first))
        _clean_worker_exit(q)
    else:           # decode role
        sid = recv_kv(eng, src=0)
        toks = []
        for _ in range(3):
            out = eng.step()
            toks.append(out[sid])
        # reference: same engine runs the whole thing locally
        ref = Engine(cfg)
        ref.load()
        ref_out = ref.generate([prompt], max_new_tokens=4)[0]
        q.put((rank, (eng.sequences[sid].token_ids[len(prompt):], ref_out)))
        _clean_worker_exit(q)


@gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")
def test_kv_handoff_2rank_gpu():
    """Disaggregated prefill->decode handoff between two GPU processes:
    the decode role's continuation must equal a single-engine run."""
    results = _run_ranks(_handoff_gpu_worker, 2)
    got, ref = results[1][0]
    assert got == ref, f"handoff continuation {got} != local {ref}"


@gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")
def test_bench_two_rank_gpu():
    """The driver's N=2 launch shape on one GPU: full control plane +
    2-shard collective engine bring-up + rolling update, end to end."""
    port = free_port()
    procs = []
    for rank in range(2):
        env = dict(os.environ)
        env.update(_env_for(rank, 2, port))
        cmd = [sys.executable, os.path.join(REPO, "bench.py"),
               "--model", "llama-tiny", "--kv-pages", "64",
               "--decode-batch", "4", "--prompt-len", "16",
               "--decode-steps", "4", "--gpus", "2", "--steps", "1",
               "--warmup", "0", "--full"]
        procs.append(subprocess.Popen(cmd, stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True,
                                      env=env, cwd=REPO))
    outs = []
    for p in procs:
        stdout, stderr = p.communicate(timeout=900)
        assert p.returncode == 0, stderr[-4000:]
        outs.append(stdout)
    line = next(l for l in outs[0].splitlines() if l.strip().startswith("{"))
    out = json.loads(line)
    assert out["n_gpus"] == 2
    assert out["config"]["parallelism"] == "tp2"
    assert out["value"] > 0
    if torch.cuda.device_count() < 2:
        assert out["config"]["collectives_staged"] is True
    else:
        assert out["config"]["backend"] == "nccl"


def _pp_gpu_worker(rank, world, port, q):
    os.environ.update(_env_for(rank, world, port))
    from lws_amd.parallel.tp import init_distributed

    init_distributed(device="cuda:0")
    import lws_amd.ops as ops
    ops.require_native()
    from lws_amd.serving.engine import Engine, EngineConfig

    cfg = EngineConfig(model="llama-tiny", kv_pages=64, device="cuda:0",
                       seed=13, pp_rank=rank, pp_world=world,
                       max_model_len=512)
    eng = Engine(cfg)
    eng.load()
    out = eng.generate([[2, 7, 1, 8]], max_new_tokens=3)[0]
    ref = None
    if rank == world - 1:
        # single-process reference on the same seed
        r = Engine(EngineConfig(model="llama-tiny", kv_pages=64,
                                device="cuda:0", seed=13, max_model_len=512))
        r.load()
        ref = r.generate([[2, 7, 1, 8]], max_new_tokens=3)[0]
    q.put((rank, out, ref))
    _clean_worker_exit(q)


@gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")
def test_pp2_engine_exact_equivalence_gpu():
    """2-stage pipeline parallelism on one MI355X (HIP kernels, staged
    activation transfer): tokens must EXACTLY match the single-process
    engine — PP is a pure partition of the same computation."""
    results = _run_ranks(_pp_gpu_worker, 2)
    out_last, ref = results[1]
    assert ref is not None
    assert out_last == ref, f"PP tokens {out_last} != single-process {ref}"
    assert results[0][0] == out_last, "stages disagree on the token stream"


@gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")
def test_bench_eight_rank_gpu():
    """The NAMED headline group shape — 1 leader + 7 workers (size 8) —
    as 8 processes on this GPU: full rendezvous, 8-way sharded bring-up,
    rolling update.  (llama-tiny8 weights; the 70B version of this exact
    run is recorded in BASELINE.md / gpurun_out/r02_tp8_staged.log.)"""
    port = free_port()
    procs = []
    for rank in range(8):
        env = dict(os.environ)
        env.update(_env_for(rank, 8, port))
        cmd = [sys.executable, os.path.join(REPO, "bench.py"),
               "--model", "llama-tiny8", "--kv-pages", "64",
               "--decode-batch", "4", "--prompt-len", "16",
               "--decode-steps", "2", "--gpus", "8", "--steps", "1",
               "--warmup", "0", "--skip-decode-bench"]
        procs.append(subprocess.Popen(cmd, stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True,
                                      env=env, cwd=REPO))
    outs = []
    for p in procs:
        stdout, stderr = p.communicate(timeout=900)
        assert p.returncode == 0, stderr[-4000:]
        outs.append(stdout)
    line = next(l for l in outs[0].splitlines() if l.strip().startswith("{"))
    out = json.loads(line)
    assert out["n_gpus"] == 8
    assert out["config"]["parallelism"] == "tp8"
    assert out["config"]["group"] == "1-leader/7-workers (size=8)"
    assert out["value"] > 0
