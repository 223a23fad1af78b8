"""GPU: geometry mode sharded over two gloo ranks on the box's card (tests/geometry_shard_worker.py), and the same worker as
one RCCL rank with FUSG_DIST_FORCE=1 (every sharded code path through a one-rank communicator: nothing may differ).  The file
name sorts before the test_gpu_* modules: worker processes are started only from a process that has not initialised HIP."""
import os
import subprocess
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(world, extra_env):
    if torch.cuda.is_initialized():
        pytest.skip("this process has initialised HIP: worker processes are started only from a process that has not")
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    base = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    base.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world), **extra_env)
    procs = [subprocess.Popen([sys.executable, os.path.join(REPO, "tests", "geometry_shard_worker.py")], env={**base, "RANK": str(r)},
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(world)]
    try:
        outs = [p.communicate(timeout=600) for p in procs]
    except subprocess.TimeoutExpired:
        for p in procs:
            p.kill()
        raise
    assert all(p.returncode == 0 for p in procs), "\n".join(f"rank {r} rc {p.returncode}:\n{so[-1500:]}{se[-3000:]}"
                                                            for r, (p, (so, se)) in enumerate(zip(procs, outs)))
    assert "SHARD_OK" in outs[0][0], outs[0][0][-3000:] + outs[0][1][-2000:]
    sys.stdout.write(outs[0][0])
    return outs[0][0]


@pytest.mark.gpu
def test_geometry_mode_sharded_over_two_ranks():
    """5 vehicles as shards of 3 + 2 (one rendering empty), then 1 vehicle (rank 1's shard empty): sharded run_frame and two
    sharded run_later_frames give rank 0 its own unsharded results (integers and poses exactly, images within the bars of
    frame_shard_worker.BARS); sharded run_frames equals sharded run_frame bit for bit."""
    out = _run(2, {})
    assert any(ln.startswith("OBS ") for ln in out.splitlines())


@pytest.mark.gpu
def test_geometry_mode_one_rank_rccl():
    """The sharded geometry paths through a one-rank RCCL communicator: the shard is the whole frame, so sharded and unsharded
    results agree exactly (the worker's checks, with images compared within the same bars)."""
    _run(1, {"FUSG_TEST_BACKEND": "nccl", "FUSG_DIST_FORCE": "1"})
