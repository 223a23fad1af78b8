"""GPU: a sharded later frame with scene['inpaint'] = {'boxes', 'box_masks'} over two gloo ranks on the box's card
(tests/later_inpaint_shard_worker.py): rank 0's result equals its own unsharded call.  The file name sorts before the test_gpu_*
modules: worker processes are started only from a process that has not initialised HIP."""
import os
import subprocess
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_later_frame_with_box_masks_sharded_over_two_ranks():
    if torch.cuda.is_initialized():
        pytest.skip("this process has initialised HIP: worker processes are started only from a process that has not")
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    base = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    base.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, os.path.join(REPO, "tests", "later_inpaint_shard_worker.py")], env={**base, "RANK": str(r)},
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(2)]
    try:
        outs = [p.communicate(timeout=300) for p in procs]
    except subprocess.TimeoutExpired:
        for p in procs:
            p.kill()
        raise
    assert all(p.returncode == 0 for p in procs), "\n".join(f"rank {r} rc {p.returncode}:\n{so[-1500:]}{se[-3000:]}"
                                                            for r, (p, (so, se)) in enumerate(zip(procs, outs)))
    assert "SHARD_OK" in outs[0][0], outs[0][0][-3000:] + outs[0][1][-2000:]
    sys.stdout.write(outs[0][0])
