"""CPU, world_size 2 over gloo: two ranks write checkpoint-<step> directories together (every rank its sampler state, rank 0
the shared files, one rename behind a barrier) and both resume from checkpoint-2 into the uninterrupted two-rank run."""
import json
import os
import socket
import sys

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, root_a, root_b, q):
    sys.path.insert(0, REPO)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    from llamarec_amd import dist as DD
    from tests import resume_fakes as F

    r, w, _ = DD.init_from_env(backend="gloo")
    out = {}
    # per rank: 2 micro-batches of 2 per optimizer step; 2 ranks -> 8 samples per step, 4 steps per epoch
    for tag, root, resume in (("a", root_a, None), ("b", root_b, os.path.join(root_a, "checkpoint-2"))):
        tr, eng = F.make_trainer(F.lora_args(2, 4, resume_from_checkpoint=resume), root, rank=r, world=w)
        steps = tr.train()
        DD.barrier()
        out[tag] = (steps, eng.seen, eng.params.numpy().copy(), eng.m.numpy().copy(), eng.v.numpy().copy(), eng.passes, tr.history)
    q.put((r, out))
    dist.destroy_process_group()


def test_two_ranks_checkpoint_together_and_resume_into_the_uninterrupted_run(tmp_path):
    root_a, root_b = str(tmp_path / "a"), str(tmp_path / "b")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, root_a, root_b, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=120) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for r in range(2):
        a, b = got[r]["a"], got[r]["b"]
        assert a[0] == b[0] == 6
        assert len(a[1]) == 12 and a[1][4:] == b[1]                         # the passes after step 2, sample for sample
        for x, y in zip(a[2:5], b[2:5]):
            assert np.array_equal(x, y)
        assert a[5] == b[5] == 12 and a[6] == b[6] and len(a[6]) == 3
    assert np.array_equal(got[0]["a"][2], got[1]["a"][2])                   # the ranks agree (one averaged gradient)
    assert got[0]["a"][1] != got[1]["a"][1]                                 # ... on different samples
    from safetensors.torch import load_file

    shared = ["adapter_config.json", "adapter_model.safetensors", "best_adapter_model.safetensors", "optimizer.safetensors"]
    for root, steps in ((root_a, (2, 4, 6)), (root_b, (4, 6))):
        assert sorted(d for d in os.listdir(root) if d.startswith("checkpoint")) == [f"checkpoint-{s}" for s in steps]
        for s in steps:
            assert sorted(os.listdir(os.path.join(root, f"checkpoint-{s}"))) == \
                shared + ["rng_state_0.json", "rng_state_1.json", "trainer_state.json"]
    r0, r1 = (json.load(open(os.path.join(root_a, "checkpoint-4", f"rng_state_{r}.json"))) for r in range(2))
    assert r0 != r1
    for s in (4, 6):
        sa, sb = (json.load(open(os.path.join(r, f"checkpoint-{s}", "trainer_state.json"))) for r in (root_a, root_b))
        assert sa == sb and sa["fingerprint"]["world_size"] == 2 and sa["passes_per_rank"] == [2 * s, 2 * s]
        for f in shared[1:] + ["rng_state_0.json", "rng_state_1.json"]:
            pa, pb = (os.path.join(r, f"checkpoint-{s}", f) for r in (root_a, root_b))
            if f.endswith(".json"):
                assert json.load(open(pa)) == json.load(open(pb)), (s, f)
            else:
                ta, tb = load_file(pa), load_file(pb)
                assert sorted(ta) == sorted(tb) and all(torch.equal(ta[k], tb[k]) for k in ta), (s, f)
