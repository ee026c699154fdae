"""One process of the sharded transformer-report test (tests/test_gpu_transformers.py), in tests/losses_worker.py's
pattern (the engine and the test data of tests/network_worker.py are imported): two processes over gloo, each rank owning
a node-aligned share of the residences on cuda:0, a few iterations of the real loop, then the transformer report of the
schedule and of a given profile.  Every rank stores its whole report for the parent to compare with the one-rank run.

    python tests/transformers_worker.py spec.json"""
import datetime
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))


def fleet_of(w):
    """Data of the test, the same on every rank: five node rows per transformer (the last rows owned by nobody) and
    ratings off the ladder."""
    import numpy as np
    xf_of = np.arange(w.M) // 5
    xf_of[-7:] = -1
    K = int(xf_of.max()) + 1
    return xf_of, np.random.default_rng(13).choice([50.0, 75.0, 100.0, 167.0], K)


def reports(e, w, lo, hi, steps):
    import numpy as np
    from network_worker import profile_of
    xf_of, kva = fleet_of(w)
    e.run_steps(steps)
    out = {}
    for tag, rep in (("sch", e.transformer_report(xf_of, kva)),
                     ("prof", e.transformer_report(xf_of, kva, profile=profile_of(w)[lo:hi], substeps=4, slot_hours=0.5,
                                                   initial=(10.0, 2.0), hot_limit=90.0))):
        for k in ("load", "ratio", "top_oil", "hot_spot", "faa"):
            out[f"{tag}_{k}"] = getattr(rep, k)
        for k in ("summary_ratio", "summary_hot", "xf_day"):
            out[f"{tag}_{k}"] = getattr(rep, k).view(np.uint8)
        out[f"{tag}_fleet"] = np.frombuffer(rep.fleet.tobytes(), np.uint8)
    out["iteration"] = np.asarray(e.iteration)
    return out


def main():
    spec = json.load(open(sys.argv[1]))
    import numpy as np
    import torch
    import torch.distributed as dist
    from network_worker import engine
    from sharded_worker import make_case, node_aligned_split
    rank, world, case = spec["rank"], spec["world"], spec["case"]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(spec["port"]))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    torch.cuda.set_device(0)
    w = make_case(case)
    cuts = node_aligned_split(w.node_of, world)
    lo, hi = int(cuts[rank]), int(cuts[rank + 1])
    counts = np.bincount(w.node_of, minlength=w.M)

    def hook(a, op):
        dist.all_reduce(torch.from_numpy(a), op={0: dist.ReduceOp.SUM, 2: dist.ReduceOp.MAX, 3: dist.ReduceOp.MIN}[op])

    e = engine(w, lo, hi, dist.group.WORLD, counts, hook)
    assert e._comm is not None
    np.savez(os.path.join(spec["outdir"], f"xf_r{rank}.npz"), **reports(e, w, lo, hi, case["steps"]))
    del e
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
