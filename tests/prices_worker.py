"""One process of the sharded price-report test (tests/test_gpu_prices.py), in tests/losses_worker.py's pattern (the
engine and the test data of tests/network_worker.py are imported): two processes over gloo, each rank owning a
node-aligned share of the residences on cuda:0, a few iterations of the real loop, then the price report of the schedule
under the operator's own multipliers and of a given profile under given ones.  Every rank stores its whole report for
the parent to compare with the one-rank run.

    python tests/prices_worker.py spec.json"""
import datetime
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

ARRAYS = ("price", "cong", "lossp", "line_y", "rent", "drop", "flow")


def given_multipliers(w, seed=13):
    """Signed multipliers on a twentieth of the rows: data of the test, the same on every rank."""
    import numpy as np
    rng = np.random.default_rng(seed)
    return np.where(rng.random((w.M, w.load.shape[1])) < 0.05, rng.normal(0.0, 0.5, (w.M, w.load.shape[1])), 0.0)


def reports(e, w, lo, hi, steps):
    import numpy as np
    from network_worker import line_ratings, profile_of
    _, nodes = line_ratings(w)
    e.run_steps(steps)
    out = {}
    for tag, rep in (("sch", e.price_report(lines=nodes, nodes=nodes, scale=0.5)),
                     ("prof", e.price_report(profile=profile_of(w)[lo:hi], multipliers=given_multipliers(w), price_cap=0.2,
                                             slot_hours=0.5))):
        for k in ARRAYS:
            out[f"{tag}_{k}"] = getattr(rep, k)
        for k in ("summary", "slot", "node_day", "line_day"):
            out[f"{tag}_{k}"] = getattr(rep, k).view(np.uint8)
        out[f"{tag}_day"] = np.frombuffer(rep.day.tobytes(), np.uint8)
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
    assert e._comm is not None and e._tree is not None
    np.savez(os.path.join(spec["outdir"], f"price_r{rank}.npz"), **reports(e, w, lo, hi, case["steps"]))
    del e
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
