"""One process of the sharded power-flow-report test (tests/test_gpu_powerflow.py), in tests/losses_worker.py's pattern (the
engine and the test data of tests/network_worker.py are imported): two processes over gloo, each rank owning a
node-aligned share of the residences on cuda:0, a few iterations of the real loop, then the power-flow report of the
schedule (active only) and of a given profile (with reactances).  Every rank stores its whole report for the parent to
compare with the one-rank run.

    python tests/powerflow_worker.py spec.json"""
import datetime
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))


def reports(e, w, lo, hi, steps):
    import numpy as np
    from network_worker import line_ratings, profile_of
    _, nodes = line_ratings(w)
    edge_x = 0.5 * np.asarray(w.edge_r, np.float64)
    e.run_steps(steps)
    out = {}
    for tag, rep in (("sch", e.powerflow_report(nodes=nodes)),
                     ("prof", e.powerflow_report(profile=profile_of(w)[lo:hi], edge_x=edge_x, power_factor=0.95, vmin=0.97,
                                                 slot_hours=0.5))):
        for k in ("volt", "volt_lin", "flow", "loss") + (("qflow",) if tag == "prof" else ()):
            out[f"{tag}_{k}"] = getattr(rep, k)
        for k in ("summary", "slot", "node_day"):
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
    np.savez(os.path.join(spec["outdir"], f"pf_r{rank}.npz"), **reports(e, w, lo, hi, case["steps"]))
    del e
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
