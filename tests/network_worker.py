"""One process of the sharded network-report tests (tests/test_gpu_network.py), in tests/sharded_worker.py's pattern
(its helpers are imported): two processes over gloo, or `world` logical ranks in one process -- each rank owns a
node-aligned share of the residences on cuda:0, runs a few iterations of the real loop, then takes the report of the
schedule and of a given profile.  Every rank stores its whole report for the parent to compare with the one-rank run.

    python tests/network_worker.py spec.json"""
import datetime
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))


def line_ratings(w, seed=11):
    """Ratings of the workload's lines (some unrated) and a node subset: data of the test, the same on every rank."""
    import numpy as np
    rng = np.random.default_rng(seed)
    rating = rng.uniform(30.0, 400.0, w.M)
    rating[rng.random(w.M) < 0.1] = np.nan
    return rating, np.flatnonzero(rng.random(w.M) < 0.7)


def profile_of(w, seed=12):
    import numpy as np
    return np.random.default_rng(seed).uniform(0.0, 6.0, w.load.shape).astype(np.float32)


def reports(e, w, lo, hi, steps):
    import numpy as np
    rating, nodes = line_ratings(w)
    e.run_steps(steps)
    out = {}
    for tag, rep in (("sch", e.network_report(rating=rating, nodes=nodes)),
                     ("prof", e.network_report(profile=profile_of(w)[lo:hi], rating=rating, nodes=nodes))):
        for k in ("flow", "loading", "volt", "node_sums"):
            out[f"{tag}_{k}"] = getattr(rep, k)
        out[f"{tag}_sl"] = rep.summary_loading.view(np.uint8)
        out[f"{tag}_sv"] = rep.summary_volt.view(np.uint8)
    out["iteration"] = np.asarray(e.iteration)
    return out


def engine(w, lo, hi, group, counts, hook=None):
    from revs_admm_amd.engine import AdmmEngine
    return AdmmEngine(w.cost, w.homes[lo:hi], w.load[lo:hi], w.node_of[lo:hi], w.Rn, kappa=w.kappa, vset=w.vset,
                      vlow=w.vlow, vhigh=w.vhigh, mode="pdhg", device="cuda:0", group=group, node_counts=counts,
                      feeder=w.feeder, comm_hook=hook)


def main_local(spec):
    import threading
    import traceback
    import numpy as np
    import torch
    from revs_admm_amd.comm import LocalRanks
    from sharded_worker import make_case, node_aligned_split
    world, case = spec["world"], spec["case"]
    torch.cuda.set_device(0)
    w = make_case(case)
    cuts = node_aligned_split(w.node_of, world)
    counts = np.bincount(w.node_of, minlength=w.M)
    ranks = LocalRanks(world, timeout=180.0)
    outs, errs = [None] * world, [None] * world

    def work(r):
        try:
            torch.cuda.set_device(0)
            lo, hi = int(cuts[r]), int(cuts[r + 1])
            e = engine(w, lo, hi, ranks.rank(r), counts)
            outs[r] = reports(e, w, lo, hi, case["steps"])
        except Exception:
            errs[r] = traceback.format_exc()
            ranks.abort()

    threads = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    bad = [f"rank {r}:\n{x}" for r, x in enumerate(errs) if x]
    if bad:
        print("\n".join(bad), flush=True)
        raise SystemExit(1)
    for r in range(world):
        np.savez(os.path.join(spec["outdir"], f"local_r{r}.npz"), **outs[r])


def main():
    spec = json.load(open(sys.argv[1]))
    if spec.get("local"):
        return main_local(spec)
    import numpy as np
    import torch
    import torch.distributed as dist
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
    np.savez(os.path.join(spec["outdir"], f"two_r{rank}.npz"), **reports(e, w, lo, hi, case["steps"]))
    del e
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
