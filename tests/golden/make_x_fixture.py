#!/usr/bin/env python3
"""Generate tests/golden/revs_121144_x.npz: the reactance of every line of the 121144 feeder.

Run once, where the reference tree is present (REVS_REFERENCE, as for make_fixtures.py):

    python tests/golden/make_x_fixture.py

Only the edges' `x` attribute is read from the reference's data file `input/121144-dist-net.gpickle`, in the edge order of
revs_121144.npz (which this script asserts).  What ends up in the fixture: one double per edge -- numbers only."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_fixtures import REF, _Unpickler  # noqa: E402


def main():
    g = _Unpickler(open(f"{REF}/input/121144-dist-net.gpickle", "rb")).load()
    nodes, edges = list(g.nodes()), list(g.edges())
    nidx = {n: i for i, n in enumerate(nodes)}
    base = np.load(os.path.join(HERE, "revs_121144.npz"))
    assert np.array_equal(base["edge_u"], [nidx[u] for u, v in edges])
    assert np.array_equal(base["edge_v"], [nidx[v] for u, v in edges])
    x = np.array([g.edges[e]["x"] for e in edges], np.float64)
    assert x.shape == base["edge_u"].shape and np.isfinite(x).all()
    out = os.path.join(HERE, "revs_121144_x.npz")
    np.savez_compressed(out, edge_x=x)
    print(f"wrote {out}: {os.path.getsize(out)} bytes; {x.size} edges, x in [{x.min():.3g}, {x.max():.3g}]")


if __name__ == "__main__":
    main()
