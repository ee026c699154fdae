#!/usr/bin/env python3
"""Generate tests/golden/revs_121144_lines.npz: the conductor type and the rating of every line of the 121144 feeder.

Run once, where the reference tree is present (REVS_REFERENCE, as for make_fixtures.py):

    python tests/golden/make_line_fixture.py

The edges' `type` attribute comes from the reference's data file `input/121144-dist-net.gpickle`, in the edge order of
revs_121144.npz (which this script asserts).  A line's rating is sqrt(3) x ampacity [A] x line voltage [kV] in kVA; the
ampacity and the voltage level of each conductor are read as NUMBERS out of the text of the reference's drawing.py
(compute_flows' table): the file is scanned with a regular expression, never imported or run, and none of its text is
kept.  What ends up in the fixture: per edge the type string and the rating, and per type that occurs the name, the
ampacity, the kV level, the rating and the number of edges -- names and numbers only."""
import os
import re
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
    table = {}
    for name, amp, kv in re.findall(r"'(\w+)'\s*:\s*np\.sqrt\(3\)\s*\*\s*([\d.]+)\s*\*\s*([\d.]+)",
                                    open(f"{REF}/drawing.py").read()):
        table[name] = (float(amp), float(kv))
    types = [g.edges[e]["type"] for e in edges]
    names = sorted(set(types), key=lambda s: (-types.count(s), s))
    amp = np.array([table[s][0] for s in names])
    kv = np.array([table[s][1] for s in names])
    rate = np.sqrt(3.0) * amp * kv
    by = dict(zip(names, rate))
    out = os.path.join(HERE, "revs_121144_lines.npz")
    np.savez_compressed(out, edge_type=np.array(types, dtype="S16"), edge_rating=np.array([by[s] for s in types]),
                        type_name=np.array(names, dtype="S16"), type_ampacity=amp, type_kv=kv, type_rating=rate,
                        type_count=np.array([types.count(s) for s in names], np.int64))
    print(f"wrote {out}: {os.path.getsize(out)} bytes;", ", ".join(f"{s} {types.count(s)}" for s in names))


if __name__ == "__main__":
    main()
