"""The two power-flow functions of the reference's drawing.py (lines 29-78) over the GPU network report:

    from revs_admm_amd.drawing import compute_flows, compute_voltage, compute_losses

Same arguments and the same dicts back -- {edge: loading per slot} over graph.edges, {node: voltage per slot} over
the non-substation nodes -- so the code that feeds the reference's box plots runs unchanged.  compute_losses is the
third of the kind, over the loss report: {edge: kW lost per slot}.  The figures
themselves (matplotlib, seaborn, geopandas) are outside the project.

Line ratings are the caller's data: an edge attribute `rating` (kVA) on the graph, or `rating=` as a mapping from
the edges' `type` attribute to kVA (the reference keeps such a table inside compute_flows; INTEGRATION.md shows how
to pass one)."""
from __future__ import annotations

import numpy as np

from .lpsolver import feeder_arrays
from .network import report_for_tree

__all__ = ["compute_flows", "compute_voltage", "compute_losses"]


def _edge_ratings(graph, rating):
    """kVA of every edge, in graph.edges order."""
    edges = list(graph.edges)
    if rating is not None:
        missing = sorted({graph.edges[e].get("type") for e in edges} - set(rating), key=str)
        if missing:
            raise KeyError(f"compute_flows: rating= has no entry for line type {missing[0]!r}")
        return np.array([float(rating[graph.edges[e]["type"]]) for e in edges])
    if edges and all("rating" in graph.edges[e] for e in edges):
        return np.array([float(graph.edges[e]["rating"]) for e in edges])
    raise ValueError("compute_flows needs line ratings: give every edge a `rating` attribute (kVA), or pass "
                     "rating={line type: kVA} for the edges' `type` attribute")


def _node_profile(graph, p_sch):
    res = [n for n in graph if graph.nodes[n]["label"] == "H"]
    nonsub = [n for n in graph if graph.nodes[n]["label"] != "S"]
    return res, nonsub, np.array([p_sch[h] for h in res], np.float64)


def line_nodes(graph, rating, parent, nonsub):
    """-> (rating per tree node: that of the line to its parent; the tree node below each edge of graph.edges; the
    edge's sign towards it)."""
    rate = _edge_ratings(graph, rating)
    pos = {n: i for i, n in enumerate(nonsub)}
    child = np.empty(len(rate), np.int64)
    sign = np.empty(len(rate))
    for k, (u, v) in enumerate(graph.edges):
        down = pos.get(v, -1) >= 0 and parent[pos[v]] == pos.get(u, -1)
        child[k], sign[k] = (pos[v], 1.0) if down else (pos[u], -1.0)
    node_rating = np.zeros(len(nonsub))
    node_rating[child] = rate
    return node_rating, child, sign


def compute_flows(graph, p_sch, rating=None, device="cuda:0"):
    """drawing.py:29-58: {edge: [flow / rating per slot]} in graph.edges order, signed like the reference's
    A^-1 P (positive from the edge's first node to its second; the box plots take the absolute value)."""
    res, nonsub, P = _node_profile(graph, p_sch)
    parent, edge_r, cons_of = feeder_arrays(graph, res)
    node_rating, child, sign = line_nodes(graph, rating, parent, nonsub)
    rep = report_for_tree(parent, edge_r, cons_of, P, rating=node_rating, device=device)
    signed = sign[:, None] * np.sign(rep.flow[child]) * rep.loading[child]
    return {e: signed[k].tolist() for k, e in enumerate(graph.edges)}


def compute_voltage(graph, p_sch, vset=1.0, device="cuda:0"):
    """drawing.py:60-78: {node: [sqrt(vset^2 - (R P)[node]) per slot]} over the non-substation nodes."""
    res, nonsub, P = _node_profile(graph, p_sch)
    parent, edge_r, cons_of = feeder_arrays(graph, res)
    rep = report_for_tree(parent, edge_r, cons_of, P, vset=vset, device=device)
    return {n: rep.volt[i].tolist() for i, n in enumerate(nonsub)}


def compute_losses(graph, p_sch, vset=1.0, device="cuda:0"):
    """Next to compute_flows / compute_voltage: {edge: [kW lost on the line per slot]} in graph.edges order, the
    loss report's r P^2 / v at the line's receiving end (losses.report_for_tree)."""
    from .losses import report_for_tree as loss_report
    res, nonsub, P = _node_profile(graph, p_sch)
    parent, edge_r, cons_of = feeder_arrays(graph, res)
    pos = {n: i for i, n in enumerate(nonsub)}
    rep = loss_report(parent, edge_r, cons_of, P, vset=vset, device=device)
    out = {}
    for u, v in graph.edges:                      # (the tree node below the edge, as line_nodes finds it)
        down = pos.get(v, -1) >= 0 and parent[pos[v]] == pos.get(u, -1)
        out[(u, v)] = rep.loss[pos[v] if down else pos[u]].tolist()
    return out
