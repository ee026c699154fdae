"""What the reports over the feeder as a tree stage alike around their one call into the library (study.py, headroom.py,
losses.py, attribution.py, risk.py, prices.py, powerflow.py; transformers.py, which has no tree, uses the checks of the node sums, the device context and the
buffers): the checks of the node sums and of the feeder, the tree and the stream of the launch, a host caller's upload,
the out= tensor, the scratch, the records' buffers and their read-back, and the per-position masks and classes.  Plain
functions; `who` is the report's name in front of every message ("headroom report")."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .bills import check_scenarios
from .network import tree_on_device


def check_node_sums(who, node_g, dims=(2, 3), forms=None, bound=True):
    """node_g: a contiguous float64 tensor (S, M, T), or (M, T) where dims allows it -> (single: it was (M, T), node_g
    as (S, M, T)).  forms = (feeder, tree): the feeder must come in exactly one of its two forms.  bound=False: the
    caller checks the number of scenarios itself, behind checks of its own (the study report)."""
    if not isinstance(node_g, torch.Tensor) or node_g.dtype != torch.float64 or node_g.dim() not in dims \
            or not node_g.is_contiguous():
        raise ValueError(f"{who}: node_g must be a contiguous (scenarios, rows, slots) float64 tensor")
    if forms is not None and (forms[0] is None) == (forms[1] is None):
        raise ValueError(f"{who}: pass the feeder either as feeder=(parent, edge_r, cons_of) or as tree=")
    single = node_g.dim() == 2
    g3 = node_g[None] if single else node_g
    if bound:
        check_scenarios(who, g3.shape[0])
    return single, g3


def on_device(dev, stream, run):
    """run(the HIP stream of the launch: `stream`, by default torch's current one) with dev the current device."""
    def go():
        st = stream
        if st is None and dev.type == "cuda":
            st = torch.cuda.current_stream(dev).cuda_stream
        return run(st)

    if dev.type != "cuda":          # (a host stand-in of the kernels: no device to make current)
        return go()
    with torch.cuda.device(dev):
        return go()


def run_on_device(g3, feeder, tree, native, lib=None, stream=None):
    """native(lib, dev, stream, _lib.Tree, the dict of feeder_tree, nodes before padding, g3) on g3's device.  The feeder
    comes as feeder=(parent, edge_r, cons_of) -- its tree is built and uploaded here, every row kept -- or as
    tree=(_lib.Tree, the dict of feeder_tree, nodes before padding) where it already lies on that device."""
    dev = g3.device

    def run(st):
        if tree is None:
            th, tr, _keep = tree_on_device(dev, *feeder, g3.shape[1])
            n_nodes = len(feeder[0])
        else:
            tr, th, n_nodes = tree
        return native(lib or _lib.load(), dev, st, tr, th, n_nodes, g3)

    return on_device(dev, stream, run)


def device_report(who, node_g, feeder, tree, native, lib=None, stream=None):
    """The shell of a report over node sums that lie on the device: the checks, then run_on_device -> the list of S
    reports that native returns, or the one of an (M, T) node_g."""
    single, g3 = check_node_sums(who, node_g, forms=(feeder, tree))
    reps = run_on_device(g3, feeder, tree, native, lib, stream)
    return reps[0] if single else reps


def host_report(device, arrays, report):
    """The shell of a report over node injections held on the host: report(every array of `arrays` as a float64 tensor on
    the device, None for None) with that device current."""
    from .engine import _dev_check
    _lib.load()
    dev = _dev_check(device)
    with torch.cuda.device(dev):
        return report(*[None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(dev)
                        for a in arrays])


def check_out(who, out, shape, dev):
    """out=: None, or a contiguous float64 tensor of `shape` on dev that receives the report's first array."""
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.float64 or tuple(out.shape) != shape
                            or not out.is_contiguous() or out.device != dev):
        raise ValueError(f"{who}: out must be a contiguous float64 {shape} tensor on {dev}")


def scratch(who, nbytes, sizes, dev, what="scratch"):
    """The scratch of nbytes that the library's *_scratch function asks for (0: it refuses the sizes)."""
    if nbytes <= 0:
        raise ValueError(f"{who}: no {what} size for {sizes}")
    return torch.empty((int(nbytes) + 7) // 8, dtype=torch.float64, device=dev)


def record_buffer(dev, dtype, count):
    """`count` zeroed records of `dtype` on the device, as bytes."""
    return torch.zeros(count * dtype.itemsize, dtype=torch.uint8, device=dev)


def records(d, dtype, *shape):
    """A record_buffer read back as `shape` records."""
    return d.cpu().numpy().view(dtype).reshape(*shape)


def _by_position(tree_host, n_nodes):
    """(whether a preorder position holds one of the caller's n_nodes tree nodes, that node or 0)."""
    order = np.asarray(tree_host["order"], np.int64)
    real = order < n_nodes
    return real, np.where(real, order, 0)


def position_mask(dev, tree_host, n_nodes, nodes, none="rows", who=None):
    """uint8 per preorder position: whether the tree node there is one of `nodes` (indices or a boolean mask).  none: what
    nodes=None stands for -- "rows": the nodes that carry a row of the injections; "no array": None is returned (the library
    then takes every position).  who = (report, name): a boolean mask must have one entry per tree node."""
    real, src = _by_position(tree_host, n_nodes)
    if nodes is None:
        if none == "no array":
            return None
        mk = real & (np.asarray(tree_host["src"]) >= 0)
    else:
        sel, idx = np.zeros(n_nodes, bool), np.asarray(nodes)
        if who is not None and idx.dtype == bool and idx.shape != (n_nodes,):
            raise ValueError(f"{who[0]}: a boolean {who[1]} mask must have one entry per tree node ({n_nodes})")
        sel[idx if idx.dtype == bool else idx.astype(np.int64)] = True
        mk = real & sel[src]
    return torch.from_numpy(np.ascontiguousarray(mk.astype(np.uint8))).to(dev)


def position_classes(dev, tree_host, n_nodes, cl, max_classes):
    """cl: one class per tree node, an array (n_nodes,) that the caller has checked -> (uint8 per preorder position, 255
    at padding positions and where the node is in no class: an entry outside 0 .. max_classes - 1; C = the largest class
    + 1).  What a report refuses -- a wrong length, for the loss report a class of max_classes or more -- it refuses
    itself, in its own words, before it calls this."""
    cl = np.where((cl >= 0) & (cl < max_classes), cl, 255).astype(np.uint8)
    real, src = _by_position(tree_host, n_nodes)
    used = cl[cl < 255]
    return (torch.from_numpy(np.ascontiguousarray(np.where(real, cl[src], 255).astype(np.uint8))).to(dev),
            int(used.max()) + 1 if used.size else 0)
