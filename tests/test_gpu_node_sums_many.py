"""revs_net_node_sums_many (csrc/network_kernels.hip) through the C ABI: the node sums of an ensemble's S scenarios
from its own layout float[n][S][T] into revs_net_study's double[S][m][T], bit for bit (a) revs_net_node_sums on
contiguous copies of each scenario's rows, (b) -- up to 192 columns -- revs_net_node_sums over the (n, S T) view,
transposed, and (c) a numpy float64 loop with one accumulator in ascending residence order (there is no multiply
anywhere: equality is exact).  Guard scenarios before and after the output stay NaN; a second call gives the same
bytes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# empty nodes, every remainder of the unroll by four, an empty node between full ones
COUNTS_SMALL = [0, 1, 2, 3, 4, 5, 9, 0, 13, 1]
SHAPES = [(1, 1),        # smallest extents
          (1, 24),       # one scenario
          (3, 7),        # ragged
          (8, 24),       # 192 columns, the last width the single entry takes over the view
          (10, 96),      # 960 columns
          (42, 24),      # 1008 columns
          (5, 192)]      # widest T


def _counts(which):
    if which == "small":
        return np.array(COUNTS_SMALL, np.int64)
    return np.random.default_rng(300).integers(0, 8, 300).astype(np.int64)


def _values(rng, shape):
    a = rng.normal(0.0, 3.0, shape).astype(np.float32)      # negatives included
    a[rng.random(shape) < 0.02] = 0.0                       # a few exact zeros
    return a


def _numpy_sums(node_ptr, load, p):
    """One float64 accumulator per output from +0.0, residences ascending, the widened pair added first."""
    n, S, T = p.shape
    m = len(node_ptr) - 1
    out = np.zeros((S, m, T))
    for node in range(m):
        acc = np.zeros((S, T))
        for i in range(node_ptr[node], node_ptr[node + 1]):
            acc = acc + ((load[i].astype(np.float64) + p[i].astype(np.float64)) if load is not None
                         else p[i].astype(np.float64))
        out[:, node, :] = acc
    return out


@pytest.mark.parametrize("with_load", [True, False], ids=["load", "no_load"])
@pytest.mark.parametrize("S,T", SHAPES)
@pytest.mark.parametrize("which", ["small", "random300"])
def test_node_sums_many_bit_for_bit(gpu_lib, which, S, T, with_load):
    import torch
    from revs_admm_amd._lib import check, ptr
    counts = _counts(which)
    m, n = len(counts), int(counts.sum())
    node_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    rng = np.random.default_rng(1000 * S + T)
    p = _values(rng, (n, S, T))
    load = _values(rng, (n, S, T)) if with_load else None
    dev = "cuda:0"
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_ptr, d_p, d_load = up(node_ptr), up(p), (up(load) if with_load else None)

    def many():
        buf = torch.full((S + 2, m, T), float("nan"), dtype=torch.float64, device=dev)      # one guard scenario each side
        check(gpu_lib.revs_net_node_sums_many(S, m, T, ptr(d_ptr), ptr(d_load), ptr(d_p), buf[1:].data_ptr(), None),
              "revs_net_node_sums_many")
        torch.cuda.synchronize()
        return buf.cpu().numpy()

    def single(cols, l, q):
        out = torch.full((m, cols), float("nan"), dtype=torch.float64, device=dev)
        dl, dq = (None if l is None else up(l)), up(q)
        check(gpu_lib.revs_net_node_sums(m, cols, ptr(d_ptr), ptr(dl), ptr(dq), ptr(out), None), "revs_net_node_sums")
        torch.cuda.synchronize()
        return out.cpu().numpy()

    buf = many()
    got = buf[1:S + 1]
    # d. the guards are untouched, and a second call gives the same bytes
    assert np.isnan(buf[0]).all() and np.isnan(buf[S + 1]).all()
    assert not np.isnan(got).any()
    assert many().tobytes() == buf.tobytes()
    # a. every scenario's slice: the single entry on contiguous copies of that scenario's rows
    for s in range(S):
        ref = single(T, None if load is None else load[:, s, :], p[:, s, :])
        assert got[s].tobytes() == ref.tobytes(), s
    # b. up to 192 columns: the single entry over the (n, S T) view, transposed
    if S * T <= 192:
        view = single(S * T, None if load is None else load.reshape(n, S * T), p.reshape(n, S * T))
        assert got.tobytes() == np.ascontiguousarray(view.reshape(m, S, T).transpose(1, 0, 2)).tobytes()
    # c. numpy, one accumulator
    ref = _numpy_sums(node_ptr, load, p)
    assert got.tobytes() == ref.tobytes()
    assert (got[:, counts == 0] == 0.0).all() and not np.signbit(got[:, counts == 0]).any()
