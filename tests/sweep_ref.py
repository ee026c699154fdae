"""float64 restatement of ONE iteration of the residences' recurrence while the operator's multipliers are zero
(lpsolver.py:254-287 with slack voltage rows), out of the oracle's own functions -- what one inner iteration of
revs_agent_step_multi computes from the state in front of it:

    pen  = max(utility_g0(P_est, P_sch, G, kappa), 0)       the operator's answer P_est[k+1] (lpsolver.py:196-207, g >= 0)
    p, g = Home(cost, P_est, P_sch, G).solve()               from the OLD estimate P_est[k] (lpsolver.py:273)
    G'   = G + (kappa/2)(pen - g)                            lpsolver.py:282-283
    diff = |pen - g|_2 / T                                   lpsolver.py:284

and the estimate the NEXT iteration's operator would give on the state just produced, pen2 = max(g0(pen, g, G'), 0),
whose node sums the sweep leaves for the voltage verdict."""
from dataclasses import dataclass

import numpy as np

from oracle import revs_oracle as ro


@dataclass
class Link:
    pen: np.ndarray       # (N,T) P_est[k+1]
    p: np.ndarray         # (N,T) charger schedule S
    soc: np.ndarray       # (N,T+1)
    g: np.ndarray         # (N,T) P_sch[k+1]
    G: np.ndarray         # (N,T) G[k+1]
    diff: np.ndarray      # (N,)
    dsq: np.ndarray       # (N,) sum_t (P_sch[k+1] - P_sch[k])^2
    status: np.ndarray    # (N,) 0 ok, 1 "No solution found"
    pen2: np.ndarray      # (N,T) P_est[k+2]


def link(cost, oh, pe, ps, G, kappa, mode):
    """One iteration from the state (pe, ps, G) = (P_est[k], P_sch[k], G[k]).  mode: "binary" or "relaxed"."""
    pe, ps, G = (np.asarray(a, np.float64) for a in (pe, ps, G))
    T = pe.shape[1]
    pen = np.maximum(ro.utility_g0(pe, ps, G, kappa), 0.0)
    solve = ro.home_solve_binary if mode == "binary" else ro.home_solve_relaxed
    p, soc, g, st = solve(cost, oh, pe, ps, G, kappa)
    chk = pen - g
    Gn = G + 0.5 * kappa * chk
    pen2 = np.maximum(ro.utility_g0(pen, g, Gn, kappa), 0.0)
    return Link(pen, p, soc, g, Gn, np.linalg.norm(chk, axis=1) / T, ((g - ps) ** 2).sum(axis=1), st, pen2)


def run(cost, oh, kappa, iters, mode, state=None):
    """`iters` links from `state` = (P_est, P_sch, G) (default zero, lpsolver.py:244-246) -> list of Link."""
    N, T = oh.LOAD.shape
    pe, ps, G = state if state is not None else (np.zeros((N, T)),) * 3
    out = []
    for _ in range(iters):
        lk = link(cost, oh, pe, ps, G, kappa, mode)
        out.append(lk)
        pe, ps, G = lk.pen, lk.g, lk.G
    return out


def node_sums(node_of, M, x):
    """float64 np.add.at of a residence profile over the nodes -> (M, T)."""
    s = np.zeros((M, x.shape[1]))
    np.add.at(s, np.asarray(node_of, np.int64), np.asarray(x, np.float64))
    return s
