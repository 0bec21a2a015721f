"""Graphs with loop closures as ADDITIONAL edges (E != N - 1), shared by tests/test_added_edges_cpu.py and
tests/test_added_edges_gpu.py: chain_problem(F) with the chain edges in ``drop`` taken out and the ``extra`` edges appended, each
measured from the ground truth with se3_exp(N(0, 0.01)) noise (one draw of six per extra edge, in order, seed 5)."""
import functools

import numpy as np

from oracle import lie
from tests.helpers import chain_problem

UNIT = (1, 1, 1, 1)
LW = (1, 0.1, 10, 0.1)

# name -> (F, extra edges, dropped chain edges)
CASES = {
    'more17': (17, ((0, 9), (4, 15), (16, 2), (3, 4), (0, 9)), ()),      # E = 21: a parallel pair, an adjacent duplicate, a reversed edge
    'fewer17': (17, ((0, 9),), (5, 6, 12)),                              # E = 14: frames without a VO edge
    'n2e3': (2, ((1, 0), (0, 1)), ()),                                   # three parallel edges, one reversed, on the only node pair
    'n3e1': (3, ((0, 2),), (0, 1)),                                      # node 1 has an empty CSR row
    'n3e4': (3, ((2, 0), (0, 2)), ()),
}


def closure_graph(F, extra, drop=(), seed=5):
    prob, tr = chain_problem(F)
    keep = np.array([e for e in range(F - 1) if e not in set(drop)], dtype=np.int64)
    links = np.asarray(prob['links'], dtype=np.int64)[keep]
    vo = np.asarray(prob['vo_motions'], dtype=np.float64)[keep]
    gt = np.concatenate([tr['gt_pos'], tr['gt_quat']], 1)
    rng = np.random.default_rng(seed)
    for (i, j) in extra:
        rel = lie.se3_mul(lie.se3_mul(lie.se3_inv(gt[i]), gt[j]), lie.se3_exp(rng.normal(0, 0.01, 6)))
        links = np.concatenate([links, [[i, j]]])
        vo = np.concatenate([vo, rel[None]])
    return dict(prob, links=links.astype(np.int64), vo_motions=vo)


@functools.lru_cache(maxsize=None)
def case(name):
    """The problem of CASES[name], built once and left unchanged by its users."""
    F, extra, drop = CASES[name]
    return closure_graph(F, extra, drop)


def sizes(name):
    """(N, E, M) of a case."""
    F, extra, drop = CASES[name]
    return F, F - 1 - len(drop) + len(extra), F - 1
