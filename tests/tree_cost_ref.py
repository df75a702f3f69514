"""NumPy float64 statement of srtGetTreeCost (include/srt_hip.h): the surface-area cost of one world item's tree, defined so
that every bit is reproducible.  No GPU and no library.  `nodes` is what Context.bvh(item) returns (tree_build_ref.NODE_DTYPE:
float32 boxes; node 0 is the root).

  a_i  = (dx dy + dy dz) + dz dx, with dx = (double)max.x - (double)min.x and dy, dz likewise: separate multiplies and adds
  S    = the pairwise sum of a_0 .. a_(n-1), padded with +0.0 to the next power of two: every level is x[0::2] + x[1::2]
  cost = S / a_0
"""
import numpy as np


def node_terms(nodes):
    """a_i of every node, float64."""
    d = nodes["bmax"].astype(np.float64) - nodes["bmin"].astype(np.float64)
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    xy = dx * dy
    yz = dy * dz
    zx = dz * dx
    return (xy + yz) + zx


def pairwise_sum(a):
    """The pairwise sum of a float64 vector padded with +0.0 to the next power of two."""
    a = np.asarray(a, np.float64)
    width = 1
    while width < len(a):
        width *= 2
    x = np.zeros(width, np.float64)
    x[:len(a)] = a
    while len(x) > 1:
        x = x[0::2] + x[1::2]
    return x[0]


def tree_cost(nodes):
    """The value srtGetTreeCost returns for this tree, as a numpy.float64 (compare its bits: .view(np.uint64))."""
    a = node_terms(nodes)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.float64(pairwise_sum(a)) / np.float64(a[0])


def bits(x):
    return int(np.array([x], np.float64).view(np.uint64)[0])
