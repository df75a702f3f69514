"""tests/tree_cost_ref.py (the NumPy statement of srtGetTreeCost) held to other statements of the same value: the tests'
long-standing tree_build_ref.sah_cost, a tree worked by hand, one node, and an explicit Python loop over a count that is no
power of two.  No GPU and no library."""
import numpy as np

import tree_build_ref as R
import tree_build_scenes as S
import tree_cost_ref as C


def _tree(boxes):
    nodes = np.zeros(len(boxes), R.NODE_DTYPE)
    for i, (mn, mx) in enumerate(boxes):
        nodes["bmin"][i], nodes["bmax"][i] = mn, mx
    return nodes


def test_agrees_with_sah_cost(abi):
    """Two summation orders of at most a few thousand non-negative doubles: each is within n * 2^-53 relative of the exact
    sum, far inside 1e-12."""
    for n in (2, 3, 37, 257, 3000):
        sb = S.soup(abi, n, 0)
        refs = np.arange(n)
        for nodes in (R.build_lbvh(sb, refs, 0.0, 1.0)[0], R.build_ploc(sb, refs, 0.0, 1.0, 16)[0]):
            got, want = float(C.tree_cost(nodes)), R.sah_cost(nodes)
            assert want >= 1.0 and abs(got - want) <= 1e-12 * want, (n, got, want)


def test_hand_worked_three_nodes():
    """Root 2 x 3 x 4: a = (6 + 12) + 8 = 26.  Children 1 x 1 x 1 (a = 3) and 2 x 1 x 0.5 (a = (2 + 0.5) + 1 = 3.5).  Padded
    to four: (26 + 3) + (3.5 + 0) = 32.5, over 26 = 1.25: every value is a dyadic rational, nothing rounds."""
    nodes = _tree([((0, 0, 0), (2, 3, 4)), ((0, 0, 0), (1, 1, 1)), ((0, 2, 3.5), (2, 3, 4))])
    assert C.node_terms(nodes).tolist() == [26.0, 3.0, 3.5]
    assert C.pairwise_sum(C.node_terms(nodes)) == 32.5
    assert C.tree_cost(nodes) == 1.25 and C.bits(C.tree_cost(nodes)) == 0x3FF4000000000000


def test_one_node_costs_one():
    nodes = _tree([((-1.5, 0.25, 3), (0.7, 0.9, 3.3))])
    assert C.bits(C.tree_cost(nodes)) == C.bits(1.0)
    # a root without area gives what the division gives
    assert np.isnan(C.tree_cost(_tree([((1, 1, 1), (1, 1, 1))])))
    assert np.isinf(C.tree_cost(_tree([((0, 0, 0), (1, 0, 0)), ((0, 0, 0), (1, 1, 1))])))


def test_non_power_of_two_count_against_a_loop():
    """11 nodes with widths that make every addition round: the levels written as a loop over Python floats (IEEE doubles),
    multiplies and adds one at a time."""
    rng = np.random.default_rng(5)
    mn = rng.normal(size=(11, 3)).astype(np.float32)
    mx = mn + rng.random((11, 3), dtype=np.float32) * np.float32(3)
    nodes = _tree(list(zip(mn, mx)))
    terms = []
    for i in range(11):
        dx, dy, dz = (float(mx[i, k]) - float(mn[i, k]) for k in range(3))
        xy, yz, zx = dx * dy, dy * dz, dz * dx
        terms.append((xy + yz) + zx)
    x = terms + [0.0] * 5
    while len(x) > 1:
        x = [x[2 * k] + x[2 * k + 1] for k in range(len(x) // 2)]
    want = x[0] / terms[0]
    assert C.bits(C.tree_cost(nodes)) == C.bits(want)
    # padding further changes nothing: the cost of the padded sum is the cost
    assert C.bits(C.pairwise_sum(terms + [0.0] * 21)) == C.bits(C.pairwise_sum(terms))
