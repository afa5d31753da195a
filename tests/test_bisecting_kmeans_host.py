"""BisectingKMeans' host logic (cycloneml_amd/bisecting_kmeans.py: the level
loop, the tree, the refusals) over the numpy step against the row-by-row
restatement of tests/bisecting_kmeans_restatement.py.  The numpy step adds a
cluster's rows in row order, as the restatement does, so trees agree by bytes
on any rows.  No device is used.
"""
import ctypes

import numpy as np
import pytest
import torch

import bisecting_kmeans_restatement as R
from cycloneml_amd import _native as N
from cycloneml_amd import bisecting_kmeans as bk
from cycloneml_amd.bisecting_kmeans import BisectingKMeans, BisectingKMeansModel, NumpyStep
from cycloneml_amd.linalg import CSRRows


def same_tree(a, b):
    """a: the package's root, b: the restatement's."""
    na, nb = list(R.walk(a)), list(R.walk(b))
    assert [n.index for n in na] == [n.index for n in nb]
    assert [n.size for n in na] == [n.size for n in nb]
    assert [len(n.children) for n in na] == [len(n.children) for n in nb]
    for x, y in zip(na, nb):
        assert x.center.tobytes() == np.ascontiguousarray(y.center).tobytes()
        assert x.cost == y.cost and x.height == y.height


def both(X, w=None, **kw):
    est = BisectingKMeans(k=kw.get("k", 4), maxIter=kw.get("maxIter", 20), seed=kw.get("seed", 0),
                          minDivisibleClusterSize=kw.get("minDiv", 1.0))
    model = est.fit_step(NumpyStep(X, w), X.shape[1])
    clusters, _ = R.fit(X, w, kw.get("k", 4), kw.get("maxIter", 20), kw.get("minDiv", 1.0),
                        kw.get("seed", 0))
    root = R.build_tree(clusters)
    same_tree(model.root, root)
    assert model.trainingCost == R.training_cost(root)
    assert model.summary.trainingCost == model.trainingCost
    assert model.summary.clusterSizes == [leaf.size for leaf in R.leaves(root)]
    assert model.summary.numIter == kw.get("maxIter", 20)
    assert model.clusterCenters.tobytes() == np.stack(
        [leaf.center for leaf in R.leaves(root)]).tobytes()
    return model, clusters


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("k", [2, 4, 7])
def test_driver_equals_restatement_exact_rows(k, weighted):
    X, w = R.exact_rows(300, 5, seed=k, weighted=weighted)
    model, _ = both(X, w, k=k, seed=11)
    assert model.k == k


def test_driver_equals_restatement_real_rows():
    X, _ = R.real_rows([40, 25, 60, 35], 3, seed=2)
    w = np.random.default_rng(3).uniform(0.5, 2.0, size=X.shape[0])
    model, _ = both(X, w, k=4, seed=5)
    assert sorted(model.summary.clusterSizes) == [25, 35, 40, 60]


def test_k_one():
    X, w = R.exact_rows(50, 4)
    model, clusters = both(X, w, k=1)
    assert sorted(clusters) == [1] and model.root.isLeaf and model.root.index == 0


def test_k_beyond_distinct_rows():
    rows = np.array([[0.0, 1.0], [8.0, 3.0], [2.0, 9.0]])
    X = np.ascontiguousarray(rows[np.arange(30) % 3])
    model, _ = both(X, None, k=8)
    # three distinct rows: three leaves.  A leaf's cost is the rounding of sumSq (about 1e-13
    # of 850), which can pass for divisible: such a cluster gets one child, itself
    assert model.k == 3
    assert all(leaf.cost < 1e-9 and leaf.size == 10 for leaf in model.root.leafNodes())


@pytest.mark.parametrize("minDiv", [0.3, 0.5, 50.0, 120.0])
def test_min_divisible_cluster_size(minDiv):
    X, _ = R.real_rows([100, 40, 30, 30], 2, seed=4)
    both(X, None, k=4, minDiv=minDiv, seed=1)


def test_min_divisible_cluster_size_stops_small_clusters():
    X, _ = R.real_rows([100, 40], 2, seed=4)
    model, _ = both(X, None, k=4, minDiv=0.8, seed=1)    # 112 rows needed: only the root
    assert sorted(model.summary.clusterSizes) == [40, 100]


def test_more_divisible_than_needed_ties_go_to_the_lower_index():
    # two mirror-image halves of 40 rows: after the root's split both children
    # are divisible with one size, and k = 3 needs one of them
    g = np.array([[0.0, 0.0], [0.0, 16.0], [1024.0, 0.0], [1024.0, 16.0]])
    X = np.ascontiguousarray(np.repeat(g, 20, axis=0)
                             + np.tile(np.arange(20.0)[:, None] % 4, (4, 2)))
    model, clusters = both(X, None, k=3, seed=7)
    left, right = model.root.children
    assert left.size == right.size == 40
    assert not left.isLeaf and right.isLeaf
    assert sorted(clusters) == [1, 2, 3, 4, 5]


def test_more_divisible_than_needed_largest_first():
    X, _ = R.real_rows([30, 30, 90, 90], 2, seed=9, spread=200.0)
    model, _ = both(X, None, k=3, seed=3)
    assert model.k == 3


def test_vanishing_child_and_one_child_nodes():
    # rows symmetric about the origin: the center's norm is 0, both children
    # are the center itself, every row ties and goes left, the right child
    # vanishes and the left one is offered alone
    X = np.array([[1.0, -1.0], [-1.0, 1.0], [2.0, -2.0], [-2.0, 2.0], [3.0, -3.0], [-3.0, 3.0]])
    model, clusters = both(X, None, k=4, maxIter=3)
    assert sorted(clusters) == [1, 2, 4, 8]
    node, depth = model.root, 0
    while not node.isLeaf:
        assert len(node.children) == 1 and node.height == 0.0
        node, depth = node.children[0], depth + 1
    assert depth == 3 and node.size == 6


def test_node_without_left_child_is_a_leaf():
    s = {i: R.Summary(2) for i in (1, 3)}
    for i, sm in s.items():
        sm.add(np.array([float(i), 1.0]), 1.0, 1.0)
        sm.add(np.array([float(i), 3.0]), 1.0, 1.0)
        sm.finish()
    mine = bk.build_tree({i: bk.ClusterSummary(v.size, v.center, v.norm, v.cost)
                          for i, v in s.items()})
    same_tree(mine, R.build_tree(s))
    assert mine.isLeaf and mine.index == 0
    # with the left child present the right one is listed after it
    s[2] = s[3]
    mine = bk.build_tree({i: bk.ClusterSummary(v.size, v.center, v.norm, v.cost)
                          for i, v in s.items()})
    same_tree(mine, R.build_tree(s))
    assert [c.index for c in mine.children] == [0, 1] and mine.index == -1


def test_max_iter_zero():
    X, w = R.exact_rows(60, 3)
    model, clusters = both(X, w, k=4, maxIter=0)
    assert sorted(clusters) == [1] and model.k == 1


def test_zero_cost_cluster_is_not_divisible():
    X = np.tile(np.array([[3.0, 4.0, 12.0]]), (25, 1))
    model, clusters = both(X, None, k=4)
    assert sorted(clusters) == [1] and model.root.cost == 0.0 and model.root.size == 25


def test_model_from_arrays_needs_no_device():
    centers = np.array([[0.0, 0.0], [-4.0, 0.0], [4.0, 3.0], [4.0, 0.0], [4.0, 6.0]])
    m = BisectingKMeansModel.from_arrays(centers, [1, -1, 3, -1, -1], [2, 0, 2, 0, 0])
    assert m.k == 3 and m.clusterCenters.tobytes() == centers[[1, 3, 4]].tobytes()
    assert [n.index for n in R.walk(m.root)] == [-1, 0, -2, 1, 2]
    assert m.root.height == 5.0 and m.root.children[1].height == 3.0
    with pytest.raises(N.IllegalArgumentException):
        BisectingKMeansModel.from_arrays(centers, [0, -1, 3, -1, -1], [2, 0, 2, 0, 0])


def test_default_seed():
    h = 0
    for ch in "org.apache.spark.ml.clustering.BisectingKMeans":
        h = (31 * h + ord(ch)) & 0xFFFFFFFF
    assert BisectingKMeans().seed == (h - (1 << 32) if h >= 1 << 31 else h)
    e = BisectingKMeans()
    assert (e.k, e.maxIter, e.minDivisibleClusterSize, e.distanceMeasure) == (4, 20, 1.0,
                                                                              "euclidean")


@pytest.mark.parametrize("kw", [dict(k=0), dict(k=-3), dict(maxIter=-1),
                                dict(minDivisibleClusterSize=0.0),
                                dict(minDivisibleClusterSize=-1.0),
                                dict(minDivisibleClusterSize=float("nan")),
                                dict(distanceMeasure="cosine"),
                                dict(distanceMeasure="manhattan")])
def test_parameter_refusals(kw):
    with pytest.raises(N.IllegalArgumentException):
        BisectingKMeans(**kw)


def test_csr_rows_are_refused():
    rp = torch.tensor([0, 1, 2], dtype=torch.int64)
    X = CSRRows(rp, torch.tensor([0, 1], dtype=torch.int32),
                torch.tensor([1.0, 2.0], dtype=torch.float64), 2)
    with pytest.raises(N.IllegalArgumentException, match="CSR"):
        BisectingKMeans().fit(X)


@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan])
def test_bad_row_is_named_by_its_lowest_index(bad):
    X, w = R.exact_rows(40, 3)
    X[31, 1] = bad
    X[17, 2] = bad
    with pytest.raises(N.IllegalArgumentException, match=r"\(row 17\)"):
        BisectingKMeans(k=2).fit_step(NumpyStep(X, w), 3)


@pytest.mark.parametrize("bad", [0.0, -0.125, np.inf, np.nan])
def test_bad_weight_is_named_by_its_lowest_index(bad):
    X, w = R.exact_rows(40, 3)
    w[29] = bad
    w[8] = bad
    with pytest.raises(N.IllegalArgumentException, match=r"weight.*\(row 8\)"):
        BisectingKMeans(k=2).fit_step(NumpyStep(X, w), 3)


NAMES = ["cyc_bkm_plan_create", "cyc_bkm_plan_destroy", "cyc_bkm_tile_rows",
         "cyc_bkm_panel_cols", "cyc_bkm_chunk_rows", "cyc_bkm_chunks_per_launch",
         "cyc_bkm_max_children", "cyc_bkm_step_dev", "cyc_bkm_predict_dev"]


def test_header_symbols():
    syms = set(N.header_symbols())
    lib = N.load()
    for name in NAMES:
        assert name in syms and name in N.SIGNATURES and hasattr(lib, name)
    assert sorted(s for s in syms if s.startswith("cyc_bkm_")) == sorted(NAMES)
    assert sorted(s for s in N.SIGNATURES if s.startswith("cyc_bkm_")) == sorted(NAMES)


def test_plan_arguments_are_checked_before_the_device():
    lib = N.load()
    h = ctypes.c_void_p()
    assert lib.cyc_bkm_plan_create(0, 0, ctypes.byref(h)) == N.CYC_ERR_INVALID_ARG
    assert lib.cyc_bkm_plan_create(4, -1, ctypes.byref(h)) == N.CYC_ERR_INVALID_ARG
    assert lib.cyc_bkm_plan_create(4, 0, None) == N.CYC_ERR_INVALID_ARG
    assert lib.cyc_bkm_tile_rows(None) == -1 and lib.cyc_bkm_chunks_per_launch(None) == -1
