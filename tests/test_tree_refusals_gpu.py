"""What the tree walks refuse (csrc/decision_tree.hip's check_tree, used by
cyc_dt_predict_dev, cyc_rf_predict_dev, cyc_gbt_update_dev and
cyc_gbt_predict_dev): a kernel only walks a tree whose children follow their
parent and lie inside it and whose splits name a feature of the rows (a bin of
the image), and only reads a leaf index below the number of leaves.  d = 3, 4
rows, a root and two leaves, alone or as tree 1 of two; every refusal returns
before a launch, and the same tree without the fault is walked.
"""
import numpy as np
import pytest
import torch

from cycloneml_amd import _native as N
from cycloneml_amd.forest import RFPlan
from cycloneml_amd.gbt import FlatTree, GBTPlan
from cycloneml_amd.tree import DTPlan

pytestmark = pytest.mark.gpu

D, ROWS = 3, 4
# (the array, its new root / last-leaf entry, the message); "leaf" faults the last leaf
FAULTS = [("first", 0, "must follow it"), ("first", 2, "must follow it"),
          ("feature", 3, "must split a feature"), ("feature", -1, "must split a feature"),
          ("leaf", 2, "leaf index"), ("bin", 255, "split at a bin")]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def small_tree(fault=None, value=None):
    t = dict(feature=np.array([1, -1, -1], dtype=np.int32), threshold=np.array([0.5, 0.0, 0.0]),
             first=np.array([1, -1, -1], dtype=np.int32), leaf=np.array([-1, 0, 1], dtype=np.int32),
             bin=np.array([7, -1, -1], dtype=np.int32), value=np.array([0.0, 1.0, 2.0]))
    if fault is not None:
        t[fault][2 if fault == "leaf" else 0] = value
    return t


def flat_of(t, image):
    flat = FlatTree(t["feature"], t["threshold"], t["first"], t["leaf"], t["value"])
    flat.splitBin = t["bin"] if image else None
    return flat


def test_a_tree_no_kernel_may_walk_is_refused(cuda):
    rng = np.random.default_rng(0)
    X = dev(rng.normal(size=(ROWS, D)))
    image = dev(rng.integers(0, 16, size=(ROWS, D)).astype(np.uint8))
    y = dev(rng.normal(size=ROWS))
    dt, rf, gbt = DTPlan(D, 0), RFPlan(D, 0), GBTPlan(D)

    def dt_predict(t):
        return dt.predict(X, t["feature"], t["threshold"], t["first"], t["leaf"], t["value"][1:])

    def rf_predict(t):
        both = [small_tree(), t]
        cat = lambda k, dtype: np.ascontiguousarray(                      # noqa: E731
            np.concatenate([b[k] for b in both]), dtype=dtype)
        flat = (np.array([0, 3, 6], dtype=np.int32), np.array([0, 2, 4], dtype=np.int32),
                cat("feature", np.int32), cat("threshold", np.float64), cat("first", np.int32),
                cat("leaf", np.int32), np.array([[1.0], [2.0], [1.0], [2.0]]))
        return rf.predict(X, flat, pred=True)

    def gbt_update(rows, asImage):
        def call(t):
            return gbt.update(rows, flat_of(t, asImage), 1.0, "squared", y, None,
                              torch.zeros_like(y))
        return call

    def gbt_predict(t):
        return gbt.predict(X, [flat_of(small_tree(), False), flat_of(t, False)], [1.0, 0.1], False,
                           pred=True)

    # (the entry, the faults it checks, the tree its message names)
    entries = [(dt_predict, ("first", "feature", "leaf"), None),
               (rf_predict, ("first", "feature", "leaf"), "of tree 1"),
               (gbt_update(image, True), ("first", "feature", "bin"), None),
               (gbt_update(X, False), ("first", "feature"), None),
               (gbt_predict, ("first", "feature"), "of tree 1")]
    for call, checked, names in entries:
        call(small_tree())                                  # the tree itself is walked
        for fault, value, message in FAULTS:
            if fault not in checked:
                continue
            for match in filter(None, (message, names)):
                with pytest.raises(N.IllegalArgumentException, match=match):
                    call(small_tree(fault, value))
    torch.cuda.synchronize()
