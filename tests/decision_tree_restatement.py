"""A row-by-row restatement of the DecisionTree fit and descent that
cycloneml_amd/tree.py implements (Spark 3.3: RandomForest.scala's
findSplitsForContinuousFeature, binsToBestSplit and the level loop,
TreePoint's binning, the gini / entropy / variance calculators, Node.scala's
toNode(prune = true)): plain Python loops, one row, node, feature and split at a
time, every sum in row order.  The natural logarithm of the entropy is numpy's
on a scalar, the one piece of arithmetic shared with the code under test.
"""
import bisect

import numpy as np

EPS = 2.0 ** -52
INVALID = -float(np.finfo(np.float64).max)


def exact_rows(n, d, seed, numClasses=3):
    """Small integer features, integer labels and weights in eighths: every
    sum of a fit is exact, so two summation orders give the same bytes.
    (X, y for a classifier, y for a regressor, w)."""
    rng = np.random.default_rng(seed)
    X = rng.integers(-6, 7, size=(n, d)).astype(np.float64)
    score = X[:, 0] + 2.0 * (X[:, min(1, d - 1)] > 0) - X[:, d - 1] // 3
    ycls = np.mod(np.floor(score / 3.0) + rng.integers(0, 2, size=n), numClasses).astype(np.float64)
    yreg = (score + rng.integers(-2, 3, size=n)).astype(np.float64)
    w = rng.integers(1, 17, size=n).astype(np.float64) / 8.0
    return X, ycls, yreg, w


def find_splits(values, weights, numSplits, W):
    counts = {}
    partNum, cnt = 0.0, 0
    for v, w in zip(values, weights):
        v, w = float(v), float(w)
        if v == 0.0:
            continue
        counts[v] = counts.get(v, 0.0) + w
        partNum += w
        cnt += 1
    if cnt == 0:
        return []
    if W - partNum > EPS * cnt * 100:
        counts[0.0] = W - partNum
    vals = sorted(counts)
    possible = len(vals) - 1
    if possible == 0:
        return []
    if possible <= numSplits:
        return [(vals[i - 1] + vals[i]) / 2.0 for i in range(1, len(vals))]
    stride = W / (numSplits + 1)
    out = []
    cur, target = counts[vals[0]], stride
    for index in range(1, len(vals)):
        prev = cur
        cur += counts[vals[index]]
        if abs(prev - target) < abs(cur - target):
            out.append((vals[index - 1] + vals[index]) / 2.0)
            target += stride
    return out


def bin_of(thresholds, x):
    """The number of thresholds strictly below x."""
    return bisect.bisect_left(list(thresholds), x)


def add_row(stats, C, y, w):
    if C:
        stats[int(y)] += w
        stats[C] += 1.0
    else:
        stats[0] += w
        stats[1] += w * y
        stats[2] += w * y * y
        stats[3] += 1.0


def histogram(image, y, w, rows, C, B):
    """feature x bin x stats over `rows`, in row order."""
    d = len(image[0]) if len(image) else 0
    S = C + 1 if C else 4
    h = [[[0.0] * S for _ in range(B)] for _ in range(d)]
    for r in rows:
        for f in range(d):
            add_row(h[f][image[r][f]], C, float(y[r]), 1.0 if w is None else float(w[r]))
    return h


def count_of(stats, C):
    if not C:
        return stats[0]
    s = 0.0
    for c in range(C):
        s += stats[c]
    return s


def calculate(stats, C, impurity):
    total = count_of(stats, C)
    if total == 0.0:
        return 0.0
    if impurity == "variance":
        return (stats[2] - stats[1] * stats[1] / total) / total
    if impurity == "gini":
        imp = 1.0
        for c in range(C):
            f = stats[c] / total
            imp -= f * f
        return imp
    imp = 0.0
    ln2 = float(np.log(np.float64(2.0)))
    for c in range(C):
        if stats[c] != 0.0:
            f = stats[c] / total
            imp -= f * (float(np.log(np.float64(f))) / ln2)
    return imp


def predict_of(stats, C):
    if C:
        best = 0
        for c in range(1, C):
            if stats[c] > stats[best]:
                best = c
        return float(best)
    return stats[1] / stats[0] if stats[0] != 0.0 else 0.0


def best_split(h, numSplits, C, impurity, minInstances=1, minWeight=0.0, minInfoGain=0.0):
    """(feature, split, gain, parent, impurity, left, right) of one node's
    histogram; feature -1 when no feature has splits."""
    S = C + 1 if C else 4
    parent, imp = None, None
    best = (-1, -1, INVALID, None, None, None, None)
    for f in range(len(h)):
        ns = numSplits[f]
        if ns == 0:
            continue
        cum = []
        run = [0.0] * S
        for b in range(ns + 1):
            run = [run[s] + h[f][b][s] for s in range(S)]
            cum.append(run)
        fbest = None
        for s in range(ns):
            left = cum[s]
            right = [cum[ns][q] - left[q] for q in range(S)]
            if parent is None:
                parent = [left[q] + right[q] for q in range(S)]
                imp = calculate(parent, C, impurity)
            lc, rc = count_of(left, C), count_of(right, C)
            if left[S - 1] < minInstances or right[S - 1] < minInstances \
                    or lc < minWeight or rc < minWeight:
                gain = INVALID
            else:
                total = lc + rc
                if total == 0.0:
                    gain = float("nan")          # the JVM's 0.0 / 0.0
                else:
                    gain = imp - (lc / total) * calculate(left, C, impurity) \
                        - (rc / total) * calculate(right, C, impurity)
                if not gain >= minInfoGain:      # NaN (no weight on either side) included
                    gain = INVALID
            if fbest is None or gain > fbest[2]:
                fbest = (f, s, gain, parent, imp, left, right)
        if best[0] < 0 or fbest[2] > best[2]:
            best = fbest
    return best


class RNode:
    def __init__(self, stats, impurity, C):
        self.stats, self.impurity, self.C = list(stats), impurity, C
        self.prediction = predict_of(stats, C)
        self.gain, self.split, self.left, self.right = 0.0, None, None, None

    @property
    def isLeaf(self):
        return self.left is None


def prune(nd):
    if nd.isLeaf:
        return nd
    nd.left, nd.right = prune(nd.left), prune(nd.right)
    if nd.left.isLeaf and nd.right.isLeaf and nd.left.prediction == nd.right.prediction:
        return RNode(nd.stats, nd.impurity, nd.C)
    return nd


def fit(X, y, w, C, impurity, maxDepth=5, maxBins=32, minInstancesPerNode=1,
        minWeightFractionPerNode=0.0, minInfoGain=0.0, pruneTree=True):
    """(root, thresholds) of a fit on rows few enough that the sample of
    find_splits is every row."""
    n, d = len(X), len(X[0])
    assert max(maxBins * maxBins, 10000) >= n
    ws = [1.0] * n if w is None else [float(v) for v in w]
    W = 0.0
    for v in ws:
        W += v
    numSplitsMax = min(maxBins, n) - 1
    thresholds = [find_splits([X[r][f] for r in range(n)], ws, numSplitsMax, W) for f in range(d)]
    numSplits = [len(t) for t in thresholds]
    B = max(numSplits) + 1
    image = [[bin_of(thresholds[f], float(X[r][f])) for f in range(d)] for r in range(n)]
    minWeight = minWeightFractionPerNode * W
    rows_of = {1: list(range(n))}
    nodes = {}
    level = 0
    while rows_of:
        nxt = {}
        for i in sorted(rows_of):
            rows = rows_of[i]
            h = histogram(image, y, w, rows, C, B)
            f, s, gain, parent, imp, left, right = best_split(
                h, numSplits, C, impurity, minInstancesPerNode, minWeight, minInfoGain)
            if i not in nodes:
                if parent is None:
                    parent = [0.0] * (C + 1 if C else 4)
                    for b in range(B):
                        parent = [parent[q] + h[0][b][q] for q in range(len(parent))]
                    imp = calculate(parent, C, impurity)
                nodes[i] = RNode(parent, imp, C)
            node = nodes[i]
            if gain <= 0.0 or level == maxDepth:
                continue
            node.gain, node.split = gain, (f, thresholds[f][s])
            node.left = RNode(left, calculate(left, C, impurity), C)
            node.right = RNode(right, calculate(right, C, impurity), C)
            nodes[2 * i], nodes[2 * i + 1] = node.left, node.right
            sides = ([r for r in rows if image[r][f] <= s], [r for r in rows if image[r][f] > s])
            for child, idx, rs in ((node.left, 2 * i, sides[0]), (node.right, 2 * i + 1, sides[1])):
                if not (level + 1 == maxDepth or abs(child.impurity) < EPS):
                    nxt[idx] = rs
        rows_of = nxt
        level += 1
    root = nodes[1]
    return (prune(root) if pruneTree else root), thresholds


def descend(root, x):
    """(leaf node, its index among the leaves of a pre-order walk)."""
    leaves = []

    def walk(nd):
        if nd.isLeaf:
            leaves.append(nd)
        else:
            walk(nd.left)
            walk(nd.right)

    walk(root)
    nd = root
    while not nd.isLeaf:
        nd = nd.left if x[nd.split[0]] <= nd.split[1] else nd.right
    return nd, [id(q) for q in leaves].index(id(nd))


def probability(raw):
    s = 0.0
    for v in raw:
        s += v
    return [v / s for v in raw] if s != 0.0 else list(raw)


def same_tree(a, b):
    """Structure, splits, statistics, gains and predictions by bytes; a: tree.py's
    Node, b: RNode."""
    if a.isLeaf != b.isLeaf:
        return False
    if np.asarray(a.stats, dtype=np.float64).tobytes() != np.asarray(b.stats, dtype=np.float64).tobytes():
        return False
    if np.float64(a.prediction).tobytes() != np.float64(b.prediction).tobytes() \
            or np.float64(a.impurity).tobytes() != np.float64(b.impurity).tobytes():
        return False
    if a.isLeaf:
        return True
    if a.split[0] != b.split[0] or np.float64(a.split[1]).tobytes() != np.float64(b.split[1]).tobytes():
        return False
    if np.float64(a.gain).tobytes() != np.float64(b.gain).tobytes():
        return False
    return same_tree(a.left, b.left) and same_tree(a.right, b.right)
