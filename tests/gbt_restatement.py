"""A row-by-row restatement of what cycloneml_amd/gbt.py adds to the trees: the
three losses (mllib/tree/loss), the boosting loop of GradientBoostedTrees.boost
grown tree by tree, the walk over binned rows, the ensemble's sums and the
importances.  Plain Python floats and loops; a tree's fit is
random_forest_restatement's forest of one tree (which bins the rows again for
every tree: the bins do not depend on the labels), its arithmetic
decision_tree_restatement's.  exp and log1p are the math module's.
"""
import math

import decision_tree_restatement as R
import random_forest_restatement as F


# ---------------------------------------------------------------------- losses
def jexp(x):
    """The JVM's Math.exp overflows to Infinity; math.exp raises."""
    try:
        return math.exp(x)
    except OverflowError:
        return float("inf")


def log1p_exp(x):
    if x > 0:
        return x + math.log1p(math.exp(-x))
    return math.log1p(math.exp(x))


def gradient(loss, pred, label):
    if loss == "squared":
        return -2.0 * (label - pred)
    if loss == "absolute":
        return 1.0 if label - pred < 0 else -1.0
    assert loss == "logistic"
    return -4.0 * label / (1.0 + jexp(2.0 * label * pred))


def error(loss, pred, label):
    if loss == "squared":
        err = label - pred
        return err * err
    if loss == "absolute":
        return abs(label - pred)
    assert loss == "logistic"
    margin = 2.0 * label * pred
    return 2.0 * log1p_exp(-margin)


def probability(margin):
    return 1.0 / (1.0 + jexp(-2.0 * margin))


# ----------------------------------------------------------------------- walks
def leaf_of(root, x):
    nd = root
    while not nd.isLeaf:
        nd = nd.left if x[nd.split[0]] <= nd.split[1] else nd.right
    return nd


def split_bin(thresholds, nd):
    """The position of the node's threshold among its feature's thresholds."""
    return list(thresholds[nd.split[0]]).index(nd.split[1])


def leaf_of_binned(root, thresholds, bins):
    nd = root
    while not nd.isLeaf:
        nd = nd.left if int(bins[nd.split[0]]) <= split_bin(thresholds, nd) else nd.right
    return nd


def flat_walk(feature, splitOrThreshold, firstChild, value, row):
    """The leaf value of a row through a tree given as arrays: row[feature] <=
    splitOrThreshold goes to firstChild."""
    node = 0
    while firstChild[node] >= 0:
        left = row[feature[node]] <= splitOrThreshold[node]
        node = firstChild[node] + (0 if left else 1)
    return float(value[node]), node


def update(leaves, weight, loss, pred, labels, w):
    """updatePredictionError and computeWeightedError over rows whose leaf
    values are given: (pred, -gradient, errors, sum of e w, sum of w) in row
    order."""
    out, resid, errs = [], [], []
    es, ws = 0.0, 0.0
    for r in range(len(labels)):
        p = float(pred[r]) + float(leaves[r]) * weight
        y = float(labels[r])
        e = error(loss, p, y)
        out.append(p)
        resid.append(-gradient(loss, p, y))
        errs.append(e)
        wr = 1.0 if w is None else float(w[r])
        es += e * wr
        ws += wr
    return out, resid, errs, es, ws


# ------------------------------------------------------------------------ boost
def fit_gbt(X, y, w, loss, classifier, maxIter, stepSize, m, maxDepth=5, maxBins=32,
            minInstancesPerNode=1, minWeightFractionPerNode=0.0, minInfoGain=0.0,
            subsamplingRate=1.0, seed=0, validation=None, validationTol=0.01, perturb=None):
    """(roots, weights, thresholds, the residuals every tree was fitted to).
    validation: (Xv, yv, wv | None); perturb(iteration, residuals): the
    residuals the next tree is fitted to instead (a test of near-ties)."""
    n = len(X)
    labels = [2.0 * float(v) - 1.0 if classifier else float(v) for v in y]
    pred = [0.0] * n
    target = list(labels)
    if validation is not None:
        Xv, yv, wv = validation
        vlabels = [2.0 * float(v) - 1.0 if classifier else float(v) for v in yv]
        vpred = [0.0] * len(Xv)
    roots, weights, targets = [], [], []
    best, bestM = None, 1
    thresholds = None
    for it in range(maxIter):
        fitted = target if perturb is None else perturb(it, target)
        targets.append(list(fitted))
        (root,), thresholds, _ = F.fit_forest(
            X, fitted, w, 0, "variance", 1, m, maxDepth, maxBins, minInstancesPerNode,
            minWeightFractionPerNode, minInfoGain, False, subsamplingRate, seed + it)
        weight = 1.0 if it == 0 else stepSize
        roots.append(root)
        weights.append(weight)
        bins = [[R.bin_of(thresholds[f], float(X[r][f])) for f in range(len(X[0]))]
                for r in range(n)]
        leaves = [leaf_of_binned(root, thresholds, bins[r]).prediction for r in range(n)]
        pred, target, _, _, _ = update(leaves, weight, loss, pred, labels, w)
        if validation is None:
            continue
        vbins = [[R.bin_of(thresholds[f], float(Xv[r][f])) for f in range(len(X[0]))]
                 for r in range(len(Xv))]
        vleaves = [leaf_of_binned(root, thresholds, vbins[r]).prediction for r in range(len(Xv))]
        vpred, _, _, es, ws = update(vleaves, weight, loss, vpred, vlabels, wv)
        current = es / ws
        if it == 0:
            best = current
        elif best - current < validationTol * max(current, 0.01):
            break
        elif current < best:
            best, bestM = current, it + 1
    if validation is not None:
        roots, weights = roots[:bestM], weights[:bestM]
    return roots, weights, thresholds, targets


def structure(nd):
    """The tree without its values: nested (feature, threshold, left, right)."""
    if nd.isLeaf:
        return None
    return (nd.split[0], nd.split[1], structure(nd.left), structure(nd.right))


def leaf_values(nd):
    if nd.isLeaf:
        return [nd.prediction]
    return leaf_values(nd.left) + leaf_values(nd.right)


# -------------------------------------------------------------------- ensemble
def margin(roots, weights, x):
    s = 0.0
    for root, wt in zip(roots, weights):
        s += leaf_of(root, x).prediction * wt
    return s


def classify(mg):
    """(raw, probability, prediction) of a margin."""
    p = probability(mg)
    return [-mg, mg], [1.0 - p, p], (1.0 if mg > 0 else 0.0)


def evaluate_each_iteration(roots, weights, X, y, w, loss, classifier):
    out = []
    pred = [0.0] * len(X)
    labels = [2.0 * float(v) - 1.0 if classifier else float(v) for v in y]
    for root, wt in zip(roots, weights):
        leaves = [leaf_of(root, x).prediction for x in X]
        pred, _, _, es, ws = update(leaves, wt, loss, pred, labels, w)
        out.append(es / ws)
    return out


def importances(roots, d):
    """gain count per feature, NOT normalised per tree, the trees' vectors
    added in tree order, normalised once."""
    total = [0.0] * d
    for root in roots:
        imp = [0.0] * d

        def walk(nd):
            if nd.isLeaf:
                return
            imp[nd.split[0]] += nd.gain * R.count_of(nd.stats, 0)
            walk(nd.left)
            walk(nd.right)

        walk(root)
        total = [a + b for a, b in zip(total, imp)]
    s = 0.0
    for v in total:
        s += v
    return [v / s for v in total] if s != 0.0 else total
