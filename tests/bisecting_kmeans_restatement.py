"""BisectingKMeans restated in plain numpy and Python, row by row, after Spark
3.3's mllib/clustering/BisectingKMeans.scala and BisectingKMeansModel.scala.
Distances and norms are the oracle's (find_closest, sqdist, norm2), the random
draws the oracle's JavaRandom: nothing here comes from the package.

Divisible clusters are visited in ascending node index (the project's rule;
Spark walks a Scala Map).  maxIter = 0 takes no summaries, so the clusters are
the root alone.

Also the input generators of the tests:
  exact rows  integers below 2^20 with weights in eighths: sum and weightSum
              are exact in any order
  real rows   Gaussian blobs
"""
import math

import numpy as np

import oracle

ROOT = 1
EPSILON = 2.0 ** -52
LEVEL_LIMIT = math.log10(float(2 ** 63 - 1)) / math.log10(2.0)


# ------------------------------------------------------------------ inputs
def exact_rows(n, d, seed=0, weighted=True, groups=4):
    """(X, w): integer rows below 2^20 around `groups` integer centers, weights
    in eighths (None when not weighted)."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 1 << 19, size=(groups, d))
    X = base[rng.integers(0, groups, size=n)] + rng.integers(0, 1 << 10, size=(n, d))
    w = rng.integers(1, 64, size=n) / 8.0 if weighted else None
    return X.astype(np.float64), w


def real_rows(sizes, d, seed=0, spread=50.0):
    """Unit Gaussian blobs of the given sizes, rows shuffled; (X, blob of each
    row).  Blob b sits at its bits, the top one on the widest axis (spread
    8^q), so halving by halving separates the blobs: a bisecting fit with k =
    len(sizes), a power of two, can find them."""
    rng = np.random.default_rng(seed)
    bits = max(1, (len(sizes) - 1).bit_length())
    assert d >= bits
    centers = rng.normal(size=(len(sizes), d))
    for b in range(len(sizes)):
        for q in range(bits):
            centers[b, q] += ((b >> q) & 1) * spread * 8.0 ** q
    X = np.concatenate([centers[b] + rng.normal(size=(s, d)) for b, s in enumerate(sizes)])
    lab = np.concatenate([np.full(s, b) for b, s in enumerate(sizes)])
    p = rng.permutation(X.shape[0])
    return np.ascontiguousarray(X[p]), lab[p]


# ----------------------------------------------------------------- summary
class Summary:
    def __init__(self, d):
        self.n, self.wsum, self.sumsq, self.sum = 0, 0.0, 0.0, np.zeros(d)

    def add(self, x, norm, w):
        self.n += 1
        self.wsum = self.wsum + w
        self.sumsq = self.sumsq + norm * norm * w
        self.sum = self.sum + w * x          # axpy

    def finish(self):
        self.size = self.n
        self.center = self.sum * (1.0 / self.wsum)      # BLAS.scal
        self.norm = oracle.norm2(self.center)
        self.cost = max(self.sumsq - self.wsum * self.norm * self.norm, 0.0)
        return self


def summarize(X, norms, w, assign):
    """{node: finished Summary} over the rows with assign[r] is not None."""
    out = {}
    for r in range(X.shape[0]):
        i = assign[r]
        if i is None:
            continue
        if i not in out:
            out[i] = Summary(X.shape[1])
        out[i].add(X[r], float(norms[r]), 1.0 if w is None else float(w[r]))
    return {i: s.finish() for i, s in out.items()}


def update_assignments(X, norms, assign, div, centers):
    out = list(assign)
    for r in range(X.shape[0]):
        i = assign[r]
        if i not in div:
            continue
        kids = [c for c in (2 * i, 2 * i + 1) if c in centers]
        if kids:
            C = np.stack([centers[c][0] for c in kids])
            cn = np.array([centers[c][1] for c in kids])
            idx, _ = oracle.find_closest(C, cn, X[r], float(norms[r]))
            out[r] = kids[idx]
    return out


def fit(X, w=None, k=4, maxIter=20, minDiv=1.0, seed=0):
    """{node index: Summary} of active ++ inactive, and the rows' final nodes."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    n, d = X.shape
    norms = oracle.row_norms(X)
    assign = [ROOT] * n
    active, inactive = summarize(X, norms, w, assign), {}
    size = active[ROOT].size
    minSize = math.ceil(minDiv) if minDiv >= 1.0 else math.ceil(minDiv * size)
    random = oracle.JavaRandom(seed)
    needed, level = k - 1, 1
    while active and needed > 0 and level < LEVEL_LIMIT:
        div = [i for i in sorted(active)
               if active[i].size >= minSize and active[i].cost > EPSILON * active[i].size]
        if len(div) > needed:
            div = sorted(sorted(div, key=lambda i: (-active[i].size, i))[:needed])
        if not div:
            inactive.update(active)
            active = {}
            break
        centers = {}
        for i in div:
            c = active[i]
            noise = np.array([random.next_double() for _ in range(d)])
            lvl = 1e-4 * c.norm
            left = c.center + (-lvl) * noise
            right = c.center + lvl * noise
            centers[2 * i] = (left, oracle.norm2(left))
            centers[2 * i + 1] = (right, oracle.norm2(right))
        last = None
        for _ in range(maxIter):
            new = update_assignments(X, norms, assign, div, centers)
            picked = [a if b in div else None for a, b in zip(new, assign)]
            last = summarize(X, norms, w, picked)
            centers = {i: (s.center, s.norm) for i, s in last.items()}
        assign = update_assignments(X, norms, assign, div, centers)
        inactive.update(active)
        active = last if last is not None else {}
        needed -= len(div)
        level += 1
    clusters = dict(inactive)
    clusters.update(active)
    return clusters, assign


# -------------------------------------------------------------------- tree
class Node:
    def __init__(self, index, size, center, cost, height, children):
        self.index, self.size, self.center, self.cost = index, size, center, cost
        self.height, self.children = height, children


def build_tree(clusters):
    counters = {"leaf": 0, "internal": -1}

    def build(raw):
        c = clusters[raw]
        if 2 * raw in clusters:
            index = counters["internal"]
            counters["internal"] -= 1
            kids = [i for i in (2 * raw, 2 * raw + 1) if i in clusters]
            height = max(math.sqrt(oracle.sqdist(c.center, clusters[i].center)) for i in kids)
            return Node(index, c.size, c.center, c.cost, height, [build(i) for i in kids])
        index = counters["leaf"]
        counters["leaf"] += 1
        return Node(index, c.size, c.center, c.cost, 0.0, [])

    return build(ROOT)


def walk(node):
    """The nodes depth first, children left first."""
    yield node
    for c in node.children:
        yield from walk(c)


def leaves(node):
    return [nd for nd in walk(node) if not nd.children]


def training_cost(root):
    s = 0.0
    for leaf in leaves(root):
        s = s + leaf.cost
    return s


def predict(root, x):
    """(leaf index, cost) of one row."""
    node, cost = root, None
    while node.children:
        ds = [oracle.sqdist(c.center, x) for c in node.children]
        best = 0
        for q in range(1, len(ds)):
            if ds[q] < ds[best]:       # minBy: the first minimum
                best = q
        node, cost = node.children[best], ds[best]
    if cost is None:
        cost = oracle.sqdist(root.center, x)
    return node.index, cost


def tree_from_arrays(centers, firstChild, numChildren):
    """A Node tree from flat arrays (node 0 the root, children at firstChild,
    firstChild + 1), indexed as build_tree does."""
    counters = {"leaf": 0, "internal": -1}

    def build(i):
        kids = [int(firstChild[i]) + q for q in range(int(numChildren[i]))]
        if kids:
            index = counters["internal"]
            counters["internal"] -= 1
            return Node(index, 0, centers[i], 0.0, 0.0, [build(c) for c in kids])
        index = counters["leaf"]
        counters["leaf"] += 1
        return Node(index, 0, centers[i], 0.0, 0.0, [])

    return build(0)


# -------------------------------------------------------- one device step
def step(X, norms, slot, table, C, cn):
    """newSlot per row: findClosest over the children on offer, left first;
    keepNew for a row that is offered none."""
    out = np.empty(X.shape[0], dtype=np.int32)
    for r in range(X.shape[0]):
        left, right, keep = (int(v) for v in table[slot[r]])
        kids = [c for c in (left, right) if c >= 0]
        if not kids:
            out[r] = keep
            continue
        idx, _ = oracle.find_closest(C[kids], cn[kids], X[r], float(norms[r]))
        out[r] = kids[idx]
    return out


def step_summary(X, norms, w, newSlot, K):
    """(count, buf, bar): the children's summary in row order as [wsum | sumSq |
    sum (K x d)], and per entry the sum of the absolute terms."""
    d = X.shape[1]
    count = np.zeros(K, dtype=np.int64)
    buf = np.zeros(K * (2 + d))
    bar = np.zeros(K * (2 + d))
    for r in range(X.shape[0]):
        c = int(newSlot[r])
        if not 0 <= c < K:
            continue
        wr = 1.0 if w is None else float(w[r])
        nr = float(norms[r])
        count[c] += 1
        buf[c] = buf[c] + wr
        buf[K + c] = buf[K + c] + nr * nr * wr
        sl = slice(2 * K + c * d, 2 * K + (c + 1) * d)
        buf[sl] = buf[sl] + wr * X[r]
        bar[c] += abs(wr)
        bar[K + c] += abs(nr * nr * wr)
        bar[sl] += np.abs(wr * X[r])
    return count, buf, bar
