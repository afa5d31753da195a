"""The entry-by-entry bound of a fixed-order fp64 fold, shared by the KMeans
conformance tests (test_kmeans_sparse_conformance.py, test_kmeans_dense_conformance.py)."""
import math

import numpy as np

U = 2.0 ** -53                       # unit roundoff of fp64


def check_entries(got, prior, calls, what, allowance=0.0):
    """got: a device buffer after accumulate calls into prior; calls: per call
    the (entry index, term) arrays of the terms the device folds.

    Derivation of the bound.  The device adds to an entry the same m fp64
    terms t_1..t_m as the host builds (one correctly rounded product each, so
    they are bit-identical), folded in some fixed tree order: m - 1 rounded
    additions.  Any order of m - 1 additions of error at most 2**-53 relative
    each is within (m - 1) * 2**-53 * sum|t| of the exact sum to first order
    (Higham, Accuracy and Stability of Numerical Algorithms, 4.2); one more
    2**-53 * sum|t| covers the rounding of the reference and the higher-order
    terms, so the bound is m * 2**-53 * sum|t| against math.fsum(terms),
    which is the exact sum rounded once.  The fold is then added to the
    entry's prior content s0: the reference is fsum([s0, fsum(terms)]) and
    that addition's rounding adds 2**-53 * (|s0| + sum|t|); a prior of 0.0
    adds exactly and gains nothing.  A second call folds into the first
    call's result in the same way.  An entry without terms is never written:
    it keeps its prior bits.

    allowance (0.0: none) widens an entry's bound by allowance * sum|t|, for a
    path that documents a correction of that relative size of its own."""
    got, prior = np.asarray(got, np.float64), np.asarray(prior, np.float64)
    ref = prior.copy()
    bound = np.zeros(len(prior))
    touched = np.zeros(len(prior), dtype=bool)
    for keys, t in calls:
        order = np.argsort(keys, kind="stable")
        ks, ts = keys[order], t[order]
        uniq, start = np.unique(ks, return_index=True)
        end = np.append(start[1:], len(ks))
        for e, s, f in zip(uniq.tolist(), start.tolist(), end.tolist()):
            tt = ts[s:f].tolist()
            total, mag = math.fsum(tt), math.fsum(abs(x) for x in tt)
            b = len(tt) * U * mag + allowance * mag
            s0 = ref[e]
            if s0 == 0.0:
                ref[e] = total
            else:
                ref[e] = math.fsum([s0, total])
                b += U * (abs(s0) + mag)
            bound[e] += b
            touched[e] = True
    err = np.abs(got - ref)
    bad = np.flatnonzero(touched & ~(err <= bound))
    assert bad.size == 0, (
        f"{what}: {bad.size} of {int(touched.sum())} entries past their bound; first "
        + ", ".join(f"[{i}] got {got[i]!r} ref {ref[i]!r} err {err[i]:.3e} bound {bound[i]:.3e}"
                    for i in bad[:5]))
    same = got.view(np.int64) == prior.view(np.int64)
    assert same[~touched].all(), (
        f"{what}: entries without terms changed: {np.flatnonzero(~touched & ~same)[:8]}")
    return touched
