"""Conformance of the block aggregators (cycloneml_amd/csrc/logistic_binary.hip,
logistic_multinomial.hip, logistic.hip, binary_rows.hpp, tiles.hip, csc.hip) at
their launch and tile edges.

Reference: ``ref_add`` below, a vectorised ``np.longdouble`` restatement of the
six ``add`` operations -- binary logistic, hinge, least squares, Huber, AFT,
multinomial -- after the Scala formulas oracle/oracle.py cites, with a stable
log1pExp and a max-subtracted softmax.  One CPU test holds it against
``oracle.*_add``.

Two kinds of operands:

* exact -- small integers everywhere (least squares: labelStd = 2, integer
  labelMean; Huber: sigma = 2, epsilon = 1.5), every partial sum far below
  2^53: hinge, least squares and Huber then give the same bits in any
  summation order and the comparison is ``array_equal``.  Every fifth row sits
  exactly on the hinge kink (1 - y'm == 0) or on Huber's |l| == sigma * eps.
* rounded -- real-valued draws, every entry checked on its own against an
  a-priori bound that holds for any summation order.  u = 2^-53,
  gamma(k) = k u / (1 - k u), L_i = terms of row i's dot, n_j = rows touching
  column j:

    margin      |dt_i| <= gamma(L_i + 2) A_i + gamma(F + 2) (|c_F| + sum|c_j s_j|)
                A_i = |offset| + sum_j |x_ij c_j|
    multiplier  |dm_i| <= w_i (K_i |dt_i| + 8 u phi_i)
    gradient    |dg_j| <= sum_i |x_ij| |dm_i| + gamma(n_j + 2) sum_i |m_i x_ij|
                (+ |s_j| sum|dm_i| + gamma(n + 2) |s_j| sum|m_i| when centred)
    loss, sigma entry: the same from the per-row terms; weight: gamma(n) sum w.

  K_i is the multiplier's Lipschitz constant in the margin (logistic 1/4,
  least squares 1, Huber quadratic 1/sigma, hinge and Huber linear 0, AFT
  exp(e_i)/sigma^2, multinomial 1/4 per class); phi_i is the magnitude of the
  multiplier's operands before they cancel (logistic sigmoid + label, hinge 1,
  least squares |t_i|, Huber |l_i|/sigma or eps, AFT (delta + exp e)/sigma,
  multinomial p_ic + [c == y_i]).  Where the formulas above leave a step out,
  the bound counts it, and says so:

  - least squares adds -label/labelStd to the margin: |label/labelStd| joins
    A_i and the count is L_i + 4 (the quotient, the product, two additions);
  - AFT's exponent is e = (log y - t)/sigma: |log y| joins A_i, the count is
    L_i + 5 (log, sigma = exp(.), the difference, the quotient), and K_i is
    taken at e_i + |de_i| so that it bounds the whole interval;
  - multinomial: p_c moves with every class margin, |dp_c| <= p_c (1 - p_c)
    (|dt_c| + max_k |dt_k|) <= 1/4 (|dt_c| + max_k |dt_k|); the rounding of
    t_c - max_k t_k, u (|t_c| + |max|), joins |dt_c|; the normalising sum of C
    terms adds gamma(C) p_c.

  The bounds themselves are evaluated in float64 (their own rounding is 1e-13
  of them).  For hinge and Huber every rounded problem asserts on the CPU that
  its reference margins stay 1e-9 from the kink, so no row changes branch.

The largest err / bound per group is printed by ``test_report_error_ratios``
(pytest -rP) and stands in every assertion message.
"""
import numpy as np
import pytest

import oracle

LD = np.longdouble
U = 2.0 ** -53
RATIOS = {}          # group -> largest err / bound seen (rounded operands)
BIN = ("log", "hinge", "ls", "huber", "aft")
EXACT_KINDS = ("hinge", "ls", "huber")
EXACT, ROUNDED = "exact", "rounded"


def gamma(k):
    k = np.asarray(k, dtype=np.float64)
    return k * U / (1.0 - k * U)


# ------------------------------------------------------------ rows


class Rows:
    """A block's rows, dense (X) or CSR (rowptr, colidx, values), with the
    products the reference needs: longdouble for the values, float64 for the
    magnitude sums of the bounds."""

    def __init__(self, X=None, csr=None, F=None):
        self.X, self.csr = X, csr
        if X is not None:
            self.n, self.F = X.shape
            self.L = np.full(self.n, self.F)
            self.ncol = np.full(self.F, self.n)
        else:
            rp, ci, _ = csr
            self.n, self.F = rp.size - 1, F
            self.L = np.diff(rp)
            self.ncol = np.bincount(ci, minlength=F)
            self.ri = np.repeat(np.arange(self.n), self.L)
        self._xl = None

    def dense(self):
        if self.X is not None:
            return self.X
        rp, ci, vv = self.csr
        X = np.zeros((self.n, self.F))
        X[self.ri, ci] = vv
        return X

    def _ld(self):
        if self._xl is None:
            self._xl = self.dense().astype(LD)
        return self._xl

    @staticmethod
    def _segsum(p, ptr):
        out = np.zeros(ptr.size - 1, dtype=p.dtype)
        ne = ptr[1:] > ptr[:-1]
        if p.size:
            out[ne] = np.add.reduceat(p, ptr[:-1][ne])
        return out

    def dot(self, c):
        if self.csr is None or c.ndim == 2:
            return self._ld() @ c
        rp, ci, vv = self.csr
        return self._segsum(vv.astype(LD) * c[ci], rp)

    def tdot(self, m):
        if self.csr is None or m.ndim == 2:
            return self._ld().T @ m
        rp, ci, vv = self.csr
        order = np.argsort(ci, kind="stable")
        cp = np.concatenate([[0], np.cumsum(self.ncol)])
        return self._segsum((vv.astype(LD) * m[self.ri])[order], cp)

    def absdot(self, c):
        c = np.abs(np.asarray(c, dtype=np.float64))
        if self.csr is None or c.ndim == 2:
            return np.abs(self.dense()) @ c
        rp, ci, vv = self.csr
        return np.bincount(self.ri, np.abs(vv) * c[ci], minlength=self.n)

    def abstdot(self, m):
        m = np.abs(np.asarray(m, dtype=np.float64))
        if self.csr is None or m.ndim == 2:
            return np.abs(self.dense()).T @ m
        rp, ci, vv = self.csr
        return np.bincount(ci, np.abs(vv) * m[self.ri], minlength=self.F)

    def oracle_block(self, y, w):
        if self.csr is None:
            return dict(labels=y, weights=w, X=self.X)
        rp, ci, vv = self.csr
        return dict(labels=y, weights=w, rowptr=rp, colidx=ci, values=vv, F=self.F)


# ------------------------------------------------------------ the reference


def _log1pexp(x):
    x = np.asarray(x, dtype=LD)
    return np.where(x > 0, x + np.log1p(np.exp(-np.abs(x))), np.log1p(np.exp(np.minimum(x, 0))))


class Ref:
    """grad / loss / weight in longdouble with their entrywise bounds, and
    `kink`: the smallest distance of a counted row's margin from a branch
    switch (hinge, Huber; inf otherwise)."""


def ref_add(p):
    """The `add` of problem p (see _problem) over one block, from a zero state."""
    if p["kind"] == "mlr":
        return _ref_mlr(p)
    kind, rows, fi = p["kind"], p["rows"], p["fi"]
    n, F = rows.n, rows.F
    coef = np.asarray(p["coef"], dtype=LD)
    y = np.asarray(p["y"], dtype=LD)
    w = np.ones(n, dtype=LD) if p["w"] is None else np.asarray(p["w"], dtype=LD)
    sm = None if p["sm"] is None else np.asarray(p["sm"], dtype=LD)
    c = coef[:F]
    ceff = np.where(np.asarray(p["inv"]) != 0, c, 0) if kind == "ls" else c
    centred = fi and (p["fwm"] if kind == "log" else True)
    base = LD(0)
    if fi:
        base = LD(p["ymean"]) / LD(p["ystd"]) if kind == "ls" else coef[F]
    off, offabs = base, 0.0
    if centred:
        off = base - (c * sm).sum()
        offabs = float(abs(base) + np.abs(c * sm).sum())
    A = float(abs(off)) + rows.absdot(ceff)
    t = off + rows.dot(ceff)
    kx = 2
    if kind == "ls":
        lab = -y / LD(p["ystd"])
        t, A, kx = t + lab, A + np.abs(lab).astype(np.float64), 4
    if kind == "aft":
        sigma = np.exp(coef[F + 1])
        ly = np.log(y)
        A, kx = A + np.abs(ly).astype(np.float64), 5
    dt = gamma(rows.L + kx) * A + float(gamma(F + 2)) * offabs
    pos = w > 0
    wf = w.astype(np.float64)
    z = np.zeros(n, dtype=LD)
    s = ds = None
    kink = np.inf
    a = lambda v: np.abs(v).astype(np.float64)
    if kind == "log":
        sig = 1 / (1 + np.exp(-t))
        m = np.where(pos, w * (sig - y), z)
        dm = wf * (0.25 * dt + 8 * U * a(sig + y))
        lt = np.where(y > 0, _log1pexp(-t), _log1pexp(t))
        ell = np.where(pos, w * lt, z)
        dl = wf * (dt + 8 * U * (a(_log1pexp(-t)) + np.where(y > 0, 0.0, a(t))))
        wsum = w.sum()
    elif kind == "hinge":
        ys = y + y - 1
        h = 1 - ys * t
        act = pos & (h > 0)
        m = np.where(act, -ys * w, z)
        dm = act * wf * 8 * U
        ell = np.where(act, w * h, z)
        dl = act * wf * (dt + 8 * U * (1 + a(t)))
        wsum = w.sum()
        if pos.any():
            kink = float(np.abs(h[pos]).min())
    elif kind == "ls":
        m = w * t
        dm = wf * (dt + 8 * U * a(t))
        ell = w * t * t / 2
        dl = wf * (a(t) * dt + 0.5 * dt * dt + 8 * U * a(t * t / 2))
        wsum = w.sum()
    elif kind == "huber":
        sg, eps = coef[-1], LD(p["eps"])
        l = y - t
        quad = np.abs(l) <= sg * eps
        sign = np.where(l >= 0, LD(-1), LD(1))
        m = np.where(pos, np.where(quad, -w * l / sg, w * sign * eps), z)
        dm = np.where(quad, wf * (dt / float(sg) + 8 * U * a(l / sg)), wf * 8 * U * float(eps))
        ell = np.where(pos, np.where(quad, 0.5 * w * (sg + l * l / sg),
                                     0.5 * w * (sg + 2 * eps * np.abs(l) - sg * eps * eps)), z)
        dl = np.where(quad, wf * (a(l / sg) * dt + 0.5 * dt * dt / float(sg) +
                                  8 * U * a(0.5 * (sg + l * l / sg))),
                      wf * (float(eps) * dt + 8 * U * a(0.5 * (sg + 2 * eps * np.abs(l) +
                                                                 sg * eps * eps))))
        s = np.where(pos, np.where(quad, 0.5 * w * (1 - (l / sg) ** 2),
                                   0.5 * w * (1 - eps * eps)), z)
        ds = np.where(quad, wf * (a(l / (sg * sg)) * dt + 0.5 * (dt / float(sg)) ** 2 +
                                  8 * U * a(0.5 * (1 + (l / sg) ** 2))),
                      wf * 8 * U * float(0.5 * (1 + eps * eps)))
        wsum = w.sum()
        if pos.any():
            kink = float(np.abs(np.abs(l[pos]) - sg * eps).min())
    else:                                            # aft: w is the censor delta
        e = (ly - t) / sigma
        ee = np.exp(e)
        de = dt / float(sigma)
        eh = a(ee) * np.exp(de)                      # exp(e) anywhere within |de|
        m = (w - ee) / sigma
        dm = eh / float(sigma) * de + 8 * U * a((w + ee) / sigma)
        ell = w * np.log(sigma) - w * e + ee
        dl = (wf + eh) * de + 8 * U * a(w * np.abs(np.log(sigma)) + w * np.abs(e) + ee)
        s = w + (w - ee) * e
        ds = (a(w - ee) + eh * a(e) + eh) * de + 8 * U * a(w + (w + ee) * np.abs(e))
        wsum = LD(n)
    g = rows.tdot(m)
    gb = rows.abstdot(dm) + gamma(rows.ncol + 2) * rows.abstdot(m)
    msum, dmsum, mabs = m.sum(), float(dm.sum()), float(np.abs(m).sum())
    gn = float(gamma(n + 2))
    tail, tailb = [], []
    if kind != "ls":
        if centred:
            g = g - sm * msum
            gb = gb + a(sm) * (dmsum + gn * mabs)
        if fi:
            tail.append(msum)
            tailb.append(dmsum + gn * mabs)
        elif kind == "aft":                          # the intercept slot stays
            tail.append(LD(0))
            tailb.append(0.0)
    if s is not None:
        tail.append(s.sum())
        tailb.append(float(ds.sum()) + gn * float(np.abs(s).sum()))
    r = Ref()
    r.grad = np.concatenate([g, np.array(tail, dtype=LD)])
    r.gbound = np.concatenate([gb, np.array(tailb, dtype=np.float64)])
    r.loss, r.lbound = ell.sum(), float(np.sum(dl)) + gn * float(np.abs(ell).sum())
    r.weight, r.wbound = wsum, float(gamma(n)) * float(wsum)
    r.kink = kink
    r.magnitude = max(float(rows.abstdot(m).max(initial=0)), float(np.abs(ell).sum()), mabs,
                      float(A.max(initial=0)))
    return r


def _ref_mlr(p):
    rows, fi, fwm, C = p["rows"], p["fi"], p["fwm"], p["C"]
    n, F = rows.n, rows.F
    coef = np.asarray(p["coef"], dtype=LD)
    W = coef[:C * F].reshape(F, C)                   # linear(c, f) = coef[f C + c]
    w = np.ones(n, dtype=LD) if p["w"] is None else np.asarray(p["w"], dtype=LD)
    wf = w.astype(np.float64)[:, None]
    sm = None if p["sm"] is None else np.asarray(p["sm"], dtype=LD)
    a = lambda v: np.abs(v).astype(np.float64)
    off, offabs = np.zeros(C, dtype=LD), np.zeros(C)
    if fi:
        off = coef[C * F:]
        if fwm:
            offabs = a(off) + a(sm) @ a(W)
            off = off - sm @ W
    T = rows.dot(W) + off
    A = a(off)[None, :] + rows.absdot(a(W))
    dT = gamma(rows.L + 2)[:, None] * A + float(gamma(F + 2)) * offabs[None, :]
    mx = T.max(axis=1, keepdims=True)
    dT = dT + U * (a(T) + a(mx))
    D = dT.max(axis=1, keepdims=True)
    E = np.exp(T - mx)
    P = E / E.sum(axis=1, keepdims=True)
    Y = np.zeros((n, C))
    yi = np.asarray(p["y"]).astype(np.int64)
    Y[np.arange(n), yi] = 1.0
    pos = (w > 0)[:, None]
    M = np.where(pos, w[:, None] * (P - Y), LD(0))
    dM = wf * (0.25 * (dT + D) + (8 * U + float(gamma(C))) * a(P) + 8 * U * Y)
    lp = np.log(P[np.arange(n), yi])
    ell = np.where(pos[:, 0], -w * lp, LD(0))
    dl = wf[:, 0] * (2 * D[:, 0] + float(gamma(C)) + 8 * U * (1 + a(lp)))
    G = rows.tdot(M)
    Gb = rows.abstdot(dM) + gamma(rows.ncol + 2)[:, None] * rows.abstdot(M)
    gn = float(gamma(n + 2))
    ms, dms, mabs = M.sum(axis=0), dM.sum(axis=0), a(M).sum(axis=0)
    tail, tailb = np.zeros(0, dtype=LD), np.zeros(0)
    if fi:
        if fwm:
            G = G - sm[:, None] * ms[None, :]
            Gb = Gb + a(sm)[:, None] * (dms + gn * mabs)[None, :]
        tail, tailb = ms, dms + gn * mabs
    r = Ref()
    r.grad = np.concatenate([G.ravel(), tail])
    r.gbound = np.concatenate([Gb.ravel(), tailb])
    r.loss, r.lbound = ell.sum(), float(dl.sum()) + gn * float(a(ell).sum())
    r.weight, r.wbound = w.sum(), float(gamma(n)) * float(w.sum())
    r.kink = np.inf
    return r


def oracle_add(p, st=None):
    """oracle.*_add of problem p: the formulas in host double arithmetic."""
    kind, rows = p["kind"], p["rows"]
    st = st or dict(grad=np.zeros(np.asarray(p["coef"]).size), loss=0.0, weight=0.0)
    if kind == "ls":
        st["grad"] = st["grad"][:rows.F]
    blk = rows.oracle_block(np.asarray(p["y"], dtype=np.float64), p["w"])
    if kind == "log":
        oracle.binary_logistic_add(blk, p["coef"], p["fi"], p["fwm"], p["sm"], st)
    elif kind == "hinge":
        oracle.hinge_add(blk, p["coef"], p["fi"], p["sm"], st)
    elif kind == "ls":
        oracle.least_squares_add(blk, p["coef"], p["inv"], p["fi"], p["ystd"], p["ymean"],
                                 p["sm"], st)
    elif kind == "huber":
        oracle.huber_add(blk, p["coef"], p["fi"], p["eps"], p["sm"], st)
    elif kind == "aft":
        oracle.aft_add(blk, p["coef"], p["fi"], p["sm"], st)
    else:
        oracle.multinomial_logistic_add(blk, p["coef"], p["C"], p["fi"], p["fwm"], p["sm"], st)
    return np.concatenate([st["grad"], [st["loss"], st["weight"]]])


# ------------------------------------------------------------ problems


def _csr(rng, n, F, k, exact, full_row=None, lead0=False):
    """n rows of at most k distinct sorted columns each; every 97th row empty;
    row `full_row` holds all F columns; lead0: every fifth row starts with
    column 0 (the exact hinge problems put its kink value there)."""
    c = rng.integers(0, F, size=(n, k))
    if lead0:
        c[::5, 0] = 0
    c.sort(axis=1)
    keep = np.ones((n, k), dtype=bool)
    keep[:, 1:] = c[:, 1:] != c[:, :-1]
    drop = rng.random((n, k)) < 0.2
    if lead0:
        drop[::5, 0] = False
    keep &= ~drop
    if n > 97:
        keep[96::97] = False
    cnt = keep.sum(axis=1)
    ci = c[keep].astype(np.int32)
    draw = (lambda m: rng.integers(-3, 4, size=m).astype(np.float64)) if exact else \
        (lambda m: rng.uniform(-1, 1, size=m))
    vv = draw(ci.size)
    rp = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    if full_row is not None:
        r0, r1 = int(rp[full_row]), int(rp[full_row + 1])
        ci = np.concatenate([ci[:r0], np.arange(F, dtype=np.int32), ci[r1:]])
        vv = np.concatenate([vv[:r0], draw(F), vv[r1:]])
        rp[full_row + 1:] += F - (r1 - r0)
    return rp, ci, vv


def _problem(kind, n, F, seed, mode=ROUNDED, nnz=None, fi=True, fwm=True, C=None,
             full_row=None, weights="mixed", colscale=None):
    """One block and one model.  nnz: None for dense rows, else at most that
    many nonzeros per CSR row.  weights: "mixed" (every 7th zero), "zero",
    "one" (all but row n // 2 zero), None (unit).  colscale: per-column
    factors for the features, the coefficients scaled inversely."""
    rng = np.random.default_rng(seed)
    exact = mode == EXACT
    fwm = fwm and fi
    if nnz is None:
        X = rng.integers(-3, 4, size=(n, F)).astype(np.float64) if exact else \
            rng.normal(size=(n, F))
        rows_csr = None
        avg = F
    else:
        rows_csr = _csr(rng, n, F, nnz, exact, full_row, lead0=exact)
        X = None
        avg = max(1, min(nnz, F))
    p = dict(kind=kind, fi=fi, fwm=fwm, C=C, sm=None, inv=None, ystd=1.0, ymean=0.0, eps=1.35,
             mode=mode, n=n, F=F)
    cls = C or 2
    if exact:
        coef = rng.integers(-2, 3, size=F * (C or 1)).astype(np.float64)
        coef[0] = 1.0
        icpt = rng.integers(-2, 3, size=C or 1).astype(np.float64)
        sm = rng.integers(-2, 3, size=F).astype(np.float64)
        w = rng.integers(0, 4, size=n).astype(np.float64)
    else:
        coef = rng.normal(size=F * (C or 1)) * ((0.1 if kind == "aft" else 1.0) / np.sqrt(avg))
        icpt = rng.normal(size=C or 1) * 0.3
        sm = rng.normal(size=F) * 0.1
        w = rng.uniform(0.1, 2.0, size=n)
        w[::7] = 0.0
    if colscale is not None:
        if X is not None:
            X = X * colscale[None, :]
        else:
            rows_csr = (rows_csr[0], rows_csr[1], rows_csr[2] * colscale[rows_csr[1]])
        coef = (coef.reshape(F, -1) / colscale[:, None]).ravel()
        sm = sm * colscale
    if weights == "zero":
        w[:] = 0.0
    elif weights == "one":
        keep = w[n // 2] if w[n // 2] > 0 else 1.0
        w[:] = 0.0
        w[n // 2] = keep
    elif weights is None:
        w = None
    centred = fi and (fwm if kind in ("log", "mlr") else True)
    p["sm"] = sm if centred else None
    if kind in ("log", "hinge", "mlr"):
        y = rng.integers(0, cls, size=n).astype(np.float64)
    elif kind == "aft":
        y = rng.exponential(2.0, size=n) + 1e-3
        w = (rng.uniform(size=n) < 0.6).astype(np.float64)
        if weights == "zero":
            w[:] = 0.0
    else:
        y = rng.integers(-5, 6, size=n).astype(np.float64) if exact else rng.normal(size=n) * 2
    tail = []
    if kind == "ls":
        p["inv"] = rng.uniform(0.5, 2.0, size=F)
        p["inv"][F // 2] = 0.0
        p["ystd"], p["ymean"] = (2.0, 3.0) if exact else (1.7, 0.3)
    elif kind == "mlr":
        tail = list(icpt) if fi else []
    elif kind == "aft":
        tail = [icpt[0] if fi else 0.0, 0.2]
    else:
        tail = [icpt[0]] if fi else []
        if kind == "huber":
            p["eps"] = 1.5 if exact else 1.35
            tail.append(2.0 if exact else 0.9)
    p["coef"] = np.concatenate([coef, tail])
    p["y"], p["w"] = y, w
    p["rows"] = Rows(X=X, csr=rows_csr, F=F)
    if exact and kind in ("hinge", "huber"):
        _put_on_kink(p)
    return p


def _put_on_kink(p):
    """Exact problems: every fifth row exactly on the branch switch -- hinge:
    column 0 (coefficient 1) set so that the margin is y'; Huber: the label
    set to margin +- sigma * eps = +- 3."""
    rows = p["rows"]
    t = ref_margin(p)
    idx = np.arange(0, rows.n, 5)
    if p["kind"] == "huber":
        p["y"][idx] = t[idx] + np.where(idx % 2 == 0, 3.0, -3.0)
        return
    ys = 2 * p["y"] - 1
    if rows.csr is None:
        rows.X[idx, 0] += ys[idx] - t[idx]
    else:
        rp, ci, vv = rows.csr
        idx = idx[(rp[idx + 1] > rp[idx])]
        idx = idx[ci[rp[idx]] == 0]
        vv[rp[idx]] += ys[idx] - t[idx]
    rows._xl = None


def ref_margin(p):
    """Margins of a hinge / Huber problem (float64 of the longdouble value)."""
    rows, F = p["rows"], p["rows"].F
    coef = np.asarray(p["coef"], dtype=LD)
    off = LD(0)
    if p["fi"]:
        off = coef[F] - (coef[:F] * np.asarray(p["sm"], dtype=LD)).sum()
    return (off + rows.dot(coef[:F])).astype(np.float64)


def _finish(p):
    """Reference of p with the conditions the comparison rests on, checked on
    the CPU: exact problems stay integer-valued far below 2^53, rounded hinge
    and Huber problems keep every counted margin 1e-9 from the kink."""
    r = ref_add(p)
    if p["mode"] == EXACT:
        assert p["kind"] in EXACT_KINDS
        assert r.magnitude < 2.0 ** 50
        for v in (r.grad, np.array([r.loss, r.weight])):
            assert np.array_equal(v * 8, np.rint(v * 8))          # multiples of 1/8
    elif p["kind"] in ("hinge", "huber"):
        assert r.kink >= 1e-9, r.kink
    return r


def _compare(group, state, p, r, what=""):
    """Device state [grad | loss | weight] against the reference r."""
    state = np.asarray(state)
    dim = r.grad.size
    assert state.size == dim + 2
    tag = f"{group} {p['kind']} n={p['n']} F={p['F']} C={p['C']} {what}"
    assert np.all(np.isfinite(state)), tag
    ref = np.concatenate([r.grad, [r.loss, r.weight]])
    if p["mode"] == EXACT:
        bad = np.flatnonzero(state != ref.astype(np.float64))
        assert bad.size == 0, f"{tag}: entries {bad[:8]} of {dim} + 2 differ: " \
                              f"{state[bad[:8]]} vs {ref[bad[:8]].astype(np.float64)}"
        return 0.0
    bound = np.concatenate([r.gbound, [r.lbound, r.wbound]])
    err = np.abs(state.astype(LD) - ref).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / bound)
    worst = int(np.argmax(ratio))
    RATIOS[group] = max(RATIOS.get(group, 0.0), float(ratio[worst]))
    assert ratio[worst] <= 1.0, \
        f"{tag}: entry {worst} of {dim} + 2: got {state[worst]!r}, reference " \
        f"{float(ref[worst])!r}, error {err[worst]:.3e} over bound {bound[worst]:.3e} = " \
        f"{ratio[worst]:.3g}"
    return float(ratio[worst])


# ------------------------------------------------------------ CPU tests


@pytest.mark.parametrize("kind", BIN + ("mlr",))
@pytest.mark.parametrize("n,F,nnz", [(1, 3, None), (257, 17, None), (300, 70, None),
                                     (1, 1, 1), (400, 5, 4), (500, 300, 8)])
def test_reference_vs_oracle(kind, n, F, nnz):
    """The longdouble restatement against oracle.*_add (the same formulas in
    host double arithmetic, sequential sums): every entry within the bound."""
    for fi, fwm in ((True, True), (True, False), (False, False)):
        p = _problem(kind, n, F, 100 + n + F, nnz=nnz, fi=fi, fwm=fwm,
                     C=5 if kind == "mlr" else None, full_row=n // 3 if nnz and n > 3 else None)
        _compare("reference vs oracle", oracle_add(p), p, _finish(p), f"fi={fi} fwm={fwm}")


@pytest.mark.parametrize("kind", EXACT_KINDS)
@pytest.mark.parametrize("n,F,nnz", [(1, 3, None), (257, 65, None), (300, 2048, None),
                                     (9, 1, 4), (700, 5, 4), (2049, 4097, 8)])
def test_exact_problems_are_exact(kind, n, F, nnz):
    """The integer problems: the oracle (fp64, sequential) gives the
    reference's bits, the kink rows sit exactly on the kink, and _finish's
    magnitude condition holds at the largest shapes the device tests use."""
    for fi in (True, False):
        p = _problem(kind, n, F, 7 + n + F, mode=EXACT, nnz=nnz, fi=fi,
                     full_row=n // 3 if nnz and n > 3 else None)
        _compare("exact", oracle_add(p), p, _finish(p), f"fi={fi}")
        if kind == "ls":
            continue
        t, rows = ref_margin(p), p["rows"]
        on = np.arange(0, n, 5)
        if rows.csr is not None:
            rp, ci, _ = rows.csr
            on = on[rp[on + 1] > rp[on]]
            on = on[ci[rp[on]] == 0]
        assert on.size > 0 or n < 5
        if kind == "hinge":
            assert np.all(1.0 - (2 * p["y"][on] - 1) * t[on] == 0.0)
        else:
            assert np.all(np.abs(p["y"][on] - t[on]) == 3.0)


def test_rounded_problems_keep_off_the_kink():
    """_finish asserts the 1e-9 distance for every rounded hinge and Huber
    problem; here at the shapes of the device tests, without a device."""
    for kind in ("hinge", "huber"):
        for n, F, nnz in [(4097, 65, None), (4097, 2048, None), (16385, 300, 8), (2049, 4097, 8)]:
            r = _finish(_problem(kind, n, F, n + F, nnz=nnz))
            assert np.isfinite(r.kink) and r.kink >= 1e-9


# ------------------------------------------------------------ device side


def _aggregator(p, cuda, coef=None, sm=None):
    from cycloneml_amd import optim as O
    F, kind = p["F"], p["kind"]
    coef = p["coef"] if coef is None else coef
    sm = p["sm"] if sm is None else sm
    ones = np.ones(F)
    if kind == "log":
        return O.BinaryLogisticBlockAggregator(ones, sm, p["fi"], p["fwm"], coef, device=cuda)
    if kind == "hinge":
        return O.HingeBlockAggregator(ones, sm, p["fi"], coef, device=cuda)
    if kind == "ls":
        return O.LeastSquaresBlockAggregator(p["inv"], sm, p["fi"], p["ystd"], p["ymean"], coef,
                                             device=cuda)
    if kind == "huber":
        return O.HuberBlockAggregator(ones, sm, p["fi"], p["eps"], coef, device=cuda)
    if kind == "aft":
        return O.AFTBlockAggregator(sm, p["fi"], coef, device=cuda)
    return O.MultinomialLogisticBlockAggregator(ones, sm, p["fi"], p["fwm"], coef, device=cuda)


def _layouts(p):
    if p["rows"].csr is None:
        return ("dense",)
    return ("csr",) if p["kind"] == "mlr" else ("csr", "csc", "wide", "compact")


def _prepare(blk, layout):
    if layout == "csc":
        blk.prepare()
    elif layout in ("wide", "compact"):
        blk.prepare(layout="tiles", tiles_format=layout).release_csr()
        assert blk.tiles.format == layout
    return blk


def _block(p, cuda, layout):
    from cycloneml_amd.optim import DeviceInstanceBlock
    rows = p["rows"]
    if rows.csr is None:
        return DeviceInstanceBlock.from_numpy(p["y"], p["w"], X=rows.X, device=cuda)
    return _prepare(DeviceInstanceBlock.from_numpy(p["y"], p["w"], csr=rows.csr,
                                                   numFeatures=rows.F, device=cuda), layout)


def _state(p, cuda, layout):
    return _aggregator(p, cuda).add(_block(p, cuda, layout))._state.cpu().numpy()


def _run(group, p, cuda, layouts=None, twice=False):
    r = _finish(p)
    for layout in layouts or _layouts(p):
        st = _state(p, cuda, layout)
        _compare(group, st, p, r, layout)
        if twice:
            assert np.array_equal(st, _state(p, cuda, layout)), f"{group} {layout}: not the same bits"
    return r


# ------------------------------------------------------------ dense binary family

DENSE_F = [1, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2047, 2048]
DENSE_F_ALL = {64, 65, 129, 257, 513, 1025, 2048}      # every kind here, logistic elsewhere


@pytest.mark.gpu
@pytest.mark.parametrize("F", DENSE_F)
def test_dense_binary_features(cuda, F):
    """k_binlog_dense<FPL> for FPL 1, 2, 4, 8, 16, 32 on both sides of each
    switch, n = 4097: two rows per wave, a last wave of one row, three idle
    waves whose zero partials the fold reads."""
    n = 4097
    for kind in (BIN if F in DENSE_F_ALL else ("log",)):
        _run("dense binary", _problem(kind, n, F, F), cuda)
        if kind in EXACT_KINDS:
            _run("dense binary", _problem(kind, n, F, F + 1, mode=EXACT), cuda)
    _run("dense binary", _problem("log", n, F, F + 2, fi=False, weights=None), cuda)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [4095, 4096, 4097, 8193, 12289])
@pytest.mark.parametrize("F", [65, 300])
def test_dense_binary_rows(cuda, n, F):
    """Rows per wave 1, 2, 3, 4 around the 4096-wave switch."""
    _run("dense binary", _problem("log", n, F, n + F, fwm=False), cuda)
    _run("dense binary", _problem("hinge", n, F, n + F + 1, mode=EXACT), cuda)
    _run("dense binary", _problem("huber", n, F, n + F + 2, mode=EXACT, fi=False), cuda)


@pytest.mark.gpu
def test_dense_binary_refuses_2049_features(cuda):
    from cycloneml_amd import _native as N
    p = _problem("log", 3, 2049, 1)
    with pytest.raises(N.CycloneError, match="supports numFeatures <= 2048"):
        _state(p, cuda, "dense")


# ------------------------------------------------------------ CSR paths


@pytest.mark.gpu
@pytest.mark.parametrize("n", [16384, 16385, 40000])
def test_csr_atomics(cuda, n):
    """k_binlog_csr: one, two and three rows per wave, empty rows, one row of
    all F columns (five 64-nonzero rounds of its wave).  The order of the
    atomic adds varies; the bound does not depend on order."""
    F = 300
    for kind in (BIN if n == 16385 else ("log",)):
        _run("csr atomics", _problem(kind, n, F, n, nnz=8, full_row=n // 2), cuda, ("csr",))
    for kind in EXACT_KINDS if n == 16385 else ("hinge",):
        _run("csr atomics", _problem(kind, n, F, n + 1, mode=EXACT, nnz=8, full_row=n // 2), cuda,
             ("csr",))


CSC_SHAPES = [(n, 5) for n in (1, 7, 8, 9, 63, 64, 65, 2 ** 18, 2 ** 18 + 1, 8192 * 64 + 1)] + \
             [(n, F) for F in (1, 300) for n in (9, 65, 2 ** 18 + 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,F", CSC_SHAPES)
def test_csr_csc_path(cuda, n, F):
    """k_binlog_csr_mult8 (64-row groups, 8 lanes per row, a second group per
    wave past 8192 * 64 rows) and k_binlog_csc_grad_blk over one, two and
    three row blocks of 2^18 rows (the first overwrites, the others add);
    bitwise reproducible."""
    full = n // 2 if n > 3 else None
    _run("csr + csc", _problem("log", n, F, n + F, nnz=4, full_row=full), cuda, ("csc",),
         twice=True)
    _run("csr + csc", _problem("hinge", n, F, n + F + 1, mode=EXACT, nnz=4, full_row=full), cuda,
         ("csc",), twice=True)


TILE_SHAPES = [(2047, 2047), (2048, 2048), (2049, 2049), (16385, 4097), (2047, 4097),
               (2049, 2047), (16385, 2048), (2048, 2049)]


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["wide", "compact"])
@pytest.mark.parametrize("n,F", TILE_SHAPES)
def test_tiles(cuda, fmt, n, F):
    """The row-block x column-chunk layout at one row block and one column
    chunk of 2048, one past, and several of each, in both entry formats."""
    _run("tiles", _problem("log", n, F, n + F, nnz=8, full_row=n // 2), cuda, (fmt,), twice=True)
    for kind in EXACT_KINDS:
        _run("tiles", _problem(kind, n, F, n + F + 1, mode=EXACT, nnz=8, full_row=n // 2), cuda,
             (fmt,))
    _run("tiles", _problem("aft", n, F, n + F + 2, nnz=8), cuda, (fmt,))


# ------------------------------------------------------------ multinomial

MLR_C = [2, 4, 5, 16, 17, 20, 21, 32, 36, 37, 48, 52, 53, 64, 68, 69, 80, 84, 85, 96, 100, 101,
         112, 116, 117, 127, 128]
MLR_F = [1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 48, 255, 256, 257, 513]
MLR_N = [1, 31, 32, 33, 255, 256, 257, 65537, 66000]
_FIT = [(True, True), (True, False), (False, False)]


@pytest.mark.gpu
@pytest.mark.parametrize("C", MLR_C)
def test_multinomial_dense_classes(cuda, C):
    """k_mlr_margins<CT> and k_mlr_grad<CT, T4> for CT 1..8 with the last
    class tile full, on the 4x4x4 form (1..4 classes) and one past it."""
    fi, fwm = _FIT[C % 3]
    _run("dense multinomial", _problem("mlr", 300, 33, C, C=C, fi=fi, fwm=fwm), cuda)


@pytest.mark.gpu
@pytest.mark.parametrize("C", [37, 100])
@pytest.mark.parametrize("F", MLR_F)
def test_multinomial_dense_features(cuda, F, C):
    """The feature tail (whole 4-feature loads or per-element ones), odd and
    even counts of 16-feature chunks, one, two and three 256-feature tiles of
    the gradient GEMM."""
    fi, fwm = _FIT[F % 3]
    _run("dense multinomial", _problem("mlr", 301, F, F + C, C=C, fi=fi, fwm=fwm), cuda)


@pytest.mark.gpu
@pytest.mark.parametrize("F,C", [(17, 53), (40, 96)])
@pytest.mark.parametrize("n", MLR_N)
def test_multinomial_dense_rows(cuda, n, F, C):
    """Row tails of the 32-row wave tiles and the 256-row workgroup tiles; past
    65,536 rows a workgroup takes a second tile."""
    fi, fwm = _FIT[n % 3]
    _run("dense multinomial", _problem("mlr", n, F, n + C, C=C, fi=fi, fwm=fwm), cuda)


@pytest.mark.gpu
def test_multinomial_dense_refuses_129_classes(cuda):
    from cycloneml_amd import _native as N
    with pytest.raises(N.CycloneError, match="numClasses <= 128"):
        _state(_problem("mlr", 5, 3, 1, C=129), cuda, "dense")


MLR_CSR = [(C, 20) for C in (2, 16, 17, 128, 129, 1000, 1024)] + \
          [(C, F) for C in (17, 129) for F in (1, 300)] + [(1024, 300)] + \
          [(C, 20) for C in (64, 65, 256, 257, 512, 513)]     # the CQ 1/2/4/8/16 switches


@pytest.mark.gpu
@pytest.mark.parametrize("C,F", MLR_CSR)
def test_multinomial_csr(cuda, C, F):
    """k_mlr_csr_margins<CQ> / k_mlr_csc_grad<CQ>: classes per lane 1, 2, 4, 8,
    16 on both sides of every switch (64, 128, 256, 512 classes)."""
    fi, fwm = _FIT[(C + F) % 3]
    _run("csr multinomial", _problem("mlr", 600, F, C + F, C=C, nnz=6, fi=fi, fwm=fwm,
                                     full_row=300), cuda)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [8193, 2 ** 18 + 1])
def test_multinomial_csr_rows(cuda, n):
    """More rows than the 8192 waves (a second row per wave) and a second
    2^18-row block of the CSC copy."""
    _run("csr multinomial", _problem("mlr", n, 5, n, C=3, nnz=3, full_row=n // 2), cuda)


@pytest.mark.gpu
def test_multinomial_csr_refuses_1025_classes(cuda):
    from cycloneml_amd import _native as N
    with pytest.raises(N.CycloneError, match="numClasses <= 1024"):
        _state(_problem("mlr", 5, 3, 1, C=1025, nnz=2), cuda, "csr")


# ------------------------------------------------------------ properties

KINDS6 = BIN + ("mlr",)


def _property_problems(kind, seed, mode=ROUNDED, **kw):
    """One dense and one CSR problem of the kind (every layout it accepts)."""
    C = 7 if kind == "mlr" else None
    return [_problem(kind, 700, 70, seed, mode=mode, C=C, **kw),
            _problem(kind, 2100, 130, seed + 1, mode=mode, nnz=6, C=C, full_row=1000, **kw)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS6)
def test_second_add_accumulates(cuda, kind):
    """Two different blocks into one aggregator: grad[f] + s, *lossSum += and
    *weightSum += from a nonzero state.  Equals the sum of the references
    within the sum of the bounds plus 2u per entry; exactly in integers."""
    for mode in (ROUNDED,) + ((EXACT,) if kind in EXACT_KINDS else ()):
        for p in _property_problems(kind, 11, mode):
            q = dict(p)                                        # same model, other rows
            o = _problem(kind, p["n"] + 37, p["F"], 99, mode=mode, C=p["C"],
                         nnz=None if p["rows"].csr is None else 6)
            q.update(rows=o["rows"], y=o["y"], w=o["w"], n=o["n"])
            if mode == EXACT and kind in ("hinge", "huber"):
                _put_on_kink(q)
            r1, r2 = _finish(p), _finish(q)
            r = Ref()
            r.grad, r.loss, r.weight = r1.grad + r2.grad, r1.loss + r2.loss, r1.weight + r2.weight
            r.gbound = r1.gbound + r2.gbound + 2 * U * np.abs(r.grad).astype(np.float64)
            r.lbound = r1.lbound + r2.lbound + 2 * U * abs(float(r.loss))
            r.wbound = r1.wbound + r2.wbound + 2 * U * abs(float(r.weight))
            for layout in _layouts(p):
                agg = _aggregator(p, cuda)
                agg.add(_block(p, cuda, layout)).add(_block(q, cuda, layout))
                _compare("second add", agg._state.cpu().numpy(), p, r, layout)


def _poisoned(arr, cuda, pad=64, after=None):
    """(view, tight copy) of arr on the device; the view lies inside a larger
    buffer whose surroundings are NaN (integers: `after`, 0 in front)."""
    import torch
    a = np.ascontiguousarray(arr)
    flat = torch.as_tensor(a.ravel(), device=cuda)
    if a.dtype == np.float64:
        big = torch.full((flat.numel() + 2 * pad,), float("nan"), dtype=flat.dtype, device=cuda)
    else:
        big = torch.zeros(flat.numel() + 2 * pad, dtype=flat.dtype, device=cuda)
        big[flat.numel() + pad:] = after
    big[pad:pad + flat.numel()] = flat
    return big[pad:pad + flat.numel()].view(a.shape), flat.clone().view(a.shape)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS6)
def test_poisoned_surroundings(cuda, kind):
    """X, labels, weights, the CSR arrays, coefficients and scaledMean as
    contiguous views into larger buffers that hold NaN in front and behind
    (rowptr: offsets that lead into the NaN behind the values, column 0): the
    same bits as with tightly allocated copies (the F atomically added
    gradient entries of the plain CSR path: both within the bound).  Rows past
    n read as zero, k_mlr_margins' padding classes and the tail loads stay
    inside."""
    from cycloneml_amd.optim import DeviceInstanceBlock
    shapes = [(333, 67, None), (1001, 129, 6)] if kind != "mlr" else [(333, 67, None), (601, 37, 6)]
    for n, F, nnz in shapes:
        p = _problem(kind, n, F, 5 + n, nnz=nnz, C=21 if kind == "mlr" else None)
        rows = p["rows"]
        y, w = _poisoned(p["y"], cuda), _poisoned(p["w"], cuda)
        coef, sm = _poisoned(p["coef"], cuda), _poisoned(p["sm"], cuda)
        if rows.csr is None:
            X = _poisoned(rows.X, cuda)
        else:
            rp = _poisoned(rows.csr[0], cuda, after=int(rows.csr[0][-1]) + 32)
            ci = _poisoned(rows.csr[1], cuda, after=0)
            vv = _poisoned(rows.csr[2], cuda)
        for layout in _layouts(p):
            st = []
            for k in (0, 1):
                if rows.csr is None:
                    blk = DeviceInstanceBlock(y[k], w[k], X=X[k])
                else:
                    blk = _prepare(DeviceInstanceBlock(y[k], w[k], rowptr=rp[k], colidx=ci[k],
                                                       values=vv[k], numFeatures=F), layout)
                st.append(_aggregator(p, cuda, coef[k], sm[k]).add(blk)._state.cpu().numpy())
            assert np.all(np.isfinite(st[0])), f"{kind} {layout}: NaN read from the surroundings"
            if layout == "csr" and kind != "mlr":
                # k_binlog_csr adds the gradient with atomics in no fixed order:
                # both within the bound, everything past the F entries the same bits
                r = _finish(p)
                for s_ in st:
                    _compare("poisoned surroundings", s_, p, r, layout)
                st = [s_[F:] for s_ in st]
            assert np.array_equal(st[0], st[1]), f"{kind} {layout}: views and copies differ"


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS6)
def test_mixed_column_scales(cuda, kind):
    """Feature columns scaled by 10^-6 .. 10^6, coefficients inversely, so the
    margins stay of order 1 and the gradient spans twelve decades: every
    entry within its own bound."""
    for p0 in _property_problems(kind, 21):
        F = p0["F"]
        scale = 10.0 ** np.random.default_rng(F).uniform(-6, 6, size=F)
        p = _problem(kind, p0["n"], F, 21 + F, C=p0["C"], colscale=scale,
                     nnz=None if p0["rows"].csr is None else 6)
        r = _run("mixed column scales", p, cuda)
        g = np.abs(r.grad[:F * (p["C"] or 1)].astype(np.float64))
        assert g.max() / g[g > 0].min() > 1e9


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS6)
@pytest.mark.parametrize("weights", ["zero", "one"])
def test_zero_weight_rows(cuda, kind, weights):
    """All weights zero, and all but one: zero-weight rows add nothing (AFT:
    the weights are the censors, every row still counts)."""
    for p in _property_problems(kind, 31, weights=weights):
        r = _run("zero weights", p, cuda)
        if weights == "zero" and kind != "aft":
            assert not r.grad.any() and r.loss == 0 and r.weight == 0
    if kind in EXACT_KINDS:
        for p in _property_problems(kind, 33, EXACT, weights=weights):
            _run("zero weights", p, cuda)


EXTREME = [0.0, 1e-300, 1.0, 18.0, 36.0, 37.0, 40.0, 708.0, 709.8, 710.0, 745.0, 746.0, 1e4]


@pytest.mark.gpu
def test_extreme_margins_binary_logistic(cuda):
    """One-row, one-feature blocks with margins +- EXTREME, both labels, dense
    and CSR: the log1p_exp branch switch, exp overflow and underflow.  Loss
    and gradient finite and equal to the longdouble reference within four
    times the error oracle.binary_logistic_add (the same formula in host
    double arithmetic) makes on the same row, at least 4u relative, or 2
    units of 2^-1074 where the value is subnormal.

    Measured on the MI355X: the largest relative error is 1.0 for the oracle
    and 1.0 for the device, in the gradient and in the loss alike -- the rows
    where the reference's own formula cancels in double arithmetic (label 1
    and a margin of 37 or more: sigmoid - 1 rounds to 0 where the value is
    -e^-m; label 0 and a margin of -37 or less: log1pExp(-m) + m rounds to 0
    likewise), on the host as on the device.  The device error is at most 0.5
    of the allowance on every row."""
    worst_o, worst_d, worst_a = np.zeros(2), np.zeros(2), 0.0
    for mag in EXTREME:
        for t in (mag, -mag):
            for y in (0.0, 1.0):
                for nnz in (None, 1):
                    rows = Rows(X=np.ones((1, 1))) if nnz is None else \
                        Rows(csr=(np.array([0, 1]), np.array([0], dtype=np.int32), np.ones(1)), F=1)
                    p = dict(kind="log", rows=rows, y=np.array([y]), w=None, coef=np.array([t]),
                             fi=False, fwm=False, sm=None, C=None, mode=ROUNDED, n=1, F=1)
                    r = ref_add(p)
                    ref = np.array([r.grad[0], r.loss], dtype=LD)
                    o = oracle_add(p)[:2]
                    d = _state(p, cuda, "dense" if nnz is None else "csr")
                    assert np.all(np.isfinite(d)) and d[2] == 1.0, (t, y, d)
                    eo = np.abs(o.astype(LD) - ref).astype(np.float64)
                    ed = np.abs(d[:2].astype(LD) - ref).astype(np.float64)
                    absref = np.abs(ref).astype(np.float64)
                    floor = np.where(absref < np.finfo(np.float64).tiny, 2 * 2.0 ** -1074,
                                     4 * U * absref)
                    allow = np.maximum(4 * eo, floor)
                    rel = np.maximum(absref, np.finfo(np.float64).tiny)
                    worst_o, worst_d = np.maximum(worst_o, eo / rel), np.maximum(worst_d, ed / rel)
                    worst_a = max(worst_a, float((ed / allow).max()))
                    assert np.all(ed <= allow), \
                        f"margin {t!r} label {y} {'dense' if nnz is None else 'csr'}: device " \
                        f"(grad, loss) {d[:2]!r}, reference {ref.astype(np.float64)!r}, device " \
                        f"error {ed!r}, oracle error {eo!r}, allowed {allow!r}"
    for i, what in enumerate(("gradient", "loss")):
        RATIOS[f"extreme margins: oracle rel. error, {what}"] = float(worst_o[i])
        RATIOS[f"extreme margins: device rel. error, {what}"] = float(worst_d[i])
    RATIOS["extreme margins: device error / allowed"] = worst_a


@pytest.mark.gpu
def test_aft_extreme_exponents(cuda):
    """One row with exp(e) near 1e300 and one near 1e-300 among ordinary
    rows: the state stays finite and within the bound."""
    for nnz in (None, 6):
        p = _problem("aft", 500, 40, 77, nnz=nnz)
        F = p["F"]
        p["coef"][F + 1] = -1.0                                # sigma = 0.37: labels stay finite
        sigma = float(np.exp(LD(p["coef"][F + 1])))
        t = ref_margin(p)
        for row, target in ((3, 690.0), (4, -690.0)):          # e = (log y - t) / sigma
            p["y"][row] = float(np.exp(LD(t[row]) + LD(target) * LD(sigma)))
        r = _run("aft extremes", p, cuda)
        assert np.isfinite(float(r.loss)) and float(np.abs(r.grad).max()) > 1e290


def test_report_error_ratios():
    """Not a check: prints the largest err / bound per group (pytest -rP)."""
    for k in sorted(RATIOS):
        print(f"{k:40s} {RATIOS[k]:.3g}")
