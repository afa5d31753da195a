"""The two forms of a Lloyd call's center preparation: the three fused
launches (centers_prepare_all, the default) against the separate launches
(CYC_KMEANS_PREP=0).  The fused form changes launches, not arithmetic, so
every output is compared bitwise (numpy.array_equal).

The switch is read once per process, so each form runs in a child process
(as test_kmeans_gpu.py::test_recheck_forms_identical does); ONE child per
form runs every case below and saves one .npz, shared by all tests here.

Shapes (k, d, n), chosen for the fused kernels' block-range arithmetic:
(1, 8, 300) no statistics pairs; (2, 3, 257); (37, 33, 4099) k no multiple
of 4 or 64, odd d; (130, 256, 8192) crosses a 128-center boundary, carried
bounds on; (1024, 256, 16384) the benchmark's center shape.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

SHAPES = [(1, 8, 300), (2, 3, 257), (37, 33, 4099), (130, 256, 8192), (1024, 256, 16384)]
ITERS = 4
NB = (37, 33, 4099)       # the call without bounds, and the require cases
NAN_CENTER_M = 5

# bench.kmeans_data-style rows (true centers N(0, 4^2), noise N(0, 1)), fixed
# seed; exec'd here and pasted into the child so both build the same rows
_DATA_SRC = r'''
def prep_data(k, d, n):
    import numpy as np
    rng = np.random.default_rng(1234 + 7 * k + d)
    true_c = rng.normal(scale=4.0, size=(k, d))
    return true_c[rng.integers(0, k, n)] + rng.normal(size=(n, d))
'''
exec(_DATA_SRC)

_CHILD = _DATA_SRC + r'''
import os, sys, numpy as np, torch
sys.path.insert(0, os.getcwd())
from cycloneml_amd.clustering import KMeansPlan, row_norms
dev = torch.device("cuda", 0)
shapes = eval(sys.argv[2]); iters = int(sys.argv[3]); nb = eval(sys.argv[4]); m = int(sys.argv[5])
out = {}

def lloyd(tag, k, d, n, bounds, iters):
    X = torch.as_tensor(prep_data(k, d, n), device=dev)
    C = X[:k].clone()
    xn, cn = row_norms(X), row_norms(C)
    p = KMeansPlan(d, k, n); rows = p.rows(X)
    rows.set_bounds(bounds)
    st = torch.empty(k * (k + 1) // 2, dtype=torch.float64, device=dev)
    p.stats(C, st)
    out[tag + "_stats"] = st.cpu().numpy()
    a = torch.empty(n, dtype=torch.int32, device=dev)
    conv = torch.zeros(1, dtype=torch.int32, device=dev)
    for it in range(iters):
        s = torch.zeros(k * d, dtype=torch.float64, device=dev)
        w = torch.zeros(k, dtype=torch.float64, device=dev)
        c = torch.zeros(1, dtype=torch.float64, device=dev)
        p.accumulate(X, xn, None, C, cn, s, w, c, a, None, rows=rows)
        p.update(C, cn, s, w, 1e-4, conv)
        for name, t in (("assign", a), ("sums", s), ("wsum", w), ("cost", c), ("centers", C),
                        ("cnorm", cn), ("conv", conv)):
            out[f"{tag}_{it}_{name}"] = t.cpu().numpy().copy()
    out[tag + "_bounds_calls"] = np.array(rows.bounds_info()[0])

for k, d, n in shapes:
    lloyd(f"s{k}", k, d, n, True, iters)
lloyd("nb", *nb, False, 1)

def failing(tag, Xh, Ch):
    k, d, n = nb
    X, C = torch.as_tensor(Xh, device=dev), torch.as_tensor(Ch, device=dev)
    p = KMeansPlan(d, k, n); rows = p.rows(X)
    try:
        p.accumulate(X, row_norms(X), None, C, row_norms(C),
                     torch.zeros(k * d, dtype=torch.float64, device=dev),
                     torch.zeros(k, dtype=torch.float64, device=dev),
                     torch.zeros(1, dtype=torch.float64, device=dev), rows=rows)
        out[tag] = np.array("no exception")
    except Exception as e:
        out[tag] = np.array(type(e).__name__ + "|" + str(e))

Xh = prep_data(*nb); Ch = Xh[:nb[0]].copy()
Cb = Ch.copy(); Cb[0, 2] = np.nan
failing("err_c0", Xh, Cb)
Cb = Ch.copy(); Cb[m, 1] = np.nan
failing("err_cm", Xh, Cb)
Xb = Xh.copy(); Xb[nb[0] + 7, 3] = np.nan
failing("err_row", Xb, Ch)
np.savez(sys.argv[1], **out)
'''


@pytest.fixture(scope="module")
def forms(cuda, tmp_path_factory):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_dir = tmp_path_factory.mktemp("prep_forms")
    res = {}
    for form in ("0", "1"):
        f = str(out_dir / f"prep_form_{form}.npz")
        env = dict(os.environ, CYC_KMEANS_PREP=form)
        r = subprocess.run([sys.executable, "-c", _CHILD, f, repr(SHAPES), str(ITERS), repr(NB),
                            str(NAN_CENTER_M)],
                           env=env, cwd=root, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        with np.load(f) as z:
            res[form] = {key: z[key] for key in z.files}
    assert res["0"].keys() == res["1"].keys()
    return res


@pytest.mark.parametrize("k,d,n", SHAPES)
def test_prep_forms_bitwise(forms, k, d, n):
    """Four Lloyd iterations (row image, bounds and incremental sums on, rows
    0..k-1 as centers): assignments, sums, weights, cost, centers, center
    norms and the converged flag of every iteration are bitwise equal between
    the separate launches and the fused form; so are the packed statistics,
    which also equal the oracle's."""
    tag = f"s{k}"
    keys = [key for key in forms["0"] if key.startswith(tag + "_")]
    assert len(keys) == 7 * ITERS + 2
    for key in keys:
        assert np.array_equal(forms["0"][key], forms["1"][key], equal_nan=True), key
    # carried bounds ran where the screen supports them (k > 96, d <= 256)
    assert int(forms["1"][tag + "_bounds_calls"]) == (ITERS if k > 96 else 0)
    ref = oracle.kmeans_stats(prep_data(k, d, n)[:k])
    for form in ("0", "1"):
        got = forms[form][tag + "_stats"]
        assert got.shape == ref.shape
        assert np.array_equal(got, ref, equal_nan=True), form


def test_prep_forms_no_bounds(forms):
    """One call with the bounds switched off (the null drift / neighbourhood
    jobs): both forms equal, and equal to the oracle's assignments."""
    for name in ("assign", "sums", "wsum", "cost", "centers", "cnorm", "conv"):
        key = f"nb_0_{name}"
        assert np.array_equal(forms["0"][key], forms["1"][key], equal_nan=True), key
    assert int(forms["1"]["nb_bounds_calls"]) == 0
    k, d, n = NB
    X = prep_data(k, d, n)
    C = X[:k].copy()
    xn, cn = oracle.row_norms(X), oracle.row_norms(C)
    a, *_ = oracle.kmeans_partition(X, xn, None, C, cn, oracle.kmeans_stats(C))
    for form in ("0", "1"):
        np.testing.assert_array_equal(forms[form]["nb_0_assign"], a)


@pytest.mark.parametrize("case,nan_side", [("err_c0", "norm1=NaN"), ("err_cm", "norm2=NaN"),
                                           ("err_row", "norm2=NaN")])
def test_prep_forms_require(forms, case, nan_side):
    """The require(norm1 >= 0.0 && norm2 >= 0.0) failure for a NaN center 0, a
    NaN center m > 0 and a NaN row norm: the fused form raises what the
    separate launches raise, text and exception class (= error code)."""
    m0, m1 = str(forms["0"][case]), str(forms["1"][case])
    assert m0 == m1
    cls, msg = m1.split("|", 1)
    assert cls == "IllegalArgumentException"
    assert msg.startswith("requirement failed: Both norms should be greater or equal to 0.0, "
                          "found norm1=")
    assert nan_side in msg
    assert msg.count("NaN") == 1
