"""CPU: the oracle's numeric utilities and a larger whole-path case against the compiled reference's own answers,
stored in tests/golden/oracle_vs_ref.npz (tools/make_golden_ref_checks.py writes it from oracle/_ref/libref.so).
Inputs are regenerated here from seeds; their hashes in the file guard against generator drift."""
import json

import numpy as np
import pytest

import golden_util as gu
import oracle
from conftest import calls_equal, make_case

WHOLE_PATH_FLAGS = [dict(), dict(m=51, trans=1), dict(gcadjust=0, cap=-1.0), dict(trans=2),
                    dict(epsilon=2.5, chklen=1.5, merge=0), dict(trans=1, threshold=0.8, maxchkbp=2000, m=75)]
WHOLE_PATH_IDS = ["nb", "med51", "nogc_nocap", "all", "eps_reflen_nomerge", "med_threshold_maxchkbp_m75"]


def quantile_inputs():
    """The arrays the histogram median / IQR are probed with, in the order the golden values are stored."""
    rng = np.random.default_rng(7)
    out = []
    for n in (1, 2, 3, 4, 5, 31, 100, 1001, 50_000):
        xi = rng.poisson(30, n).astype(np.int32)
        xf = (rng.gamma(9.0, 3.3, n)).astype(np.float32)
        xd = xf.astype(np.float64) * 1.37
        out.append((xi, xf, xd))
    return out


def exact_median_inputs():
    rng = np.random.default_rng(11)
    xs = [rng.integers(0, 60, n).astype(np.int32) for n in (1, 2, 3, 4, 7, 8, 99, 100, 196)]
    pn = np.concatenate([np.linspace(-16, 16, 1281), rng.normal(0, 4, 500)])
    return xs, pn


def whole_path_plan(flags):
    return dict(n=2_000_003, seed=0xD00D + len(flags), model=1, n_events=9, gaps=2, max_len=60000, end_n=10000, gap_len=30000)


def inputs_sha(arrays):
    return gu.sha(np.concatenate([np.ascontiguousarray(a).view(np.uint8).reshape(-1) for a in arrays]))


@pytest.fixture(scope="module")
def golden():
    return np.load(gu.GOLDEN_DIR + "/oracle_vs_ref.npz", allow_pickle=False)


def test_histogram_quantiles_match(golden, oracle_cls):
    O = oracle_cls()
    cases = quantile_inputs()
    assert inputs_sha([a for c in cases for a in c]) == str(golden["quantile_inputs_sha"]), "numpy's generator no longer gives the stored inputs"
    med, iqr = golden["median"], golden["iqr"]
    for k, (xi, xf, xd) in enumerate(cases):
        for j, x in enumerate((xi, xf, xd)):
            assert O.median(x) == med[3 * k + j]
        assert O.iqr(xi) == iqr[2 * k] and O.iqr(xf) == iqr[2 * k + 1]
    # degenerate: all equal / within the grid step -> the mean is returned
    c = np.full(17, 5, dtype=np.int32)
    assert O.median(c) == golden["median_const"] == 5.0
    f = (30.0 + 0.001 * np.arange(9)).astype(np.float32)
    assert O.median(f) == golden["median_grid"]


def test_exact_median_and_pnorm_match(golden, oracle_cls):
    O = oracle_cls()
    xs, pn = exact_median_inputs()
    assert inputs_sha(xs + [pn]) == str(golden["exact_inputs_sha"]), "numpy's generator no longer gives the stored inputs"
    for x, e in zip(xs, golden["exact_median"]):
        assert O.exact_median(x) == e == float(np.median(x))
    ref_pnorm = golden["pnorm"]
    assert ref_pnorm.shape == pn.shape
    for v, e in zip(pn, ref_pnorm):
        assert O.pnorm(float(v)) == e


@pytest.mark.parametrize("flags", WHOLE_PATH_FLAGS, ids=WHOLE_PATH_IDS)
def test_whole_path_2mb(golden, oracle_cls, hotlib, flags):
    case = WHOLE_PATH_IDS[WHOLE_PATH_FLAGS.index(flags)]
    g = {k[len(case) + 1:]: golden[k] for k in golden.files if k.startswith(case + "/")}
    assert json.loads(str(g["flags"])) == flags
    _, fasta, depth = make_case(hotlib, whole_path_plan(flags))
    assert gu.sha(fasta) == str(g["fasta_sha"]) and gu.sha(depth) == str(g["depth_sha"]), "synthetic inputs differ from the stored ones"
    p = oracle.make_params(**flags)
    O = oracle_cls()
    O.run(p, depth, fasta)
    assert np.array_equal(g["noncode"], O.i32("noncode"))
    if flags.get("gcadjust", 1):
        assert str(g["rd_gc_sha"]) == gu.sha(O.i32("rd_gc"))
    assert str(g["rd_cap_sha"]) == gu.sha(O.i32("rd_cap"))
    assert str(g["rd_concat_sha"]) == gu.sha(O.i32("rd_concat"))
    assert tuple(g["chrom"]) == tuple(O.f64("chrom")[:2])
    assert np.array_equal(g["binmedint"], O.i32("binmedint")) and np.array_equal(g["binnb"], O.f32("binnb")) and \
        np.array_equal(g["binmed"], O.f32("binmed"))
    trans = flags.get("trans", 0)
    for use_med in ([True] if trans == 1 else [False] if trans == 0 else [True, False]):
        pre = "med" if use_med else "nb"
        sc = g[f"{pre}_scan"]
        so = O.f64(f"scan_{pre}")
        assert tuple(sc[:6]) == tuple(so[:6])
        assert int(sc[7]) == int(so[7])
        for w in ("status1", "status1f", "status2"):
            assert np.array_equal(g[f"{pre}_{w}"], O.i32(f"{pre}_{w}"))
        ok, why = calls_equal(O.calls(f"segs_{pre}"), gu.calls_from_array(g[f"{pre}_segs"]), rtol=0)
        assert ok, why
    raw = gu.calls_from_array(g["calls_raw"])
    for which, exp in (("calls_raw", raw), ("calls", gu.calls_from_array(g["calls"]))):
        ok, why = calls_equal(O.calls(which), exp, rtol=0)
        assert ok, f"{which}: {why}"
    assert len(raw) >= 3
