"""GPU: whole runs of small synthetic chromosomes with the keyed form of the NB transform and its quantile chains (the default) and
with the chain of launches (RSI_HOT_NB_KEYED=0), in fresh contexts: every array the rsi_hot_fetch_* calls return, the statistics
block and the rows are equal, and the kernel table shows that each run took the form it was asked for."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FETCH = ("rd_gc", "rd_concat", "binmedint", "binsum", "binnb", "status1", "status1f", "status2")
KEYED = {"nb_keys", "nb_apply", "nb_keys_masked"}
CHAIN = {"hist_walk", "minmax_plan", "nb_raw", "nb_scale"}
CASES = {
    "events": (dict(n=3_000_000, seed=0x6B31, model=1, n_events=7, gaps=1, max_len=40000, end_n=5000, gap_len=20000), {}),
    "no_events": (dict(n=2_000_000, seed=0x6B32, model=1, n_events=0, gaps=1, end_n=5000, gap_len=20000), {}),
    "cap4_m51": (dict(n=4_000_000, seed=0x6B33, model=1, n_events=9, gaps=2, max_len=60000, end_n=8000, gap_len=30000), dict(cap=4.0, m=51)),
}


def one_run(api, depth, fasta, kw):
    hot = api.RsiHot(0)
    try:
        hot.set_timing(1)        # rsi_hot_kernel_times names what ran
        res = hot.run(api.make_params(**kw), depth, fasta)
        arrays = {name: hot.fetch(name) for name in FETCH}
        stats = {k: v for k, v in res.stats.items() if not k.startswith("t_")}
        return dict(arrays=arrays, stats=stats, rows=res.rows, lists={w: repr(res.calls(w)) for w in ("calls", "calls_raw", "segs", "blocks")},
                    kernels={k for k, _ in hot.kernel_times()}, phases=dict(hot.phase_times()))
    finally:
        hot.close()


@pytest.mark.parametrize("name", sorted(CASES))
def test_keyed_run_equals_chain_run(hotlib, monkeypatch, name):
    from rsicnv_amd import api, synth
    plan_kw, kw = CASES[name]
    fasta, depth = synth.generate_host(hotlib, synth.make_plan(mean=30.0, **plan_kw))
    monkeypatch.delenv("RSI_HOT_NB_KEYED", raising=False)
    keyed = one_run(api, depth, fasta, kw)
    monkeypatch.setenv("RSI_HOT_NB_KEYED", "0")
    chain = one_run(api, depth, fasta, kw)
    print(name, "rows", len(keyed["rows"]), "nbins", keyed["stats"].get("nbins"), sorted(keyed["kernels"] & KEYED), sorted(chain["kernels"] & CHAIN))
    assert KEYED <= keyed["kernels"] and not (CHAIN & keyed["kernels"]), sorted(keyed["kernels"])
    assert CHAIN <= chain["kernels"] and not (KEYED & chain["kernels"]), sorted(chain["kernels"])
    assert keyed["phases"].get("nb.keyed") == 1.0 and "nb.keyed" not in chain["phases"] and "nb.keyed declined" not in keyed["phases"]
    for a in FETCH:
        x, y = keyed["arrays"][a], chain["arrays"][a]
        assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8)), a
    assert keyed["stats"] == chain["stats"]
    assert keyed["rows"] == chain["rows"]
    assert keyed["lists"] == chain["lists"]
    if name != "no_events":
        assert len(keyed["rows"]) >= 1
