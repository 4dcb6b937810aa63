"""GPU: the keyed form of the NB transform and its two quantile chains (rsi_hot_debug_nb_keyed: k_nb_keys, k_nb_apply, k_nb_keys with a
mask -- the functions a run calls) on every case of tests/nb_keyed_cases.py, with == against

  (a) the restatement "statistics from the histogram of the bin sums" (nb_keyed_cases.keyed), which tests/test_nb_keyed_cases.py
      pins to the array forms on the CPU.  The raw value of each distinct sum is the device's own (the chain's raw array): the
      device's log may differ from libm's in the last place on hard inputs (tests/nb_cases.py), and that is tests/test_nb_edges.py's
      subject, not this one's;
  (b) the chain of launches on the same inputs: rsi_hot_debug_nb_transform, then rsi_hot_debug_grid_median (mode 0) on its T, with
      and without the mask.

Compared: T, median, MAD, their counts, the two records' flags and bucket counts, the raw minimum."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nb_cases as nc          # noqa: E402
import nb_keyed_cases as kc    # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nb_edges.npz")


def bits(x):
    return np.asarray(x, dtype=np.float32).view(np.int32)


@pytest.fixture(scope="module")
def hot():
    from rsicnv_amd import api
    h = api.RsiHot(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def chain_hot():
    """The chain of launches runs on a context of its own: the keyed calls then follow one another on theirs."""
    from rsicnv_amd import api
    h = api.RsiHot(0)
    yield h
    h.close()


def chain(h, c):
    """(raw, T, raw minimum bits, out, info[0:4]) of the chain of launches."""
    raw, T, info = h.debug_nb_transform(c.binsum, c.m, c.binsum.size * c.m, c.RDmedian, c.r)
    out, ginfo = h.debug_grid_median(T, c.mask, "pair")
    return raw, T, int(info[0]), out, [int(v) for v in ginfo[:4]], int(ginfo[5])


def check(hot, chain_hot, c):
    from rsicnv_amd import api
    where = c.name
    if c.form == -1:
        T, out, info = hot.debug_nb_keyed(c.binsum, c.m, c.K, c.RDmedian, c.r, c.mask)
        assert int(info[5]) == -1 and not out.any() and not T.any(), where
        return None
    if c.name == "non_finite":
        with pytest.raises(api.RsiError, match="non-finite"):
            hot.debug_nb_keyed(c.binsum, c.m, c.K, c.RDmedian, c.r, c.mask)
        with pytest.raises(api.RsiError, match="non-finite"):
            chain(chain_hot, c)
        return None
    T, out, info = hot.debug_nb_keyed(c.binsum, c.m, c.K, c.RDmedian, c.r, c.mask)
    raw_c, T_c, tmin_c, out_c, rec_c, host_c = chain(chain_hot, c)
    print(where, "form", int(info[5]), "records", [int(v) for v in info[:4]], "out", list(out), "host-driven", int(info[6]))
    assert int(info[5]) == c.form, where
    # (b) the chain of launches
    assert np.array_equal(bits(T), bits(T_c)), f"{where}: T differs from the chain's at {np.nonzero(bits(T) != bits(T_c))[0][:8]}"
    assert int(info[4]) == tmin_c, where
    assert [int(v) for v in info[:4]] == rec_c, where
    assert list(out) == list(out_c), where
    assert int(info[6]) == host_c, where
    # (a) the restatement, over the device's raw values of the distinct sums
    k = kc.keyed(c.binsum, c.m, c.RDmedian, c.r, c.mask, raw_table={int(s): v for s, v in zip(c.binsum, raw_c)})
    assert np.array_equal(bits(T), bits(k.T)), where
    assert int(info[4]) == int(bits(k.tmin)), where
    assert tuple(int(v) for v in info[:2]) == k.records[:2], where
    if k.records[0] == 0:
        assert tuple(int(v) for v in info[2:4]) == k.records[2:], where
    assert (out[0], int(out[1]), out[2], int(out[3])) == tuple(k.out), where
    return k.records[0]


def test_every_case(hot, chain_hot):
    flags = set()
    for c in kc.all_cases():
        flags.add(check(hot, chain_hot, c))
    assert {0, kc.EMPTY, kc.DEGENERATE, kc.TOO_WIDE} <= flags


def test_stored_hard_inputs(hot, chain_hot):
    """Sums whose double lies next to a float midpoint: whatever the device's log makes of them, both forms make the same."""
    z = np.load(GOLDEN)
    hard = nc.hard_cases(z)
    assert len(hard) >= 1
    for c, _ in hard:
        K = int(c.binsum.max()) + 1
        form = 1 if K <= kc.KEY_LIMIT else -1                          # (a sum of the sweep beyond the table: the route says no)
        check(hot, chain_hot, kc.Case("hard_" + c.name, c.binsum, c.m, K, c.RDmedian, c.r, None, form))
        mk = np.zeros(c.binsum.size, dtype=np.int32)
        mk[4] = 1                                                      # the known minimum's bin
        check(hot, chain_hot, kc.Case("hard_masked_" + c.name, c.binsum, c.m, K, c.RDmedian, c.r, mk, form))


def test_state_left_for_the_next_user(hot, chain_hot, monkeypatch):
    """The hook twice in a row on one context with different inputs, a declined call and one the route refuses between them, then the
    chain of launches and a whole run of a small chromosome on the same context: each finds the shared state -- arrival counters, key
    counters, the min/max record, the raw-minimum word -- as it needs it."""
    from rsicnv_amd import api, synth
    by = {c.name: c for c in kc.all_cases()}
    for name in ("nb_4097", "mask_random", "declined", "k_at_limit", "nb_7_no_route", "mask_all", "nb_9", "declined_masked", "nb_1025"):
        check(hot, chain_hot, by[name])
    c = by["mask_moves_the_median"]
    assert chain(hot, c)[3].tolist() == chain(chain_hot, c)[3].tolist()      # the chain of launches behind the keyed calls, same context
    check(hot, chain_hot, by["nb_1024"])
    plan = synth.make_plan(n=400_000, seed=0x5310CE, model=1, n_events=5, gaps=1, max_len=20000, end_n=5000, gap_len=8000)
    fasta, depth = synth.generate_host(hot.lib, plan)
    res = hot.run(api.make_params(), depth, fasta)
    assert dict(hot.phase_times()).get("nb.keyed") == 1.0
    monkeypatch.setenv("RSI_HOT_NB_KEYED", "0")                               # the same chromosome through the chain of launches
    ref = chain_hot.run(api.make_params(), depth, fasta)
    assert "nb.keyed" not in dict(chain_hot.phase_times())
    monkeypatch.delenv("RSI_HOT_NB_KEYED")
    assert [(c["start"], c["end"], c["type"]) for c in res.calls("calls")] == [(c["start"], c["end"], c["type"]) for c in ref.calls("calls")]
    assert np.array_equal(hot.fetch("status2"), chain_hot.fetch("status2")) and np.array_equal(bits(hot.fetch("binnb")), bits(chain_hot.fetch("binnb")))
    check(hot, chain_hot, by["two_sums"])
