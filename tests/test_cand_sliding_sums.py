"""The split candidate test's window sums by sliding differences (k_cand_sums, kernels_cand.hip): every chunk of windows sums
its first window outright and reaches the others by S(q + 1) = S(q) + ref(q + width) - ref(q), sixteen consecutive windows
per thread and round; no prefix array.  Whole chromosomes of 0.3 - 0.7 Mb, built as tests/test_cand_byte_walk.py builds
them (no N, no GC adjustment, Poisson(30) with planted events), put the FINAL tests (one per raw call, on the call's final
coordinates) at the shapes at which that kernel can go wrong.

Every case is checked twice.  On the CPU, `test_geometry` replays the reference walk over the oracle's compacted depth
(`_walk` of that file) and asserts that the case is the shape it claims: nref, used0, width, nwin, thinned or not.  On the
GPU, `test_forms` runs the chromosome through the one-workgroup form -- which still builds its prefix array: the independent
implementation here -- and the split form, each with byte and with int32 storage (RSI_HOT_CAND_SPLIT x RSI_HOT_CAND_BYTES),
and compares segments, raw calls and calls with the oracle; byte against int32 storage bit for bit.  No test may have gone
to the host walk.  The one exception is the neighbourhood not longer than the body: the device sets flag 1 and reads
nothing, and the run is refused as unsupported in every form (the reference aborts there)."""
import numpy as np
import pytest

from conftest import calls_equal
from test_cand_byte_walk import _walk

CHUNKS = 16             # kCandChunks: workgroups that share a test's windows
PER = 16                # consecutive windows per thread and round
THREADS = 1024          # threads of a workgroup
ROUND = PER * THREADS   # windows of a chunk per round
MEAN = 30
DEFAULTS = dict(m=101, minmlen=3.01, buffer=0.05, chklen=2.5, maxchkbp=100000)


def chunk_len(nwin, chunks=CHUNKS):
    """cand_chunk_len: a sixteenth of the windows, rounded up to a multiple of four."""
    return (((nwin + chunks - 1) // chunks) + 3) & ~3


def sum_chunks(nref, width):
    """cand_sum_chunks: as many chunks as keep chunks x width <= 4 x nref, sixteen at the most."""
    return min(CHUNKS, 4 * nref // width)


def geometry(rdc, L, i, P):
    """cand_geometry for the final test of L[i], from the replayed walk."""
    w = _walk(rdc, L, i, P)
    nbody = L[i]["end"] - L[i]["start"] + 1
    used0, rcnt = w["left"]["taken"], w["right"]["taken"]
    g = dict(used0=used0, nref_raw=used0 + rcnt, nref=used0 + rcnt, width=nbody, thin=False, nbody=nbody, type=L[i]["type"])
    budget = P["maxchkbp"] * 10
    if g["nref_raw"] + nbody > budget:
        total = g["nref_raw"] + nbody
        g["nref"] = int(g["nref_raw"] / total * budget)
        g["width"] = int(nbody / total * budget)
        g["thin"] = True
    g["nwin"] = g["nref"] - g["width"]
    return g


def _chrom(n, events, seed, const=None, wide=None, scale=1):
    """Poisson(30) with events (a, b, factor); const = (a, b, v): depth forced to v; wide = (a, b, lo, hi): uniform in lo .. hi - 1;
    scale: the whole depth times that, plus a little noise (int32 compacted depth beyond 254)."""
    rng = np.random.default_rng(seed)
    fasta = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n)
    depth = rng.poisson(MEAN, n).astype(np.int32)
    last = (n - 10_000, n - 7_000, 0.5)   # the chromosome's last marked run is never emitted: a dummy takes that place
    for a, b, f in list(events) + [last]:
        depth[a:b] = rng.poisson(MEAN * f, b - a) if f < 3 else rng.integers(100, 119, b - a)
    if const is not None:
        depth[const[0]:const[1]] = const[2]
    if wide is not None:
        depth[wide[0]:wide[1]] = rng.integers(wide[2], wide[3], wide[1] - wide[0])
    if scale != 1:
        depth = (depth * scale + rng.integers(0, scale, depth.size)).astype(np.int32)
    return fasta, depth


def _slots(T, body, frac=0.5):
    """-reflen that gives a call of `body` bases T slots on the left and T + 1 on the right: chklen * d = T + 0.5.
    With frac = 0.25 the capacity int(2 * chklen * d) is 2 T, and the right side gets T as well."""
    return (T + frac) / body


N = 400_000
BIG_END = 204_200
DEL = (180_000, 188_000, 0.5)    # becomes a call of 8004 bases at seeds 21 and 23, of 8003 at (340 000, 348 000) with seed 22
BIG = (100_000, BIG_END, 0.5)    # a third of its chromosome of 300 000
SPIKE = 100                      # beyond 3 x 30: a deletion's walks drop it


def _spiked(extra):
    """A chromosome of 300 000 with a deletion of 104 200 in the middle and, outside the deletion and its margins, a 100 on
    eight bases of every seventeen: every bin keeps a median below the spikes, the per-base walks run to both ends of the
    chromosome and take 9/17 of what they pass -- 88 values more than the body has.  `extra` more spikes, one in 85 bases
    from 20 000 on, take as many windows off."""
    fasta, depth = _chrom(300_000, [BIG], 21)
    p = np.arange(300_000)
    depth[((p % 17) < 8) & ((p < 93_000) | ((p > 207_000) & (p < 289_000)))] = SPIKE
    depth[20_000 + 8 + 85 * np.arange(extra)] = SPIKE
    return fasta, depth


def _case(name):
    """-> (parameter keywords, fasta, depth)"""
    kw = dict(gcadjust=0)
    if name in SPIKES_OFF:
        return kw, *_spiked(SPIKES_OFF[name])      # extra spikes
    if name == "one_round":                           # nref = 2 T + 1, nwin = nref - 8003
        return dict(kw, chklen=_slots((NWIN_ROUND + 8003) // 2, 8003)), *_chrom(700_000, [(340_000, 348_000, 0.5)], 22)
    if name == "one_round_and_one":
        return dict(kw, chklen=_slots((NWIN_LAST_ONE + 8003) // 2, 8003, 0.25)), *_chrom(700_000, [(340_000, 348_000, 0.5)], 22)
    if name.startswith("seam_"):                      # used0 = T
        return dict(kw, chklen=_slots(int(name.split("_")[1]), 8004)), *_chrom(N, [DEL], 23)
    if name == "thinned":
        return dict(kw, chklen=10.0, maxchkbp=3000), *_chrom(N, [(180_000, 184_000, 0.5)], 24)
    if name == "int32_depth":
        return dict(kw, chklen=4.0), *_chrom(N, [(180_000, 188_000, 1.5)], 25, scale=10)
    if name == "short_reflen":                        # nref < 4 x width: fewer, longer chunks
        return dict(kw, chklen=0.9), *_chrom(N, [(150_000, 190_000, 0.5)], 26)
    if name == "body_one_value":
        # within 2.25 of its lengths of the chromosome's start a candidate is not refined (optimize_with_derivative's range
        # check): it keeps its bin coordinates, which lie inside the plateau (a refined call ends on the first base outside)
        return dict(kw, chklen=4.0), *_chrom(N, [(10_000, 18_000, 0.5)], 27, const=(10_000, 18_000, 12))
    if name == "body_many_values":                    # the cap at 252 = 8.4 x 30 instead of 120: above every value, and the depth stays bytes
        return dict(kw, chklen=4.0, cap=8.4), *_chrom(N, [], 28, wide=(180_000, 188_000, 20, 250))
    raise KeyError(name)


NWIN_ROUND = CHUNKS * ROUND                                 # every chunk takes exactly one round
NWIN_LAST_ONE = (CHUNKS - 1) * (ROUND + 4) + ROUND + 1      # chunks of a round and four windows; the last: a round and ONE window
SPIKES_OFF = {"nwin_37": 88 - 37, "nwin_1": 88 - 1, "no_window": 88 + 7}
CASES = ["nwin_37", "nwin_1", "no_window", "one_round", "one_round_and_one", "seam_36000", "seam_36007", "thinned", "int32_depth",
         "short_reflen", "body_one_value", "body_many_values"]
_oracle_runs = {}


def _oracle(name, oracle_cls):
    """One oracle run per case, shared by the geometry test and the GPU test."""
    import oracle
    if name not in _oracle_runs:
        kw, fasta, depth = _case(name)
        O = oracle_cls()
        O.run(oracle.make_params(**kw), depth, fasta)
        P = dict(DEFAULTS)
        P.update(kw)
        _oracle_runs[name] = dict(kw=kw, fasta=fasta, depth=depth, P=P, rdc=O.i32("rd_concat"), noncode=O.i32("noncode"),
                                  calls={w: O.calls(w) for w in ("segs_nb", "calls_raw", "calls")})
    return _oracle_runs[name]


def sum_chunk_len(nwin, chunks):
    return (((nwin + chunks - 1) // chunks) + 3) & ~3


def _only(R, calls=None):
    """The geometry of the one final test of a case."""
    L = (calls or R)["calls"]["calls_raw"]
    assert len(L) == 1
    return L[0], geometry(R["rdc"], L, 0, R["P"]), _walk(R["rdc"], L, 0, R["P"])


@pytest.mark.parametrize("name", CASES)
def test_geometry(name, oracle_cls):
    R = _oracle(name, oracle_cls)
    rdc = R["rdc"]
    assert len(R["noncode"]) == 0 and np.array_equal(rdc, R["depth"])   # coordinates and values as planted
    assert (rdc.max() >= 255) == (name == "int32_depth")
    if name == "no_window":
        # the oracle drops a candidate without a window before its list of raw calls; the candidate is the one of nwin_1,
        # whose chromosome differs by eight spikes 20 000 bases and more from its edges
        assert len(R["calls"]["calls_raw"]) == 0
        c, g, w = _only(R, calls=_oracle("nwin_1", oracle_cls))
        assert g["nwin"] == -7 and not g["thin"]
        return
    c, g, w = _only(R)
    assert len(R["calls"]["calls"]) == 1
    chunks = sum_chunks(g["nref"], g["width"])
    Wc = sum_chunk_len(g["nwin"], chunks)
    assert g["thin"] == (name == "thinned") and g["nwin"] > 0
    if name in ("nwin_37", "nwin_1"):
        assert g["nwin"] == int(name.split("_")[1]) and c["type"] == 0
        assert w["left"]["end"] == "edge" and w["right"]["end"] == "edge"      # cut short by both ends of the chromosome
        assert chunks == 4 and chunk_len(g["nwin"]) == 4                        # four chunks in use, of 12 windows at the most
        assert Wc == (12 if name == "nwin_37" else 4) and g["nwin"] % Wc == 1   # the last chunk in use is partial: one window
    elif name == "one_round":
        assert chunks == CHUNKS and g["nwin"] == CHUNKS * ROUND and Wc == ROUND
    elif name == "one_round_and_one":
        assert chunks == CHUNKS and Wc == ROUND + 4 and g["nwin"] - (CHUNKS - 1) * Wc == ROUND + 1
    elif name.startswith("seam_"):
        assert chunks == CHUNKS and g["used0"] == int(name.split("_")[1]) and w["left"]["end"] == "full"
        enter = g["used0"] - g["width"]                                         # the window whose entering value is the seam's
        assert (enter - enter // Wc * Wc) % PER != 0                            # q + width crosses the seam inside a thread's sixteen
        if name == "seam_36000":
            assert g["used0"] % PER == 0 and g["used0"] % Wc == 0               # a chunk's first window starts at the seam
        else:
            assert g["used0"] % PER != 0 and g["used0"] % Wc % PER != 0         # q crosses it inside a thread's sixteen as well
    elif name == "thinned":
        assert 2000 < g["nbody"] < 6000 and g["width"] < g["nbody"] and g["nref"] < g["nref_raw"]
    elif name == "int32_depth":
        assert c["type"] == 1 and chunks == CHUNKS
    elif name == "short_reflen":
        assert 4 <= chunks < CHUNKS and g["nref"] < 2 * g["width"]
        assert chunks * g["width"] <= 4 * g["nref"]                             # what the start sums read
    elif name == "body_one_value":
        assert np.all(rdc[c["start"]:c["end"] + 1] == 12)
    elif name == "body_many_values":
        assert len(np.unique(rdc[c["start"]:c["end"] + 1])) > 200


@pytest.fixture(scope="module")
def hot():
    from rsicnv_amd import api
    h = api.RsiHot(0)
    yield h
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_forms(hot, oracle_cls, monkeypatch, name):
    from rsicnv_amd import api
    R = _oracle(name, oracle_cls)
    byte_depth = name != "int32_depth"
    got = {}
    hot.set_timing(1)        # rsi_hot_kernel_times names what ran
    for split in (0, 1):
        for wide in (1, 0):
            monkeypatch.setenv("RSI_HOT_CAND_SPLIT", str(split))
            monkeypatch.setenv("RSI_HOT_CAND_BYTES", str(wide))
            if name == "no_window":
                # flag 1 from the device, which reads nothing; the host finds the neighbourhood empty as well and refuses the
                # chromosome as the reference does (it aborts in isitcnv, rsi.cpp:107)
                with pytest.raises(api.RsiError, match="longer than the neighbourhood"):
                    hot.run(api.make_params(**R["kw"]), R["depth"], R["fasta"])
                continue
            res = hot.run(api.make_params(**R["kw"]), R["depth"], R["fasta"])
            phases = dict(hot.phase_times())
            kernels = {k for k, _ in hot.kernel_times() if k.startswith("candidate_test")}
            print(name, "split", split, "bytes", wide, "tests", phases["calls.ntests"], "host fallbacks", phases["calls.host_fallbacks"],
                  "raw calls", len(res.calls("calls_raw")), sorted(kernels))
            # the form and the storage that were asked for are the ones that ran (int32 depth has the one storage, under the plain names)
            want = ("candidate_test" if split else "candidate_test_one_wg") + ("_i32" if wide == 0 and byte_depth else "")
            assert kernels == {want}, (split, wide, kernels)
            assert phases["calls.ntests"] >= 1
            assert phases["calls.host_fallbacks"] == 0, (split, wide, phases)
            for mine, theirs in (("segs", "segs_nb"), ("calls_raw", "calls_raw"), ("calls", "calls")):
                ok, why = calls_equal(res.calls(mine), R["calls"][theirs])
                assert ok, f"split {split} bytes {wide} {mine}: {why}"
            got[split, wide] = res.calls("calls_raw")
        if name == "no_window":
            continue
        ok, why = calls_equal(got[split, 1], got[split, 0], rtol=0)    # the storage width changes no bit
        assert ok, f"split {split}, byte against int32 storage: {why}"
