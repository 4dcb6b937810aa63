"""The candidate tests' byte-wide scratch and the 65 536-position trips of the byte walk (kernels_cand.hip), on whole
chromosomes of 0.7 Mb placed so that the walks of the FINAL tests (call_from_segments: one test per raw call, on the
call's final coordinates) meet the shapes at which a trip's bookkeeping can go wrong.

Every case is checked twice.  On the CPU, `test_geometry_*` replays the reference walk (rsi.cpp:206-257) over the
oracle's compacted depth and asserts that the case is what it says: how many values a side takes, at which position of a
trip a trigger or the last slot falls, where the walk ends.  On the GPU, `test_forms_*` runs the chromosome through the
one-workgroup and the four-launch form, each with byte and with int32 storage (RSI_HOT_CAND_SPLIT x RSI_HOT_CAND_BYTES),
and compares segments, raw calls and calls with the oracle, as tests/test_hot_extra.py does; byte against int32 storage
bit for bit.  No test may have gone to the host walk.

The chromosomes have no N, so compacted and reference coordinates are the same, and no GC adjustment, so planted values
arrive in the compacted depth as they are.  Depth is Poisson(30): for a deletion the walk drops values above 3 x 30, which
Poisson(30) never reaches, so every position outside a neighbour is taken unless a case plants a 100 there."""
import numpy as np
import pytest

from conftest import calls_equal

TRIP = 65536            # positions per trip of the byte walk: 1024 threads x four 16-byte loads
N = 700_000
MEAN = 30
LAST = (690_000, 693_000, 0.5)   # the chromosome's last marked run is never emitted: a dummy takes that place
BODY = 8003             # length of the call that a planted deletion of 8000 bases becomes


def _chrom(events, seed, spikes=(), n=N):
    rng = np.random.default_rng(seed)
    fasta = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n)
    depth = rng.poisson(MEAN, n).astype(np.int32)
    for a, b, f in list(events) + [LAST]:
        depth[a:b] = rng.poisson(MEAN * f, b - a) if f < 3 else rng.integers(100, 119, b - a)
    for p in spikes:
        depth[p] = 100
    return fasta, depth


def _sides(T):
    """-reflen that gives the call of BODY bases T slots on the left and T + 1 on the right: chklen * d = T + 0.5."""
    return (T + 0.5) / BODY


def _walk(rdc, L, i, P):
    """isitcnvwrap's two walks for the final test of L[i] (the host restatement: host_calls.cpp, test_candidate).  Per side:
    values taken, and for every straight stretch (a trip sequence of the device walk starts at each) the positions of
    triggers, of the value that filled the last slot and of the chromosome's end, counted from the stretch's start."""
    n = len(rdc)
    me = L[i]
    kind, blen = me["type"], me["end"] - me["start"] + 1
    d = max(blen, int(P["m"] * P["minmlen"]))
    cap = int(P["chklen"] * d * 2)
    margin = int(blen * P["buffer"] + 1)
    top = int(P["chklen"] * d - 1)
    if n - me["end"] < P["chklen"] * d:
        top = cap - 1 - n + me["end"]
    med = float(np.median(rdc))
    skip = (lambda v: v > med * 3.0) if kind == 0 else (lambda v: v < med * 0.15)
    out = {}
    # left
    pos = me["start"] - margin
    nb = i - 1
    while pos > 0 and nb > 0 and pos < L[nb]["start"]:
        nb -= 1
    fill, seg = top, pos
    side = dict(taken=0, triggers=[], last_t=None, end="full", crossed_extreme=0, first_pos=pos)
    while pos > 2 and fill >= 0:
        pos -= 1
        if nb >= 0 and pos == L[nb]["start"] and all(skip(v) for v in rdc[L[nb]["start"]:L[nb]["end"] + 1]):
            side["crossed_extreme"] += 1
        if skip(rdc[pos]):
            continue
        if nb >= 0 and L[nb]["start"] <= pos <= L[nb]["end"]:
            side["triggers"].append(seg - 1 - pos)
            pos = L[nb]["start"] - 1
            seg = pos
            nb -= 1
            continue
        fill -= 1
        side["taken"] += 1
        side["last_t"] = seg - 1 - pos
    if fill >= 0:
        side["end"] = "edge"
        side["edge_t"] = seg - 1 - pos
    out["left"] = side
    used = side["taken"] if fill >= 0 else top + 1
    # right
    pos = me["end"] + margin
    nb = i + 1
    while pos < n - 2 and nb < len(L) and pos > L[nb]["end"]:
        nb += 1
    seg = pos
    side = dict(taken=0, triggers=[], last_t=None, end="edge", crossed_extreme=0, first_pos=pos)
    while pos < n - 2 and used < 2 * P["chklen"] * d:
        pos += 1
        if nb < len(L) and pos == L[nb]["end"] and all(skip(v) for v in rdc[L[nb]["start"]:L[nb]["end"] + 1]):
            side["crossed_extreme"] += 1
        if skip(rdc[pos]):
            continue
        if nb < len(L) and L[nb]["start"] <= pos <= L[nb]["end"]:
            side["triggers"].append(pos - seg - 1)
            pos = L[nb]["end"] + 1
            seg = pos
            nb += 1
            continue
        if used >= cap:
            break
        used += 1
        side["taken"] += 1
        side["last_t"] = pos - seg - 1
    if used >= cap or not used < 2 * P["chklen"] * d:
        side["end"] = "full"
    else:
        side["edge_t"] = pos - seg - 1
    out["right"] = side
    out["total"] = used + blen
    return out


MAIN = (340_000, 348_000, 0.5)
EDGE_T = [64 * tid + e for tid in (0, 5, 517, 1023) for e in (0, 15, 16, 31, 32, 47, 48, 63)]   # both ends of a thread's four loads
# first positions of the two walks of MAIN's call with the spikes in place (start 340 000, end 348 002, margin 401): the
# geometry test holds them to that
L0, R0 = 340_000 - 401, 348_002 + 401


def _case(name):
    """-> (oracle / api parameter keywords, fasta, depth)"""
    kw = dict(gcadjust=0)
    if name.startswith("sides_"):
        T = int(name.split("_")[1])
        return dict(kw, chklen=_sides(T)), *_chrom([MAIN], 11)
    if name in ("trigger_last_of_trip", "trigger_first_of_next_trip"):
        # the right walk of the first call starts behind end + margin = 208 001 + 401; the neighbour's call starts with its deletion
        t = TRIP - 1 if name == "trigger_last_of_trip" else TRIP
        first = 208_001 + 401 + 1 + t
        return dict(kw, chklen=10.0), *_chrom([(200_000, 208_000, 0.5), (first, first + 6000, 0.5)], 12)
    if name == "neighbour_all_extreme":
        # Boundary refinement ends a call on the first base outside its plateau, so a refined duplication always holds a base
        # that is not extreme.  A candidate within 2.25 of its lengths of the chromosome's start is not refined
        # (optimize_with_derivative's range check): it keeps its bin coordinates, which lie inside the plateau of 100 and more.
        return dict(kw, chklen=10.0), *_chrom([(2_500, 5_500, 0.5), (8_000, 14_000, 4.0), (40_000, 48_000, 0.5)], 13)
    if name == "chromosome_ends":
        return dict(kw, chklen=10.0), *_chrom([(30_000, 38_000, 0.5), (N - 60_000, N - 52_000, 0.5)], 14)
    if name == "extremes_at_load_edges":
        return dict(kw, chklen=10.0), *_chrom([MAIN], 11, spikes=[R0 + 1 + t for t in EDGE_T] + [L0 - 1 - t for t in EDGE_T])
    if name == "thinned":
        return dict(kw, chklen=10.0, maxchkbp=5000), *_chrom([MAIN], 16)
    raise KeyError(name)


CASES = ["sides_65535", "sides_65536", "sides_65537", "sides_131073", "trigger_last_of_trip", "trigger_first_of_next_trip",
         "neighbour_all_extreme", "chromosome_ends", "extremes_at_load_edges", "thinned"]
_oracle_runs = {}


def _oracle(name, oracle_cls):
    """One oracle run per case, shared by the geometry test and the GPU test."""
    import oracle
    if name not in _oracle_runs:
        kw, fasta, depth = _case(name)
        O = oracle_cls()
        O.run(oracle.make_params(**kw), depth, fasta)
        P = dict(m=101, minmlen=3.01, buffer=0.05, chklen=2.5, maxchkbp=100000)
        P.update(kw)
        _oracle_runs[name] = dict(kw=kw, fasta=fasta, depth=depth, P=P, rdc=O.i32("rd_concat"), noncode=O.i32("noncode"),
                                  calls={w: O.calls(w) for w in ("segs_nb", "calls_raw", "calls")})
    return _oracle_runs[name]


@pytest.mark.parametrize("name", CASES)
def test_geometry(name, oracle_cls):
    R = _oracle(name, oracle_cls)
    rdc, L, P = R["rdc"], R["calls"]["calls_raw"], R["P"]
    assert len(R["noncode"]) == 0 and len(rdc) == N and np.array_equal(rdc, R["depth"])   # coordinates and values as planted
    assert len(R["calls"]["calls"]) >= 1 and rdc.max() < 255
    W = [_walk(rdc, L, i, P) for i in range(len(L))]
    if name.startswith("sides_"):
        T = int(name.split("_")[1])
        assert len(L) == 1 and L[0]["end"] - L[0]["start"] + 1 == BODY and L[0]["type"] == 0
        w = W[0]
        assert (w["left"]["taken"], w["right"]["taken"]) == (T, T + 1)
        assert w["left"]["end"] == "full" and w["right"]["end"] == "full" and not w["left"]["triggers"] and not w["right"]["triggers"]
        # nothing dropped: the value that fills the last slot is the taken-count's own position -- for 65 536 slots the last of a trip
        assert w["left"]["last_t"] == T - 1 and w["right"]["last_t"] == T
        assert w["total"] <= P["maxchkbp"] * 10
    elif name.startswith("trigger_"):
        t = TRIP - 1 if name == "trigger_last_of_trip" else TRIP
        assert len(L) == 2
        assert W[0]["right"]["triggers"] == [t] and rdc[L[1]["start"]] <= 90
        assert W[0]["right"]["taken"] > t + 1            # the walk goes on behind the neighbour
    elif name == "neighbour_all_extreme":
        assert len(L) == 3 and [c["type"] for c in L] == [0, 1, 0]
        assert rdc[L[1]["start"]:L[1]["end"] + 1].min() > 90
        # the first call's right walk crosses the duplication without a trigger, and -- its neighbour pointer left where it
        # was -- walks through the third call as well, taking its values; the third call's left walk likewise, to the chromosome's start
        r = W[0]["right"]
        assert r["crossed_extreme"] == 1 and r["triggers"] == [] and r["first_pos"] + r["last_t"] + 1 > L[2]["end"]
        l = W[2]["left"]
        assert l["crossed_extreme"] == 1 and l["triggers"] == [] and l["end"] == "edge"
    elif name == "chromosome_ends":
        assert len(L) == 2
        assert W[0]["left"]["end"] == "edge" and 0 < W[0]["left"]["edge_t"] < TRIP - 1 and W[0]["left"]["taken"] > 0
        assert W[1]["right"]["end"] == "edge" and 0 < W[1]["right"]["edge_t"] < TRIP - 1 and W[1]["right"]["taken"] > 0
        assert W[1]["left"]["taken"] > TRIP          # top follows the short right side (rsi.cpp:203): the left takes more
    elif name == "extremes_at_load_edges":
        assert len(L) == 1 and (W[0]["left"]["first_pos"], W[0]["right"]["first_pos"]) == (L0, R0)
        assert all(rdc[R0 + 1 + t] == 100 and rdc[L0 - 1 - t] == 100 for t in EDGE_T)
        assert W[0]["left"]["taken"] > TRIP and W[0]["right"]["taken"] > TRIP
        assert W[0]["left"]["last_t"] == W[0]["left"]["taken"] - 1 + len(EDGE_T)
    elif name == "thinned":
        assert len(L) == 1 and W[0]["total"] > P["maxchkbp"] * 10 and W[0]["left"]["taken"] > TRIP


def _run_forms(hot, monkeypatch, R, need_device_tests=True, byte_depth=True):
    from rsicnv_amd import api
    got = {}
    hot.set_timing(1)        # rsi_hot_kernel_times names what ran
    for split in (0, 1):
        for wide in (1, 0):
            monkeypatch.setenv("RSI_HOT_CAND_SPLIT", str(split))
            monkeypatch.setenv("RSI_HOT_CAND_BYTES", str(wide))
            res = hot.run(api.make_params(**R["kw"]), R["depth"], R["fasta"])
            phases = dict(hot.phase_times())
            kernels = {k for k, _ in hot.kernel_times() if k.startswith("candidate_test")}
            # the form and the storage that were asked for are the ones that ran (int32 depth has the one storage, under the plain names)
            want = ("candidate_test" if split else "candidate_test_one_wg") + ("_i32" if wide == 0 and byte_depth else "")
            assert kernels == {want}, (split, wide, kernels)
            if need_device_tests:
                assert phases["calls.host_fallbacks"] == 0 and phases["calls.ntests"] >= 1, (split, wide, phases)
            for mine, theirs in (("segs", "segs_nb"), ("calls_raw", "calls_raw"), ("calls", "calls")):
                ok, why = calls_equal(res.calls(mine), R["calls"][theirs])
                assert ok, f"split {split} bytes {wide} {mine}: {why}"
            got[split, wide] = res.calls("calls_raw")
        ok, why = calls_equal(got[split, 1], got[split, 0], rtol=0)    # the storage width changes no bit
        assert ok, f"split {split}, byte against int32 storage: {why}"


@pytest.fixture(scope="module")
def hot():
    from rsicnv_amd import api
    h = api.RsiHot(0)
    yield h
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_forms(hot, oracle_cls, monkeypatch, name):
    R = _oracle(name, oracle_cls)
    assert len(R["calls"]["calls"]) >= 1
    _run_forms(hot, monkeypatch, R)


@pytest.mark.gpu
def test_forms_deep_coverage_keeps_the_int32_path(hot, oracle_cls, monkeypatch):
    """Ten times the depth (values to 600, int32 compacted depth): storage stays int32 whatever RSI_HOT_CAND_BYTES says."""
    import oracle
    fasta, depth = _chrom([MAIN], 17)
    depth = (depth * 10 + np.random.default_rng(17).integers(0, 10, depth.size)).astype(np.int32)
    kw = dict(gcadjust=0, chklen=10.0)
    O = oracle_cls()
    O.run(oracle.make_params(**kw), depth, fasta)
    assert O.i32("rd_concat").max() >= 255 and len(O.calls("calls")) >= 1
    R = dict(kw=kw, fasta=fasta, depth=depth, calls={w: O.calls(w) for w in ("segs_nb", "calls_raw", "calls")})
    _run_forms(hot, monkeypatch, R, need_device_tests=False, byte_depth=False)
