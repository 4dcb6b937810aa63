"""GPU: a BGZF bedGraph read by its index (rsi_genome_bedgraph_open_indexed, `-d FILE.bed.gz -c RNAME` with FILE.tbi / FILE.csi).
Whatever the member layout and wherever the index comes from -- a .tbi or .csi written by tabix_util from the format's layout, or
the .tbi the project's own track writer leaves -- the reader hands over what rsi_genome_bedgraph_open hands over for the same
file and names, from the members of the chromosome's range alone; an index that does not fit the file is an error."""
import os
import subprocess

import numpy as np
import pytest

import tabix_util as tx
from bgzf_util import bgzf
from conftest import make_case
from test_bedgraph_depth import check_equal
from test_genome_text import EXE, write_fasta

LENS = {"chr1": 60_000, "chr2": 90_000, "chr3": 50_000, "chr4": 40_000}
BAD_ARG = -2


def chrom_text(name, n, seed, lines=100):
    """About `lines` bedGraph lines covering [0, n), one of them across a 16 384-base window boundary."""
    rng = np.random.default_rng(seed)
    cuts = sorted(set([0, n] + [int(x) for x in rng.integers(1, n, lines - 1)]))
    return "".join(f"{name}\t{a}\t{b}\t{int(rng.integers(0, 90))}\n" for a, b in zip(cuts, cuts[1:])).encode()


TEXTS = {name: chrom_text(name, n, 40 + k) for k, (name, n) in enumerate(LENS.items())}


def layout(kind):
    """(text, member sizes, the chromosomes to ask for)."""
    three = TEXTS["chr1"] + TEXTS["chr2"] + TEXTS["chr3"]
    if kind == "one_member":                       # begin and end inside the same member
        return three, [len(three)], ["chr2"]
    if kind == "late_begin":                       # chr2 begins in the last line of a member
        first = TEXTS["chr2"].index(b"\n") + 1
        return three, [len(TEXTS["chr1"]) + first] + [700] * 40, ["chr2"]
    if kind == "first_and_last":
        return three + TEXTS["chr4"], [1000] * 60, ["chr1", "chr4"]
    if kind == "single_member":                    # chr2's range is exactly one member
        return three, [len(TEXTS["chr1"]), len(TEXTS["chr2"]), len(TEXTS["chr3"])], ["chr2"]
    if kind == "unsorted":                         # the host fallback: chr3 has an interval out of order
        text = three + b"chr3\t10\t20\t55\n" + TEXTS["chr4"]
        return text, [900] * 60, ["chr3"]
    if kind == "cut_name":                         # the range's last member ends inside a chr10 line, cut behind "chr1"
        ten = chrom_text("chr10", 30_000, 77, lines=40)
        k = ten.index(b"\n", 200) + 1
        assert ten[k:k + 5] == b"chr10"
        return TEXTS["chr1"] + ten, [len(TEXTS["chr1"]) + k + 4, 500, 500, 500], ["chr1"]
    raise KeyError(kind)


def read(path, name, index=None):
    """({name: (depth, stats)}, inflate stats, index range) of one reader."""
    from rsicnv_amd import api
    out = {}
    with api.GenomeText(str(path), [name], [LENS[name]], bedgraph=True, index=None if index is None else str(index)) as g:
        for nm, ptr, n, st in g:
            out[nm] = (None if ptr is None else g.depth(st["slot"]), st)
        return out, g.inflate_stats(), (g.index_range() if index is not None else None)


def range_members(table, index, name):
    """The members from the one of the smallest chunk begin to the one that holds the last byte before the largest end."""
    ref = index["refs"][index["names"].index(name)]
    beg = min(c[0] for cs in ref["bins"].values() for c in cs)
    end = max(c[1] for cs in ref["bins"].values() for c in cs)
    tb, te = tx.resolve(beg, table), tx.resolve(end, table)
    return [m for m in table if m[2] < te and m[2] + len(m[3]) > tb], beg, end


WHOLE = {}


@pytest.mark.gpu
@pytest.mark.parametrize("source", ["tbi", "csi", "csi_12_6_pseudo"])
@pytest.mark.parametrize("kind", ["one_member", "late_begin", "first_and_last", "single_member", "unsorted", "cut_name"])
def test_indexed_reader_equals_the_whole_file_reader(tmp_path, kind, source):
    text, sizes, asked = layout(kind)
    data = bgzf(text, sizes=iter(sizes + [65280] * 8))
    path = tmp_path / "f.bed.gz"
    path.write_bytes(data)
    table = tx.member_table(data)
    if source == "tbi":
        index = tx.build_index(text, table, "tbi")
        ipath = tmp_path / "f.bed.gz.tbi"
        tx.write_index(str(ipath), index)
    else:
        index = tx.build_index(text, table, "csi", *((12, 6) if source != "csi" else (14, 5)))
        ipath = tmp_path / "f.bed.gz.csi"
        tx.write_index(str(ipath), index, pseudo=source != "csi")
    for name in asked:
        if (kind, name) not in WHOLE:
            WHOLE[(kind, name)] = read(path, name)[:2]
        ref, ref_st = WHOLE[(kind, name)]
        got, st, rng = read(path, name, ipath)
        # the sequences the reader does not know are named and passed over (no depth): the whole-file reader meets all of
        # them, the indexed one only those inside the range; what is handed over with a depth must be the same
        kept = lambda d: {k: v for k, v in d.items() if v[0] is not None}
        check_equal(kept(got), kept(ref), f"{kind} {source} {name}")
        assert list(kept(got)) == [name] and set(got) <= set(ref) and got[name][1]["fallback"] == (1 if kind == "unsorted" else 0)
        members, beg, end = range_members(table, index, name)
        assert st["blocks"] == len(members) and st["compressed_bytes"] == sum(m[1] for m in members)
        assert rng == (members[0][0], members[-1][0] + members[-1][1])
        assert st["format"] == "bgzf" and st["eof_block"] == ref_st["eof_block"] == 1 and ref_st["blocks"] == len(table) + 1
        if kind == "one_member":
            assert beg & 0xFFFF > 0 and beg >> 16 == end >> 16 == 0 and len(members) == 1
        if kind == "late_begin":
            m = members[0]
            assert m[3][(beg & 0xFFFF):].count(b"\n") == 1 and m[3].endswith(b"\n") and beg & 0xFFFF > 0
        if kind == "single_member":
            assert len(members) == 1 and beg & 0xFFFF == 0 and end & 0xFFFF == 0
        if kind == "cut_name":                     # what follows the range in its member is not handed on: no "chr1" fragment
            assert members[0][3].endswith(b"\nchr1") and end & 0xFFFF == len(TEXTS["chr1"]) and list(got) == ["chr1"]
    # a name the index does not hold: nothing is handed over, as for a file without its lines
    from rsicnv_amd import api
    with api.GenomeText(str(path), ["chr9"], [1000], bedgraph=True, index=str(ipath)) as g:
        assert list(g) == [] and g.index_range() == (0, 0) and g.inflate_stats()["blocks"] == 0


def misfits(text, table, good):
    """(what, index) for the four ways an index can miss its file; each changes chr2's range in the good index."""
    import copy
    ref_k = good["names"].index("chr2")
    lo = min((c[0], b, k) for b, cs in good["refs"][ref_k]["bins"].items() for k, c in enumerate(cs))
    hi = max((c[1], b, k) for b, cs in good["refs"][ref_k]["bins"].items() for k, c in enumerate(cs))

    def with_chunk(which, value):
        ix = copy.deepcopy(good)
        _, b, k = lo if which == 0 else hi
        c = list(ix["refs"][ref_k]["bins"][b][k])
        c[which] = value
        ix["refs"][ref_k]["bins"][b][k] = tuple(c)
        return ix

    lines = tx.parse_lines(text)
    first2 = next(l for l in lines if l[0] == "chr2")
    last2 = [l for l in lines if l[0] == "chr2"][-1]
    before = [l for l in lines if l[0] == "chr1"][-1]
    return [
        ("no sound member", with_chunk(0, ((lo[0] >> 16) + 3) << 16 | (lo[0] & 0xFFFF))),                 # not at a member header
        ("inside a line", with_chunk(0, tx.to_voff(first2[3] + 2, table))),                             # behind a byte other than '\n'
        ("names chr1", with_chunk(0, tx.to_voff(before[3], table))),                                    # the first line is another chromosome's
        ("a line of chr2 follows", with_chunk(1, tx.to_voff(last2[3], table))),                         # chr2 goes on behind the end
    ] if tx.to_voff(last2[3], table) & 0xFFFF else pytest.fail("the layout puts chr2's last line at a member's start: nothing follows inside the member")


@pytest.mark.gpu
def test_an_index_that_does_not_fit_the_file_is_refused(tmp_path):
    from rsicnv_amd import api
    text, sizes, _ = layout("first_and_last")
    data = bgzf(text, sizes=iter(sizes))
    path = tmp_path / "f.bed.gz"
    path.write_bytes(data)
    table = tx.member_table(data)
    good = tx.build_index(text, table, "tbi")
    for what, ix in misfits(text, table, good):
        ipath = tmp_path / "bad.tbi"
        tx.write_index(str(ipath), ix)
        with pytest.raises(api.RsiError) as e:
            read(path, "chr2", ipath)
        assert e.value.code == BAD_ARG and "bad.tbi" in str(e.value) and what in str(e.value), (what, str(e.value))
    (tmp_path / "junk.tbi").write_bytes(b"junk")
    with pytest.raises(api.RsiError) as e:
        read(path, "chr2", tmp_path / "junk.tbi")
    assert e.value.code == BAD_ARG and "junk.tbi" in str(e.value)
    plain = tmp_path / "plain.bed"
    plain.write_bytes(text)
    tx.write_index(str(tmp_path / "good.tbi"), good)
    with pytest.raises(api.RsiError) as e:
        read(plain, "chr2", tmp_path / "good.tbi")
    assert e.value.code == BAD_ARG and "not BGZF" in str(e.value)


def test_the_symbols_are_declared_and_exported(hotlib):
    from rsicnv_amd import api
    for sym in ("rsi_genome_bedgraph_open_indexed", "rsi_genome_text_index_range"):
        assert sym in api.EXPORTS and hasattr(hotlib, sym)


# ---- the command line, on a track the project wrote and indexed itself ----

def _cli(args, timeout=600):
    return subprocess.run([EXE, "rsi"] + args, capture_output=True, text=True, timeout=timeout)


def rows_of(path):
    return [l for l in open(path).read().splitlines() if not l.startswith("#")]


def steady(log):
    """A log without what differs by design: the index line, timings, the inflate line (its byte counts are the range's), and
    the echo of the command, which holds -dindex none."""
    return [l for l in log.splitlines() if not l.startswith(("#depth index:", "#depth file: BGZF", "timing:", "#command:"))]


@pytest.fixture(scope="module")
def own_track(hotlib, tmp_path_factory):
    """Three chromosomes run from a whole-genome depth file, their depth saved as a BGZF track with -trackindex."""
    from test_genome_text import chrom_lines, render
    tmp = str(tmp_path_factory.mktemp("indexed_cli"))
    specs = [("chr1", dict(n=150_007, seed=0xE21, model=1, n_events=3, gaps=1, max_len=8000, end_n=3000, gap_len=5000)),
             ("chr2", dict(n=120_019, seed=0xE22, model=0, n_events=3, gaps=0, max_len=8000, end_n=3000)),
             ("chr3", dict(n=100_003, seed=0xE23, model=0, n_events=2, gaps=0, max_len=8000, end_n=3000))]
    lines, seqs = [], []
    for i, (name, kw) in enumerate(specs):
        _, fasta, depth = make_case(hotlib, kw)
        seqs.append((name, fasta))
        lines += chrom_lines(name, depth, fasta.size, 500 + i, quirks=False)
    fa = os.path.join(tmp, "ref.fa")
    write_fasta(fa, seqs)
    depth_file = os.path.join(tmp, "genome.depth")
    with open(depth_file, "w") as f:
        f.write(render(lines, 9))
    track = os.path.join(tmp, "t.bed.gz")
    r = _cli(["-f", fa, "-d", depth_file, "-o", os.path.join(tmp, "first.txt"), "-np", "-track", track, "-trackindex"])
    assert r.returncode == 0 and os.path.exists(track + ".tbi"), r.stderr[-3000:]
    return dict(tmp=tmp, fa=fa, track=track, rows=rows_of(os.path.join(tmp, "first.txt")))


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_cli_reads_by_the_sibling_index(own_track):
    g = own_track
    tmp = g["tmp"]
    whole, fast = os.path.join(tmp, "whole.txt"), os.path.join(tmp, "fast.txt")
    r0 = _cli(["-f", g["fa"], "-d", g["track"], "-c", "chr2", "-o", whole, "-np", "-dindex", "none"])
    r1 = _cli(["-f", g["fa"], "-d", g["track"], "-c", "chr2", "-o", fast, "-np"])
    assert r0.returncode == 0 and r1.returncode == 0, r0.stderr[-2000:] + r1.stderr[-2000:]
    assert open(fast).read().replace(fast, whole) == open(whole).read() and rows_of(fast) == [l for l in g["rows"] if l.split("\t")[0] == "chr2"]
    log0, log1 = open(whole + ".log").read(), open(fast + ".log").read()
    assert "#depth index:" not in log0 and f"#depth index: {g['track']}.tbi, members at compressed offsets " in log1
    assert steady(log1.replace(fast, whole)) == steady(log0)
    # the range in the log is chr2's part of the file, and fewer bytes were inflated than the file holds
    data = open(g["track"], "rb").read()
    index = tx.parse_index(g["track"] + ".tbi")
    members, _, _ = range_members(tx.member_table(data), index, "chr2")
    a, b = [l for l in log1.splitlines() if l.startswith("#depth index: /")][0].split("offsets ")[1].split(" ")[0].split("-")
    assert (int(a), int(b)) == (members[0][0], members[-1][0] + members[-1][1]) and int(a) > 0 and int(b) < len(data) - 28
    # the same through the project's own reader API: its .tbi, its file
    from rsicnv_amd import api
    names, lens = ["chr2"], [120_019]
    with api.GenomeText(g["track"], names, lens, bedgraph=True) as gw, api.GenomeText(g["track"], names, lens, bedgraph=True, index=g["track"] + ".tbi") as gi:
        s0 = next(st for nm, ptr, n, st in gw if nm == "chr2")      # (the whole-file reader names chr1 first, and passes over it)
        s1 = next(st for nm, ptr, n, st in gi if nm == "chr2")
        assert np.array_equal(gw.depth(s0["slot"]), gi.depth(s1["slot"]))
        assert all(s0[k] == s1[k] for k in ("lines", "stored", "beyond", "fallback"))
        assert gi.inflate_stats()["blocks"] == len(members)
    # an older index: a warning, and it is used
    os.utime(g["track"] + ".tbi", (1, 1))
    r2 = _cli(["-f", g["fa"], "-d", g["track"], "-c", "chr2", "-o", fast, "-np"])
    assert r2.returncode == 0 and "#depth index: warning: " in open(fast + ".log").read() and rows_of(fast) == rows_of(whole)


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_cli_refuses_an_index_of_another_file_and_an_absent_name(own_track):
    g = own_track
    tmp = g["tmp"]
    data = open(g["track"], "rb").read()
    table = tx.member_table(data)
    text = b"".join(m[3] for m in table)
    good = tx.build_index(text, table, "tbi")
    assert tx.resolved(tx.parse_index(g["track"] + ".tbi"), table) == {k: dict(chunks=v["chunks"], linear=v["linear"])
                                                                          for k, v in tx.expected_index(text, table).items()}
    out = os.path.join(tmp, "refused.txt")
    for k, (what, ix) in enumerate(misfits(text, table, good)):
        bad = os.path.join(tmp, f"other_{k}.tbi")
        tx.write_index(bad, ix)
        r = _cli(["-f", g["fa"], "-d", g["track"], "-c", "chr2", "-o", out, "-np", "-dindex", bad])
        assert r.returncode == 1 and what in r.stderr and bad in r.stderr and not os.path.exists(out), (what, r.stderr[-1500:])
    only13 = dict(good, names=[n for n in good["names"] if n != "chr2"], refs=[r for n, r in zip(good["names"], good["refs"]) if n != "chr2"])
    absent = os.path.join(tmp, "absent.tbi")
    tx.write_index(absent, only13)
    r = _cli(["-f", g["fa"], "-d", g["track"], "-c", "chr2", "-o", out, "-np", "-dindex", absent])
    assert r.returncode == 1 and "no lines for chr2" in r.stderr and not os.path.exists(out)
    r = _cli(["-f", g["fa"], "-d", g["track"], "-o", out, "-np", "-dindex", absent])          # without -c the whole file is read anyway
    assert r.returncode == 1 and "-dindex" in r.stderr and not os.path.exists(out)
