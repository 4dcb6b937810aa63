"""GPU: region queries through the .tbi the track writer leaves (rsi_track_index_write_tbi), as a tabix reader makes them
(tabix_util.query): one file grown chromosome by chromosome with write_track(append=True), one joined from part files whose
indexes are appended with their shifts (rsi_track_index_append).  Every query returns exactly the overlapping lines."""
import gzip
import os

import numpy as np
import pytest

import bgzf_walk as bw
import tabix_util as tx
from conftest import make_case

CHROMS = [("chrA", 30_000, 0x1D01), ("chrB", 50_000, 0x1D02), ("chrC", 20_000, 0x1D03)]


@pytest.fixture(scope="module")
def files(hotlib, tmp_path_factory):
    """(grown file, joined file): each dict(data, index, text), after the same three runs."""
    from rsicnv_amd import api
    tmp = str(tmp_path_factory.mktemp("tbi_query"))
    grown, joined = os.path.join(tmp, "grown.bedgraph.gz"), os.path.join(tmp, "joined.bedgraph.gz")
    h = api.RsiHot(0)
    h.set_track_format("bgzf")
    whole, parts = api.TrackIndex(), []
    for k, (name, n, seed) in enumerate(CHROMS):
        _, fasta, depth = make_case(hotlib, dict(n=n, seed=seed, model=0, n_events=2, gaps=0, min_len=500, max_len=2000, end_n=1000))
        h.run(api.make_params(), depth, fasta)
        h.set_track_index(whole)
        h.write_track(0, name, grown, append=True)
        parts.append(api.TrackIndex())
        h.set_track_index(parts[-1])
        h.write_track(0, name, f"{joined}.part.{k}")
        h.set_track_index(None)
    h.close()
    api.bgzf_write_eof(grown)
    whole.write_tbi(grown + ".tbi")
    both = api.TrackIndex()
    with open(joined, "wb") as out:
        for k, ix in enumerate(parts):
            both.append(ix, out.tell())
            with open(f"{joined}.part.{k}", "rb") as f:
                out.write(f.read())
    api.bgzf_write_eof(joined)
    both.write_tbi(joined + ".tbi")
    res = []
    for path in (grown, joined):
        data = open(path, "rb").read()
        res.append(dict(data=data, index=tx.parse_index(path + ".tbi"), text=gzip.decompress(data), table=tx.member_table(data)))
    return res


def regions():
    rng = np.random.default_rng(60)
    out = []
    for name, n, _ in CHROMS:
        for _ in range(20):                                   # 60 seeded regions in all
            a = int(rng.integers(0, n))
            out.append((name, a, min(n, a + int(rng.choice([1, 10, 1_000, 20_000])))))
        for p in (0, 16_383, 16_384, n - 1):
            out.append((name, p, p + 1))
        out += [(name, 0, n), (name, 16_383, 16_385), (name, n, n + 100), (name, 0, 2**29)]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("which", [0, 1], ids=["appended", "joined_parts"])
def test_queries_return_exactly_the_overlapping_lines(files, which):
    f = files[which]
    bw.check_file(f["data"], f["text"])
    assert f["text"] == files[0]["text"] and f["text"].count(b"\n") > 10_000
    assert f["index"]["names"] == [c[0] for c in CHROMS]
    assert tx.resolved(f["index"], f["table"]) == {k: dict(chunks=v["chunks"], linear=v["linear"])
                                                    for k, v in tx.expected_index(f["text"], f["table"]).items()}
    for name, beg, end in regions():
        lines, touched = tx.query(f["data"], f["index"], name, beg, end, f["table"])
        assert lines == tx.overlapping(f["text"], name, beg, end), (name, beg, end)
        # no member outside the chunks of the bins that can hold such a line
        ref = f["index"]["refs"][f["index"]["names"].index(name)]
        allowed = set()
        for b in tx.reg2bins(beg, min(end, 2**29)):
            for x, y in ref["bins"].get(b, []):
                tx.text_range(f["table"], tx.resolve(x, f["table"]), tx.resolve(y, f["table"]), allowed)
        assert touched <= allowed and (lines == [] or touched)
    assert tx.query(f["data"], f["index"], "chrZ", 0, 1000, f["table"]) == ([], set())


@pytest.mark.gpu
def test_both_files_hold_the_same_index(files):
    """Appended in place or joined from parts: the same bytes of data, the same index."""
    assert files[0]["data"] == files[1]["data"]
    for a, b in zip(files[0]["index"]["refs"], files[1]["index"]["refs"]):
        assert a["bins"] == b["bins"] and a["linear"] == b["linear"]
