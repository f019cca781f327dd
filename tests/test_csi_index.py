"""CSI indexes written by the library: the device tables for any level scheme (snf_csi_run, csrc/snf_bamindex.h), the CSIv1 writer
and its loffset rule (bamindex.csi_bytes), bam.index_bam(fmt="csi") for references beyond 2^29 bases, and
bgzfout.VcfGzWriter(index="csi") - exact comparisons against the restatements of tests/csi_cases.py, against the indexes htslib
wrote for the golden files, and against the whole-file path (bam.read_bam).  Every device check runs on the host tier and, marked
gpu, through the real library."""
import functools
import gzip
import io
import json
import os
import struct

import numpy as np
import pytest

import bam_index_cases as K
import bgzf_cases as B
import csi_cases as Q
from sniffles_amd import abi, bam, bamindex, bgzfout, pipeline
from sniffles_amd.config import SnifflesConfig

GOLDEN = K.GOLDEN
COLUMNS = ("end", "bin", "vbeg", "vend", "runs", "win_index", "win_min")


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def tier(request, monkeypatch):
    for k in ("SNF_BGZF_GRID", "SNF_BGZF_THREAD", "SNF_BAI_GRID", "SNF_BAI_THREAD"):
        monkeypatch.delenv(k, raising=False)
    if request.param == "emu":
        import emu.emu as E
        E.lib()
    return request.param


@pytest.fixture
def zdev(tier):
    z = bam.BgzfDevice(0)
    yield z
    z.close()


def set_form(monkeypatch, form):
    if form == "thread":
        monkeypatch.setenv("SNF_BAI_THREAD", "1")
    elif form != "wave":
        monkeypatch.setenv("SNF_BAI_GRID", form)


def run_tables(z, data, scheme, carry=None, win_shift=None):
    """One run over a whole file: the tables of snf_csi_run (scheme None: of snf_bai_run), the members and their file offsets.
    `win_shift`: the shift of the window table where the scheme's own is not one."""
    mem = bam.bgzf_members(data)
    foff = bam.member_file_offsets(mem)
    names, lens, hlen = bam.leading_header(data)
    z.inflate(data, mem, header_len=hlen)
    if scheme is None:
        return z.bai_run(foff, bam.window_offsets(lens), carry), mem, foff
    return z.csi_run(foff, bam.window_offsets(lens, scheme[0] if win_shift is None else win_shift), carry, *scheme), mem, foff


def check_against_rules(z, recs, borders, scheme, names=Q.NAMES, lens=Q.LENS):
    raw, hlen, starts = K.stream_of(recs, names, lens)
    data = B.reblock(raw, borders)
    b, mem, foff = run_tables(z, data, scheme)
    exp = Q.expected_tables(recs, starts, mem, foff, *scheme)
    assert b["n"] == len(recs)
    got = list(zip(b["end"].tolist(), b["bin"].tolist(), b["vbeg"].tolist(), b["vend"].tolist()))
    wrong = [(i, g, e) for i, (g, e) in enumerate(zip(got, exp)) if g != e]
    assert not wrong, wrong[:5]
    assert [[k >> 32, k & 0xffffffff, a, e] for k, a, e in b["runs"].tolist()] == K.naive_runs(recs, exp)
    assert dict(zip(b["win_index"].tolist(), b["win_min"].tolist())) == Q.naive_linear(recs, exp, lens, scheme[0])
    assert b["head_n"] == 0
    return b, exp, data


def write_bam(tmp_path, name, recs, names, lens, cuts=700):
    raw, hlen, starts = K.stream_of(recs, names, lens)
    data = B.reblock(raw, list(range(cuts, len(raw), cuts)))
    p = tmp_path / name
    p.write_bytes(data)
    return str(p), raw, hlen, starts, data


# ------------------------------------------------------------------------------------------- 1. bins at every level's border
@functools.lru_cache(None)
def border_table(scheme):
    return Q.border_table(*scheme)


@pytest.mark.parametrize("form", ["wave", "thread", "1", "2", "7"])
@pytest.mark.parametrize("scheme", Q.SCHEMES, ids=lambda s: f"{s[0]}_{s[1]}")
def test_bins_at_every_level_border(zdev, scheme, form, monkeypatch):
    set_form(monkeypatch, form)
    ms, depth = scheme
    labelled = border_table(scheme)
    recs = [r for _, r in labelled]
    raw, hlen, starts = K.stream_of(recs, Q.NAMES, Q.LENS)
    b, exp, data = check_against_rules(zdev, recs, [starts[7] + 3, starts[30]], scheme)
    by = dict(zip([a for a, _ in labelled], exp))
    leaf0 = ((1 << (3 * depth)) - 1) // 7
    assert by["top_across_a"][1] == 0 and by["top_across_b"][1] == 0
    pos = {a: K.fields(r)[1] for a, r in labelled}
    for l in range(depth):
        s = ms + 3 * l
        first = ((1 << (3 * (depth - l))) - 1) // 7                        # first bin of the level whose bins have 2^s bases
        above = ((1 << (3 * (depth - l - 1))) - 1) // 7
        Bd = pos[f"l{l}_base_0"]
        assert by[f"l{l}_base_-1"][1] == leaf0 + ((Bd - 1) >> ms) and by[f"l{l}_base_0"][1] == leaf0 + (Bd >> ms)
        assert by[f"l{l}_ends_-1"][1] == by[f"l{l}_ends_0"][1] == leaf0 + ((Bd - 10) >> ms)      # `end - 1` keeps them in the leaf
        assert by[f"l{l}_ends_1"][1] == by[f"l{l}_across"][1] == above + ((Bd - 1) >> (s + 3)), l   # across a 2^s border: the level above
        assert first + (Bd >> s) != by[f"l{l}_across"][1]
    assert by["ref_length_zero"][0] == pos["ref_length_zero"] + 1 and by["flag_unmapped_with_position"][0] == pos["flag_unmapped_with_position"] + 1
    assert by["unplaced"][:2] == (0, leaf0 - 1)
    if depth == 6:
        assert by["at_2_31_minus_2"][0] == (1 << 31) - 1
        lo, hi = by["around_2_29_-2"][1], by["around_2_29_0"][1]
        assert lo == leaf0 + (((1 << 29) - 2) >> ms) and hi == leaf0 + ((1 << 29) >> ms) and by["around_2_29_-1"][1] not in (lo, hi)
    if scheme == (14, 5):                  # the instance with the BAI's scheme: what snf_bai_run returns, field for field
        want, _, _ = run_tables(zdev, data, None)
        for k in COLUMNS:
            assert np.array_equal(b[k], want[k]), k
        assert (b["head_n"], b["head_end"], b["n"]) == (want["head_n"], want["head_end"], want["n"])
        for k in ("count", "have_prev", "prev_ref", "prev_pos", "prev_bin"):
            assert getattr(b["carry"], k) == getattr(want["carry"], k), k


# ------------------------------------------------------------------------------------------- 2. window minima at the shift
@pytest.mark.parametrize("form", ["wave", "thread", "2"])
@pytest.mark.parametrize("scheme", [(12, 6), (16, 4)], ids=lambda s: f"{s[0]}_{s[1]}")
def test_window_minima_at_the_shift(zdev, scheme, form, monkeypatch):
    set_form(monkeypatch, form)
    recs = Q.windows_table(scheme[0])
    raw, hlen, starts = K.stream_of(recs, Q.NAMES, Q.LENS)
    b, exp, _ = check_against_rules(zdev, recs, [starts[3] + 5, starts[9]], scheme)
    lin = Q.naive_linear(recs, exp, Q.LENS, scheme[0])
    assert len(lin) >= 65 + 6 and b["win_index"].shape[0] == len(lin)
    wo = bam.window_offsets(Q.LENS, scheme[0])
    assert int(wo[1]) == ((Q.LONG - 1) >> scheme[0]) + 1
    assert lin[0] == exp[1][2] and 0 not in [w for w, v in lin.items() if v == exp[0][2]]      # the flagged read touches no window
    k = int(wo[1])                                                                             # second reference: its own windows, each read over two
    assert lin[k] == lin[k + 1] == exp[10][2] and lin[k + 2] == exp[11][2] and lin[k + 6] == exp[15][2] and k + 7 not in lin


# -------------------------------------------------------------------------------------------------- 3. loffset and structure
def test_csi_depth_follows_htslib_s_rule():
    assert bamindex.csi_depth(248_956_422) == 5 and bamindex.csi_depth((1 << 29) - 256) == 5 and bamindex.csi_depth((1 << 29) - 255) == 6
    assert bamindex.csi_depth(1 << 30) == 6 and bamindex.csi_depth((1 << 31) - 1) == 6 and bamindex.csi_depth(5_000_000) == 3
    assert bamindex.csi_depth(1 << 30, 12) == 7 and bamindex.csi_depth(100) == 0 and bamindex.csi_depth((1 << 14) - 255) == 1
    for name in ("hg002", "hg008"):
        ix = bamindex.read_index(os.path.join(GOLDEN, name + ".bam.csi"))
        lens = bam.leading_header(open(os.path.join(GOLDEN, "hg002.bam"), "rb").read())[1]
        assert bamindex.csi_depth(max(lens), ix.min_shift) == ix.depth == 5


def test_loffset_and_structure_of_a_built_index(tier, tmp_path):
    recs, names, lens = Q.holes_table()
    path, raw, hlen, starts, data = write_bam(tmp_path, "h.bam", recs, names, lens, cuts=300)
    mem = bam.bgzf_members(data)
    exp = Q.expected_tables(recs, starts, mem, bam.member_file_offsets(mem), 14, 3)
    refs, n_no_coor = Q.naive_csi(recs, exp, lens, 14, 3)
    out = tmp_path / "h.bam.csi"
    ix = bam.index_bam(path, out=str(out), fmt="csi")
    assert (ix.fmt, ix.min_shift, ix.depth, ix.n_no_coor) == ("csi", 14, 3, 1)
    assert ix == Q.as_index(refs, n_no_coor, 14, 3)
    assert Q.check_bgzf_file(out.read_bytes()) == Q.csi_raw(refs, n_no_coor, 14, 3)
    assert bamindex.read_index(str(out)) == ix and bamindex.parse_index(bamindex.csi_bytes(ix)) == ix
    # the cases the table is built for
    bins0, loff0, meta0 = refs[0]
    a, b2, c = exp[0][2], exp[3][2], exp[4][2]
    assert loff0[10] == a and 10 in bins0                      # windows 8 .. 15, the first one a hole: the value of window 9
    assert loff0[1] == a and loff0[73 + 40] == exp[2][2] and loff0[73 + 9] == a
    assert loff0[73 + 200] == 0 and bins0[73 + 200] == [[c, exp[4][3]]]      # behind the last known window
    assert refs[1] == ({}, {}, None) and ix.refs[1].meta is None and ix.refs[1].bins == {}
    assert refs[3][1] == {73 + 5: 0} and refs[3][2][2:] == (0, 1) and meta0[2:] == (4, 1)
    assert ix.mapped == 5 and b2 > a
    with pytest.raises(ValueError, match="no loffset table"):
        bamindex.csi_bytes(bamindex.BamIndex([bamindex.RefIndex({5: np.array([[1, 2]], np.uint64)}, np.zeros(0, np.uint64))], 0, "csi"))


def test_a_csi_of_several_members_round_trips():
    rng = np.random.default_rng(5)
    refs = []
    for i in range(3):
        bins = {int(b): np.sort(rng.integers(1, 1 << 40, (int(rng.integers(1, 4)), 2), dtype=np.uint64), axis=1)
                for b in rng.choice(bamindex.meta_bin(6) - 1, 2500, replace=False)}
        refs.append(bamindex.RefIndex(bins, None, {b: int(rng.integers(0, 1 << 40)) for b in bins}, (1, 2, 3 + i, 4) if i != 1 else None))
    refs.append(bamindex.RefIndex({}, None, {}, None))
    ix = bamindex.BamIndex(refs, 7, "csi", 12, 6, aux=b"some aux bytes")
    data = bamindex.csi_bytes(ix)
    raw = Q.check_bgzf_file(data)
    assert len(raw) > 2 * 0xff00 and bam.bgzf_members(data).shape[0] >= 4
    back = bamindex.parse_index(data)
    assert back == ix and (back.aux, back.fmt, back.n_no_coor) == (b"some aux bytes", "csi", 7)
    assert raw == Q.csi_raw([({b: c.tolist() for b, c in r.bins.items()}, r.loffset, r.meta) for r in refs], 7, 12, 6, b"some aux bytes")


@functools.lru_cache(None)
def sample():
    return K.sample_file()


def test_three_runs_give_the_bytes_of_one(tier, tmp_path):
    data, names, lens, recs = sample()
    p = tmp_path / "s.bam"
    p.write_bytes(data)
    st = {}
    one = bam.index_bam(str(p), out=str(p) + ".csi", stats=st, fmt="csi")
    assert st["runs"] == 1 and (one.min_shift, one.depth) == (14, 2)
    want = (tmp_path / "s.bam.csi").read_bytes()
    for run_bytes in (len(data) // 3 + 1000, 9000):
        st = {}
        ix = bam.index_bam(str(p), out=str(tmp_path / "x.csi"), run_bytes=run_bytes, stats=st, fmt="csi")
        assert st["runs"] >= 3 and (tmp_path / "x.csi").read_bytes() == want and ix == one
    raw, hlen, starts = K.stream_of(recs, names, lens)
    mem = bam.bgzf_members(data)
    exp = Q.expected_tables(recs, starts, mem, bam.member_file_offsets(mem), 14, 2)
    assert Q.check_bgzf_file(want) == Q.csi_raw(*Q.naive_csi(recs, exp, lens, 14, 2), 14, 2)
    other = bam.index_bam(str(p), fmt="csi", min_shift=12)
    assert (other.min_shift, other.depth) == (12, 3)
    exp = Q.expected_tables(recs, starts, mem, bam.member_file_offsets(mem), 12, 3)
    assert other == Q.as_index(*Q.naive_csi(recs, exp, lens, 12, 3), 12, 3)


# ------------------------------------------------------------------------------------------------------------ 4. completeness
def fetched_offsets(f, contig, beg, end, offsets, vbeg, ends, ch):
    """Offsets (in the file's record table) of the records a fetch keeps for [beg, end)."""
    d = f.fetch_device(contig, beg, end)
    try:
        assert (d.n == 0) == (ch.shape[0] == 0)
        if not d.n:
            return set()
        first = int(np.nonzero(vbeg == ch[0, 0])[0][0])
        got = d.rec_off[:-1] + int(offsets[first])
        assert np.array_equal(got, offsets[first:first + d.n])
        return set(got[d.keep & (d.pos < end) & (ends[first:first + d.n] > beg)].tolist())
    finally:
        d.close()


def test_every_border_query_through_the_built_csi_is_complete(tier, tmp_path):
    data, names, lens, recs = sample()
    p = tmp_path / "s.bam"
    p.write_bytes(data)
    bam.index_bam(str(p), out=str(p) + ".csi", run_bytes=3000, fmt="csi")
    raw, hlen, starts = K.stream_of(recs, names, lens)
    mem = bam.bgzf_members(data)
    exp = Q.expected_tables(recs, starts, mem, bam.member_file_offsets(mem), 14, 2)
    host = bam.parse_bam(raw)
    ends, vbeg = np.array([e[0] for e in exp]), np.array([e[2] for e in exp], np.uint64)
    mapped = (host.ref_id >= 0) & ((bam.record_flags(host) & 4) == 0)
    offsets = host.rec_off[:-1]
    f = bam.open_indexed(str(p))
    try:
        ix = f.index
        assert ix.fmt == "csi" and ix.refs[0].loffset and ix.mapped == int(mapped.sum())
        for rid, contig in enumerate(names):
            sel = host.ref_id == rid
            qs = Q.border_queries(host.pos[sel & mapped], ends[sel & mapped], 14)
            assert len(qs) > 100
            # the host tier fetches for the set tests/test_bam_index.py uses: the first and the last window border, the borders
            # of the longest stretch without a record, the middle one (a fetch costs about 25 ms there); the GPU for every query
            bs = sorted({a for a, e in qs if e == a + 1 and a % 16384 == 0})
            gap = max(range(len(bs) - 1), key=lambda k: bs[k + 1] - bs[k])
            chosen = {bs[0], bs[-1], bs[gap], bs[gap + 1], bs[len(bs) // 2]}
            near = lambda a, e: any(abs(a - c) <= 1 or abs(e - c) <= 1 for c in chosen)
            n_fetch = 0
            for beg, end in qs:
                want = np.nonzero(sel & mapped & (host.pos < end) & (ends > beg))[0]
                ch = ix.query(rid, beg, end)
                for i in want.tolist():
                    assert any(a <= int(vbeg[i]) < b for a, b in ch.tolist()), (contig, beg, end, i)
                if tier == "gpu" or near(beg, end):
                    assert fetched_offsets(f, contig, beg, end, offsets, vbeg, ends, ch) == set(offsets[want].tolist()), (contig, beg, end)
                    n_fetch += 1
            assert n_fetch >= 30
    finally:
        f.close()


# ----------------------------------------------------------------------------------------------------------- 5. against htslib
def records_in(ch, vbeg):
    keep = np.zeros(vbeg.shape[0], bool)
    for a, b in ch.tolist():
        keep |= (vbeg >= np.uint64(a)) & (vbeg < np.uint64(b))
    return keep


def test_built_csi_against_htslib_s(tier, tmp_path):
    # hg002.bam: the file htslib indexed, so the offsets are comparable and both indexes go through fetch_device
    path = os.path.join(GOLDEN, "hg002.bam")
    theirs = bamindex.read_index(path + ".csi")
    ours = bam.index_bam(path, fmt="csi")
    head = lambda ix: (ix.fmt, ix.min_shift, ix.depth, ix.n_ref, ix.mapped, ix.n_no_coor)
    assert head(ours) == head(theirs) == ("csi", 14, 5, 25, 1, 0)
    # the metadata: equal but for off_end behind the file's last record - htslib names the EOF member that follows it, the tables
    # of the device the byte behind that empty member (a virtual offset here never names a member without bytes; the BAI has the same)
    assert [r.meta and (r.meta[0],) + r.meta[2:] for r in ours.refs] == [r.meta and (r.meta[0],) + r.meta[2:] for r in theirs.refs]
    assert [r.meta[1] for r in ours.refs if r.meta] == [r.meta[1] + (28 << 16) for r in theirs.refs if r.meta] == [os.path.getsize(path) << 16]
    host = bam.read_bam(path)
    raw = bam.bgzf_inflate(open(path, "rb").read())
    recs = [raw[len(raw) - int(host.rec_off[-1]) + int(a):len(raw) - int(host.rec_off[-1]) + int(b)] for a, b in zip(host.rec_off[:-1], host.rec_off[1:])]
    ends = np.array([K.endpos(r) for r in recs])
    fa, fb = bam.open_indexed(path, index=ours), bam.open_indexed(path, index=theirs)
    try:
        for rid in sorted(set(host.ref_id.tolist())):
            sel = host.ref_id == rid
            for beg, end in Q.border_queries(host.pos[sel], ends[sel], 14):
                got = []
                for f in (fa, fb):
                    d = f.fetch_device(host.ref_names[rid], beg, end)
                    got.append(sorted(zip(d.pos[d.keep & (d.pos < end)].tolist(), [d.qname(i) for i in np.nonzero(d.keep & (d.pos < end))[0].tolist()])))
                    d.close()
                want = sorted((int(host.pos[i]), host.qname(i)) for i in np.nonzero(sel & (host.pos < end) & (ends > beg))[0].tolist())
                keep_end = lambda rows: [r for r in rows if r in want]
                assert keep_end(got[0]) == keep_end(got[1]) == want, (rid, beg, end)
    finally:
        fa.close(); fb.close()
    # hg008: the golden stream deflated anew - htslib's offsets belong to the original members (hg008_members.json), so the
    # records a query selects are compared: those that start inside the returned chunks and overlap the interval
    with gzip.open(os.path.join(GOLDEN, "bam_hg008.bam.gz"), "rb") as f:
        raw = f.read()
    p = tmp_path / "hg008.bam"
    p.write_bytes(bam.bgzf_deflate(raw, 6))
    theirs = bamindex.read_index(os.path.join(GOLDEN, "hg008.bam.csi"))
    ours = bam.index_bam(str(p), fmt="csi")
    assert head(ours) == head(theirs) == ("csi", 14, 5, 218, 16, 0)
    assert [r.meta and r.meta[2:] for r in ours.refs] == [r.meta and r.meta[2:] for r in theirs.refs]
    h = bam.parse_bam(raw)
    hlen = len(raw) - int(h.rec_off[-1])
    with open(os.path.join(GOLDEN, "hg008_members.json")) as f:
        mem = json.load(f)
    out_off = np.cumsum([0] + [m[1] for m in mem])
    def their_voff(pp):
        k = int(np.searchsorted(out_off, pp, side="right")) - 1
        return mem[k][0] << 16 | (pp - int(out_off[k]))
    mine = bam.bgzf_members(p.read_bytes())
    foff = bam.member_file_offsets(mine)
    v_theirs = np.array([their_voff(hlen + int(o)) for o in h.rec_off[:-1]], np.uint64)
    v_ours = np.array([K.voffset(mine, foff, hlen + int(o)) for o in h.rec_off[:-1]], np.uint64)
    ends = np.array([K.endpos(raw[hlen + int(a):hlen + int(b)]) for a, b in zip(h.rec_off[:-1], h.rec_off[1:])])
    n = 0
    for rid in sorted(set(h.ref_id.tolist())):
        sel = h.ref_id == rid
        for beg, end in Q.border_queries(h.pos[sel], ends[sel], 14):
            over = sel & (h.pos < end) & (ends > beg)
            a, b = records_in(ours.query(rid, beg, end), v_ours) & over, records_in(theirs.query(rid, beg, end), v_theirs) & over
            assert np.array_equal(a, b) and np.array_equal(a, over), (rid, beg, end)
            n += int(over.sum())
    assert n > 50


# --------------------------------------------------------------------------------------------------- 6. a long contig end to end
def sample_config():
    import vcf_util as vu
    cfg = SnifflesConfig(all_contigs=True)
    for k, v in vu.FIXED.items():
        setattr(cfg, k, v)
    return cfg


@functools.lru_cache(None)
def long_sample():
    names, lens, recs, places = Q.long_contig_sample()
    raw, hlen, starts = K.stream_of(recs, names, lens)
    return B.reblock(raw, list(range(15000, len(raw), 15000))), names, lens, recs, places


def long_files(tmp_path):
    data, names, lens, recs, places = long_sample()
    p = tmp_path / "long.bam"
    p.write_bytes(data)
    return str(p), names, lens, recs, places


def test_a_contig_of_2_30_bases_is_indexed_and_fetched(tier, tmp_path):
    path, names, lens, recs, places = long_files(tmp_path)
    assert lens[0] == 1 << 30
    with pytest.raises(ValueError, match=r"BAI cannot hold reference 0 of 1073741824 bases: its bins end at 2\^29 \(a CSI index can\)"):
        bam.index_bam(path, out=path + ".bai")
    st = {}
    ix = bam.index_bam(path, out=path + ".csi", fmt="csi", run_bytes=100_000, stats=st)
    assert (ix.fmt, ix.min_shift, ix.depth) == ("csi", 14, 6) and st["runs"] > 2
    assert bamindex.find_index(path) == path + ".csi" and bamindex.read_index(path + ".csi") == ix
    host = bam.read_bam(path)
    ends = np.array([K.endpos(r) for r in recs])
    mapped = (host.ref_id >= 0) & ((bam.record_flags(host) & 4) == 0)
    assert ix.mapped == int(mapped.sum()) and int(host.pos.max()) > (1 << 30) - 60_000
    assert ((host.pos < 1 << 29) & (ends > 1 << 29)).sum() >= 1                                 # reads across 2^29
    f = bam.open_indexed(path)
    try:
        P = 1 << 29
        for beg, end in [(0, 20_000), (P - 20_000, P), (P - 1, P + 1), (P, P + 20_000), (P - 5000, P + 5000), ((1 << 30) - 30_000, 1 << 30),
                         (100_000, P - 40_000), (None, None)] + [(a + 10_000, a + 10_001) for a, _ in places]:
            d = f.fetch_device("chrLong", beg, end)
            b0, e0 = (0, 1 << 40) if beg is None else (beg, end)
            got = sorted(zip(d.pos[d.keep].tolist(), [d.qname(i) for i in np.nonzero(d.keep)[0].tolist()]))
            d.close()
            want = sorted((int(host.pos[i]), host.qname(i)) for i in np.nonzero((host.ref_id == 0) & mapped & (host.pos < e0) & (ends > b0))[0].tolist())
            assert [g for g in got if g in set(want)] == want, (beg, end)
            assert (len(want) > 3) == ((beg, end) != (100_000, P - 40_000))
    finally:
        f.close()


def test_call_sample_through_the_csi_of_a_long_contig(tier, tmp_path):
    path, names, lens, recs, places = long_files(tmp_path)
    bam.index_bam(path, out=path + ".csi", fmt="csi")
    want = io.StringIO()
    res = pipeline.call_sample(bam.read_bam(path), sample_config(), vcf_handle=want)
    got = io.StringIO()
    f = bam.open_indexed(path)
    try:
        res2 = pipeline.call_sample(f, sample_config(), vcf_handle=got)
    finally:
        f.close()
    assert got.getvalue() == want.getvalue() and res.read_count == res2.read_count
    calls = [ln.split("\t") for ln in want.getvalue().splitlines() if not ln.startswith("#")]
    at = [int(c[1]) for c in calls if c[0] == "chrLong"]
    assert any(p < 60_000 for p in at) and any((1 << 29) - 30_000 < p < 1 << 29 for p in at) and any(1 << 29 <= p < (1 << 29) + 30_000 for p in at)
    assert any(p > (1 << 30) - 60_000 for p in at) and any(c[0] == "chrS" for c in calls)


# ------------------------------------------------------------------------------------------------------ 7. VcfGzWriter(index="csi")
def vcf_text(positions, contig=b"chrL"):
    head = b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"
    lines = []
    for k, (c, pos, ref, info) in enumerate(positions):
        lines.append(b"\t".join([c, str(pos).encode(), b"id%d" % k, ref, b"<DEL>" if b"END" in info else b"A" + b"T" * (k % 5), b"60", b"PASS", info]) + b"\n")
    return head, lines


def tabix_over_csi(lines, head, member_off, depth):
    """The restated tabix-over-CSI index of VCF lines written behind `head`: [(bins, loffset, meta)] per contig and the names.
    beg = POS - 1, end = beg + len(REF) or INFO END; a line's virtual offsets from its place in the uncompressed text and the
    file offsets of the 0xff00-byte members."""
    voff = lambda u: int(member_off[u // 0xff00]) << 16 | (u % 0xff00)
    names, per, u = [], {}, len(head)
    for ln in lines:
        f = ln.rstrip(b"\n").split(b"\t")
        beg = int(f[1]) - 1
        end = beg + len(f[3])
        for kv in f[7].split(b";"):
            if kv.startswith(b"END=") and int(kv[4:]) > beg:
                end = int(kv[4:])
        if f[0] not in names:
            names.append(f[0])
        per.setdefault(f[0], []).append((beg, end, voff(u), voff(u + len(ln))))
        u += len(ln)
    refs = []
    for nm in names:
        rows = per[nm]
        bins, prev = {}, None
        arr = [Q.U64_MAX] * (((max(e for _, e, _, _ in rows) - 1) >> 14) + 1)
        for beg, end, vb, ve in rows:
            b = bamindex.reg2bin(beg, end, 14, depth)
            if b == prev:
                bins[b][-1][1] = ve
            else:
                bins.setdefault(b, []).append([vb, ve])
            prev = b
            for w in range(beg >> 14, ((end - 1) >> 14) + 1):
                arr[w] = min(arr[w], vb)
        for w in range(len(arr) - 2, -1, -1):
            if arr[w] == Q.U64_MAX:
                arr[w] = arr[w + 1]
        loff = {}
        for b in bins:
            l, k = Q.bin_level(b, depth)
            w = k << (3 * (depth - l))
            loff[b] = arr[w] if w < len(arr) else 0
        refs.append((bins, loff, (rows[0][2], rows[-1][3], len(rows), 0)))
    nm = b"".join(n + b"\0" for n in names)
    return refs, struct.pack("<7i", 2, 1, 2, 0, ord("#"), 0, len(nm)) + nm


def lines_of_chunks(data, ch):
    """The text between the virtual offsets of every chunk."""
    mem = bam.bgzf_members(data)
    foff = bam.member_file_offsets(mem)
    raw = bam.bgzf_inflate(data)
    at = lambda v: int(mem["out_off"][int(np.searchsorted(foff[:-1], v >> 16))]) + (v & 0xffff)
    return b"".join(raw[at(int(a)):at(int(b))] for a, b in ch.tolist())


def test_vcf_gz_writer_with_a_csi(tier, tmp_path):
    P, E = 1 << 29, (1 << 31) - 2
    rows = [(b"chrL", 100, b"A", b"SVTYPE=INS"), (b"chrL", 5000, b"N", b"SVTYPE=DEL;END=90000"), (b"chrL", P - 1, b"A", b"."), (b"chrL", P, b"AC", b"."),
            (b"chrL", P + 1, b"A", b"."), (b"chrL", P + 2, b"N", b"SVTYPE=DEL;END=%d" % (P + 400_000)), (b"chrL", E - 5, b"ACGT", b"."), (b"chrL", E, b"A", b"."),
            (b"chrS", 7, b"A", b"."), (b"chrS", 70_000, b"A", b".")]
    head, lines = vcf_text(rows)
    path = str(tmp_path / "long.vcf.gz")
    with pytest.raises(ValueError, match=r"VCF line 6: position 536870913 is beyond 2\^29, the last base a tabix index reaches"):
        with bgzfout.VcfGzWriter(str(tmp_path / "refused.vcf.gz")) as h:
            h.write(head + b"".join(lines))
    with pytest.raises(ValueError, match="neither 'tbi' nor 'csi'"):
        bgzfout.VcfGzWriter(path, index="bai")
    with bgzfout.VcfGzWriter(path, index="csi") as h:
        for ln in [head] + lines:
            h.write(ln)
    assert os.path.exists(path + ".csi") and not os.path.exists(path + ".tbi")
    data = open(path, "rb").read()
    assert bam.bgzf_inflate(data) == head + b"".join(lines)
    raw = Q.check_bgzf_file(open(path + ".csi", "rb").read())
    refs, aux = tabix_over_csi(lines, head, h.member_off, 6)
    assert raw == Q.csi_raw(refs, 0, 14, 6, aux)
    ix = bamindex.read_index(path + ".csi")
    assert (ix.fmt, ix.min_shift, ix.depth, ix.aux) == ("csi", 14, 6, aux) and ix == Q.as_index(refs, 0, 14, 6, aux)
    assert aux[:28] == struct.pack("<7i", 2, 1, 2, 0, 35, 0, 10) and aux[28:] == b"chrL\0chrS\0"
    iv = [(int(r[1]) - 1, max(int(r[1]) - 1 + len(r[2]), int(r[3].split(b"END=")[1]) if b"END=" in r[3] else 0)) for r in rows]
    for rid, nm in enumerate((b"chrL", b"chrS")):
        for beg, end in [(0, 1), (99, 100), (100, 101), (4000, 95000), (P - 3, P - 2), (P - 2, P - 1), (P - 1, P), (P, P + 1), (P + 1, P + 2), (P - 10, P + 10),
                         (P + 300_000, P + 300_001), (E - 10, E), (E - 1, E), (E - 2, E - 1), (0, 1 << 32), (6, 7), (69_999, 70_000), (1 << 30, (1 << 30) + 5)]:
            text = lines_of_chunks(data, ix.query(rid, beg, end))
            for k, (r, (b0, e0)) in enumerate(zip(rows, iv)):
                if r[0] == nm and b0 < end and e0 > beg:
                    assert lines[k] in text, (nm, beg, end, k)
            assert all(ln + b"\n" in lines for ln in text.split(b"\n")[:-1])      # whole lines of the file, nothing else
    # records all below 2^29: the .tbi and the .csi answer the same queries
    low = [r for r in rows if iv[rows.index(r)][1] < P]
    head, lines = vcf_text(low)
    a, b = str(tmp_path / "a.vcf.gz"), str(tmp_path / "b.vcf.gz")
    for p_, kind in ((a, "tbi"), (b, "csi")):
        with bgzfout.VcfGzWriter(p_, index=kind) as h:
            h.write(head + b"".join(lines))
    assert open(a, "rb").read() == open(b, "rb").read()
    tbi = bam.bgzf_inflate(open(a + ".tbi", "rb").read())
    csi = bamindex.read_index(b + ".csi")
    assert csi.depth == 5 and csi.aux == tbi[8:36] + tbi[36:36 + struct.unpack_from("<i", tbi, 32)[0]]
    as_bai = bamindex.parse_index(b"BAI\x01" + tbi[4:8] + tbi[36 + struct.unpack_from("<i", tbi, 32)[0]:])      # the .tbi behind its header is a BAI body
    for rid in range(2):
        assert as_bai.refs[rid].meta == csi.refs[rid].meta and sorted(as_bai.refs[rid].bins) == sorted(csi.refs[rid].bins)
        for beg, end in [(0, 1), (99, 100), (100, 101), (4000, 95000), (89_999, 90_000), (90_000, 90_001), (0, P), (P - 2, P - 1), (6, 7), (69_999, 70_000)]:
            assert lines_of_chunks(open(a, "rb").read(), as_bai.query(rid, beg, end)) == lines_of_chunks(open(b, "rb").read(), csi.query(rid, beg, end))


# ---------------------------------------------------------------------------------------------------------------- 8. refusals
def test_parameters_out_of_range_are_refused_and_the_handle_stays_usable(zdev):
    recs = [K.rec(0, 100 + k, [(K.M, 10)], name=f"g{k}") for k in range(8)] + [K.rec(1, 50 + k, [(K.M, 10)], name=f"h{k}") for k in range(4)]
    raw, hlen, starts = K.stream_of(recs, Q.NAMES, Q.LENS)
    data = B.reblock(raw, [starts[2] + 7])
    assert (abi.CSI_MIN_SHIFT, abi.CSI_DEPTH, abi.CSI_TOP_BITS) == ((8, 30), (1, 10), 40)
    for ms, depth in ((7, 5), (31, 1), (14, 0), (14, 11), (-1, 5), (14, -3), (30, 4), (11, 10), (20, 7)):
        with pytest.raises(ValueError, match=f"snf_csi_run: min_shift {ms} / depth {depth} out of range"):
            run_tables(zdev, data, (ms, depth), win_shift=14)
        b, _, _ = run_tables(zdev, data, (14, 6))
        assert b["n"] == len(recs) and b["runs"].shape[0] == 2
    for ms, depth in ((8, 1), (8, 10), (30, 1), (10, 10), (28, 4)):      # the corners that are accepted
        check_against_rules(zdev, recs, [starts[2] + 7], (ms, depth))


@pytest.mark.parametrize("form", ["1", "wave", "thread"])
def test_unsorted_and_truncated_records_are_refused_in_the_bai_path_s_words(zdev, form, monkeypatch):
    set_form(monkeypatch, form)
    good = [K.rec(0, 100 + k, [(K.M, 10)], name=f"g{k}") for k in range(8)] + [K.rec(1, 50 + k, [(K.M, 10)], name=f"h{k}") for k in range(4)]
    def refusal(recs, scheme):
        raw, hlen, starts = K.stream_of(recs, Q.NAMES, Q.LENS)
        with pytest.raises(ValueError) as e:
            run_tables(zdev, B.reblock(raw, [starts[2] + 7]), scheme)
        return str(e.value)
    cases = []
    x = list(good); x[3] = K.rec(0, 99, [(K.M, 10)], name="b"); x[6] = K.rec(0, 3, [(K.M, 10)], name="b2")
    cases.append((x, "BAM not coordinate-sorted: record 3 (reference 0, position 99) lies before its predecessor's position"))
    x = list(good); x[9] = K.rec(0, 5000, [(K.M, 10)], name="b")
    cases.append((x, "BAM not coordinate-sorted: record 9 (reference 0, position 5000) follows a record of a later reference"))
    x = good[:5] + [K.rec(-1, -1, [], flag=0x4, name="u")] + good[5:]
    cases.append((x, "BAM not coordinate-sorted: record 6 (reference 0, position 105) follows an unplaced record"))
    x = list(good); x[4] = K.rec(7, 104, [(K.M, 10)], name="b")
    cases.append((x, "BAM not coordinate-sorted: record 4 (reference 7, position 104) names a reference the header does not have"))
    x = list(good)
    for k in (5, 10):
        bad = bytearray(x[k]); struct.pack_into("<H", bad, 16, 2000); x[k] = bytes(bad)
    cases.append((x, f"truncated BAM record at byte {K.stream_of(x, Q.NAMES, Q.LENS)[2][5]}"))
    for recs, words in cases:
        assert refusal(recs, (14, 6)) == refusal(recs, None) == words
    raw, hlen, starts = K.stream_of(good, Q.NAMES, Q.LENS)
    b, _, _ = run_tables(zdev, B.reblock(raw, [starts[2] + 7]), (12, 6))
    assert b["n"] == len(good)


def test_index_bam_refuses_what_it_cannot_build(tier, tmp_path):
    data, names, lens, recs = sample()
    p = tmp_path / "s.bam"
    p.write_bytes(data)
    with pytest.raises(ValueError, match="neither 'bai' nor 'csi'"):
        bam.index_bam(str(p), fmt="tbi")
    for ms in (7, 31, -2):
        with pytest.raises(ValueError, match=f"min_shift {ms} outside 8 .. 30"):
            bam.index_bam(str(p), fmt="csi", min_shift=ms)
    swapped = list(recs)
    swapped[150], swapped[151] = swapped[151], swapped[150]
    raw2 = K.stream_of(swapped, names, lens)[0]
    p.write_bytes(B.reblock(raw2, list(range(700, len(raw2), 700))))
    for rb in (256 << 20, 1500):
        with pytest.raises(ValueError, match="BAM not coordinate-sorted: record 151 "):
            bam.index_bam(str(p), run_bytes=rb, fmt="csi")
