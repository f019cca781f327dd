"""BAM indexes: the host reader / query / writer (sniffles_amd/bamindex.py), the index built on the device (csrc/snf_bamindex.h,
bam.index_bam) and the fetch through an index (bam.open_indexed) - exact comparisons against a restatement of the SAM
specification's rules (tests/bam_index_cases.py), against indexes htslib wrote, and against the whole-file path (bam.read_bam).
Every device check runs on the host tier and, marked gpu, through the real library."""
import functools
import gzip
import io
import json
import os
import shutil
import struct

import numpy as np
import pytest

import bam_index_cases as K
import bgzf_cases as B
import cases
import snf_util as su
from sniffles_amd import bam, bamindex, extract, pipeline, snf, sv
from sniffles_amd.config import SnifflesConfig

GOLDEN = K.GOLDEN


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


def task_inputs_equal(a, b):
    for k in a.leads:
        assert np.array_equal(a.leads[k], b.leads[k], equal_nan=a.leads[k].dtype.kind == "f"), k
    for k in ("seq_pool", "read_start", "read_end", "read_hp"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    for k in ("contig", "contig_len", "qc_nm_threshold", "qnames", "ps_names", "contig_names"):
        assert getattr(a, k) == getattr(b, k), k


def sample_config():
    import vcf_util as vu
    cfg = SnifflesConfig(all_contigs=True)
    for k, v in vu.FIXED.items():      # (command line and start date of the VCF header)
        setattr(cfg, k, v)
    return cfg


def tables(z, data, carry=None):
    """One run over a whole file: (inflate result, index tables, members, file offsets)."""
    mem = bam.bgzf_members(data)
    foff = bam.member_file_offsets(mem)
    names, lens, hlen = bam.leading_header(data)
    r = z.inflate(data, mem, header_len=hlen)
    return r, z.bai_run(foff, bam.window_offsets(lens), carry), mem, foff


def check_against_rules(z, recs, borders, names=K.NAMES, lens=K.LENS):
    raw, hlen, starts = K.stream_of(recs, names, lens)
    data = B.reblock(raw, borders)
    r, b, mem, foff = tables(z, data)
    exp = K.expected_tables(recs, starts, mem, foff)
    assert b["n"] == len(recs)
    got = list(zip(b["end"].tolist(), b["bin"].tolist(), b["vbeg"].tolist(), b["vend"].tolist()))
    wrong = [(i, g, e) for i, (g, e) in enumerate(zip(got, exp)) if g != e]
    assert not wrong, wrong[:5]
    runs = K.naive_runs(recs, exp)
    assert [[k >> 32, k & 0xffffffff, a, e] for k, a, e in b["runs"].tolist()] == runs
    lin = K.naive_linear(recs, exp, bam.window_offsets(lens))
    assert dict(zip(b["win_index"].tolist(), b["win_min"].tolist())) == lin
    assert b["head_n"] == 0
    return b, exp, (raw, hlen, starts, data)


# ------------------------------------------------------------------------------------------------------ 1. real indexes
def test_the_reference_s_csi_files_read_as_htslib_wrote_them():
    a, b = bamindex.read_index(os.path.join(GOLDEN, "hg002.bam.csi")), bamindex.read_index(os.path.join(GOLDEN, "hg008.bam.csi"))
    assert (a.fmt, a.min_shift, a.depth, a.n_ref, a.mapped, a.n_no_coor) == ("csi", 14, 5, 25, 1, 0)
    assert (b.fmt, b.min_shift, b.depth, b.n_ref, b.mapped, b.n_no_coor) == ("csi", 14, 5, 218, 16, 0)
    assert [b.contig_mapped(i) for i in (0, 17, 22)] == [4, 8, 4] and sum(b.contig_mapped(i) for i in range(218)) == 16
    assert a.refs[0].meta[2:] == (1, 0) and [i for i, r in enumerate(b.refs) if r.meta] == [0, 17, 22]
    assert b.refs[0].bins[95].tolist() == [[0xffc0000, 0x3216a0000]] and b.refs[0].bins[762].tolist() == [[0x3216a0000, 0x55d990000]]
    # every chunk border is a record border of the golden stream, through the member table of the original file
    with open(os.path.join(GOLDEN, "hg008_members.json")) as f:
        mem = json.load(f)
    assert len(mem) == 59
    out_off = np.cumsum([0] + [m[1] for m in mem])
    with gzip.open(os.path.join(GOLDEN, "bam_hg008.bam.gz"), "rb") as f:
        raw = f.read()
    h = bam.parse_bam(raw)
    hlen = len(raw) - int(h.rec_off[-1])
    borders = set((h.rec_off + hlen).tolist())
    by_off = {m[0]: k for k, m in enumerate(mem)}
    n = 0
    for r in b.refs:
        for ch in list(r.bins.values()) + ([np.array([r.meta[:2]], np.uint64)] if r.meta else []):
            for v in ch.reshape(-1).tolist():
                assert int(out_off[by_off[v >> 16]]) + (v & 0xffff) in borders, hex(v)
                n += 1
    assert n >= 18
    # records 0, 2 and 4 are where the first chunks begin and end
    def voff(p):
        k = int(np.searchsorted(out_off, p, side="right")) - 1
        return mem[k][0] << 16 | (p - int(out_off[k]))
    assert [voff(hlen + int(h.rec_off[i])) for i in (0, 2, 4)] == [0xffc0000, 0x3216a0000, 0x55d990000]
    # whole-contig queries have the hull of the metadata bin; contigs without reads give nothing
    for i, r in enumerate(b.refs):
        q = b.query(i)
        assert (q.shape[0] == 0) == (r.meta is None)
        if r.meta:
            assert (int(q[0, 0]), int(q[-1, 1])) == r.meta[:2]


def test_hg002_through_its_csi(tier):
    case = cases.EXTRACT["extract_hg002_chr1"]
    path = os.path.join(GOLDEN, "hg002.bam")
    assert bamindex.find_index(path) == path + ".csi"
    host = bam.read_bam(path)
    cfg = type("Cfg", (), dict(case["cfg"]))()
    f = bam.open_indexed(path)
    try:
        assert (f.ref_names, f.ref_lens) == (host.ref_names, host.ref_lens) and f.index.mapped == 1
        for region in (case["region"], (0, host.ref_lens[0] - 1)):
            want, wi = extract.extract_region(bam.contig_records(host, "chr1"), "chr1", *region, cfg)
            for d in (f.fetch_device("chr1", *region), f.fetch_device("chr1"), bam.contig_records(f, "chr1")):
                got, gi = extract.extract_region(d, "chr1", *region, cfg)
                d.close()
                task_inputs_equal(want, got)
                assert (gi.read_id, gi.read_count) == (wi.read_id, wi.read_count) and gi.read_count == 1
        for contig in ("chr2", "chrM"):
            d = f.fetch_device(contig)
            assert d.n == 0 and d.info["bytes_read"] == 0
            ti, _ = extract.extract_region(d, contig, 0, host.ref_lens[host.ref_names.index(contig)] - 1, cfg)
            assert ti.n_leads == 0 and ti.n_reads == 0
            d.close()
        d = f.fetch_device("chr1", 0, 1000)      # nothing overlaps: the extraction sees no read of the interval
        ti, _ = extract.extract_region(d, "chr1", 0, 1000, cfg)
        assert ti.n_reads == 0
        d.close()
    finally:
        f.close()


def test_a_missing_index_is_refused_in_the_reference_s_words(tmp_path):
    p = tmp_path / "x.bam"
    shutil.copy(os.path.join(GOLDEN, "hg002.bam"), p)
    with pytest.raises(ValueError, match="Unable to load index for input file .*sorted \\+ indexed"):
        bam.open_indexed(str(p))
    shutil.copy(os.path.join(GOLDEN, "hg002.bam.csi"), tmp_path / "x.bai")      # found under the second name; a CSI by its magic
    assert bamindex.find_index(str(p)) == str(tmp_path / "x.bai")
    f = bam.open_indexed(str(p))
    assert f.index.fmt == "csi"
    f.close()
    with pytest.raises(ValueError, match="218 references"):
        bam.open_indexed(str(p), index=os.path.join(GOLDEN, "hg008.bam.csi"))


def test_truncated_and_inconsistent_indexes_name_the_field(tmp_path):
    ix = bamindex.read_index(os.path.join(GOLDEN, "hg008.bam.csi"))
    for r in ix.refs:
        r.linear, r.loffset = np.zeros(0, np.uint64), None
    data = bamindex.bai_bytes(bamindex.BamIndex(ix.refs, 3))
    assert bamindex.parse_index(data).n_no_coor == 3
    seen = set()
    for cut in range(4, len(data) - 8):
        with pytest.raises(ValueError, match="truncated in ") as e:
            bamindex.parse_index(data[:cut], "x.bai")
        seen.add(str(e.value).split("truncated in ")[1].split(" ")[0])
    assert {"n_ref", "n_bin", "bin", "n_chunk", "chunks", "n_intv"} <= seen, seen
    with pytest.raises(ValueError, match="neither BAI"):
        bamindex.parse_index(b"BAM\x01" + data[4:])
    with open(os.path.join(GOLDEN, "hg002.bam.csi"), "rb") as f:
        raw = bytearray(bam.bgzf_inflate(f.read()))
    for off, what in ((8, "depth"), (16, "n_ref")):
        bad = bytearray(raw)
        struct.pack_into("<i", bad, off, -2)
        with pytest.raises(ValueError, match=what):
            bamindex.parse_index(bam.bgzf_deflate(bytes(bad)))
    with pytest.raises(ValueError, match="truncated in "):
        bamindex.parse_index(bam.bgzf_deflate(bytes(raw[:60])))


# ------------------------------------------------------------------------------------ 2. span and bin, 3. virtual offsets
@functools.lru_cache(None)
def span_table():
    return K.span_table()


@pytest.mark.parametrize("form", ["wave", "thread"])
def test_span_and_bin_of_every_case(zdev, form, monkeypatch):
    if form == "thread":
        monkeypatch.setenv("SNF_BAI_THREAD", "1")
    labelled = span_table()
    step = K.wave_step()
    labels = [a for a, _ in labelled]
    for want in [f"ops_{n}" for n in (0, 1, 63, 64, 65, 127, 128, 129, step - 1, step, step + 1)] + ["only_M", "only_P", "only_X", "all_mixed",
                 "ref_length_zero", "flag_unmapped_with_position", "long_cigar_placeholder", "stale_bin", "border_14_across", "border_26_up_to",
                 "just_below_2_29", "unplaced_2"]:
        assert want in labels, want
    recs = [r for _, r in labelled]
    for label, r in labelled:      # one record at a time (the unplaced ones have no predecessor here)
        check_against_rules(zdev, [r], [])
    b, exp, _ = check_against_rules(zdev, recs, [40000, 90000])      # ... and in one table
    by = dict(zip(labels, exp))
    pos = {a: K.fields(r)[1] for a, r in labelled}
    assert by["ref_length_zero"][0] == pos["ref_length_zero"] + 1 and by["flag_unmapped_with_position"][0] == pos["flag_unmapped_with_position"] + 1
    assert by["long_cigar_placeholder"][0] == pos["long_cigar_placeholder"] + 123456
    assert by["stale_bin"][1] != 1 and K.fields(dict(labelled)["stale_bin"])[4] == 1
    for s, above in ((14, 585), (17, 73), (20, 9), (23, 1), (26, 0)):
        assert by[f"border_{s}_across"][1] == above, s                                 # [k 2^s - 1, k 2^s + 1): the level above s (k = 3: its first bin)
        assert by[f"border_{s}_up_to"][1] == 4681 + (((4 << s) - 2) >> 14), s          # [k 2^s - 2, k 2^s): `end - 1` keeps it in the leaf
    assert by["just_below_2_29"][1] == 4681 + 32767 and by["unplaced_0"][:2] == (0, 4680)


def test_virtual_offsets_at_member_borders(zdev):
    recs = [K.rec(0, 100 + 10 * k, [(K.M, 50)], name=f"v{k}") for k in range(12)]
    recs[6] = K.rec(0, 160, [(K.M, 3)] * 600, name="long")      # long enough to span four members
    raw, hlen, st = K.stream_of(recs)
    assert st[7] - st[6] > 2400
    for borders in ([st[1]],                                       # a record at offset 0 of a member
                    [st[2] + 1], [st[2] - 1],                      # ... at a member's last byte; ending one byte into the next
                    [st[3], st[3]], [st[3], st[3], st[3], st[5]],  # ... exactly at its end, empty members in between
                    [st[4] + 1], [st[4] + 2], [st[4] + 3],         # block_size split 1/3, 2/2, 3/1
                    [st[6] + 100, st[6] + 900, st[6] + 1700],      # one record over four members
                    [hlen], [st[11]], [len(raw)]):
        check_against_rules(zdev, recs, borders)
    b, exp, (_, _, _, data) = check_against_rules(zdev, recs, [st[3], st[3]])
    mem = bam.bgzf_members(data)
    foff = bam.member_file_offsets(mem)
    assert mem["isize"].tolist()[1] == 0 and exp[3][2] == int(foff[2]) << 16 and exp[2][3] == int(foff[2]) << 16      # the empty member is not named
    b, exp, _ = check_against_rules(zdev, recs, [st[2] + 1])
    assert exp[2][2] == st[2] and exp[1][3] == st[2]                    # (the first member lies at file offset 0)
    b, exp, (_, _, _, data) = check_against_rules(zdev, recs, [st[1]])
    assert exp[1][2] == int(bam.member_file_offsets(bam.bgzf_members(data))[1]) << 16 == exp[0][3]
    b, exp, _ = check_against_rules(zdev, recs, [st[6] + 100, st[6] + 900, st[6] + 1700])
    assert len({v >> 16 for v in (exp[6][2], exp[6][3])}) == 2 and exp[6][3] >> 16 > exp[6][2] >> 16


# ------------------------------------------------------------------------------------------------------------- 4. forms
@functools.lru_cache(None)
def windows_file():
    recs = K.windows_table()
    raw, hlen, starts = K.stream_of(recs)
    return recs, B.reblock(raw, [starts[3] + 5, starts[9], starts[15] - 1])


@pytest.mark.parametrize("grid", ["1", "2", "7", "n-1", "n", "unset", "thread"])
def test_forms_give_identical_tables(zdev, grid, monkeypatch):
    recs, data = windows_file()
    n = len(recs)
    _, want, _, _ = tables(zdev, data)
    assert want["n"] == n and want["win_index"].shape[0] >= 65 + 12
    if grid == "thread":
        monkeypatch.setenv("SNF_BAI_THREAD", "1")
    elif grid != "unset":
        monkeypatch.setenv("SNF_BAI_GRID", str({"n-1": n - 1, "n": n}.get(grid, grid)))
    _, got, _, _ = tables(zdev, data)
    for k in ("end", "bin", "vbeg", "vend", "runs", "win_index", "win_min"):
        assert np.array_equal(got[k], want[k]), k
    raw, hlen, starts = K.stream_of(recs)
    check_against_rules(zdev, recs, [starts[3] + 5, starts[9], starts[15] - 1])


# -------------------------------------------------------------------------------------------------------------- 5. runs
def test_chunk_runs(zdev):
    W = 16384
    one = lambda ref, pos, k: K.rec(ref, pos, [(K.M, 10)], name=f"r{k}")
    n = 40
    b, _, _ = check_against_rules(zdev, [one(0, W * k + 5, k) for k in range(n)], [3000])            # every record in a new bin
    assert b["runs"].shape[0] == n
    b, _, _ = check_against_rules(zdev, [one(0, 5 + k, k) for k in range(n)], [3000])                # all in one bin
    assert b["runs"].shape[0] == 1
    two = [one(0, 5 + k, k) for k in range(5)] + [one(1, 5 + k, k) for k in range(5)]                # two references, the same bin number
    b, _, _ = check_against_rules(zdev, two, [])
    assert [(k >> 32, k & 0xffffffff) for k in b["runs"][:, 0].tolist()] == [(0, 4681), (1, 4681)]
    # A B A: a read of two windows (bin 585) between reads of bin 4681, then bin 585 again
    aba = [one(0, 10, 0), K.rec(0, 20, [(K.M, W)], name="b1"), one(0, 30, 2), one(0, 40, 3), K.rec(0, 50, [(K.M, W)], name="b2"), one(0, 60, 5)]
    b, exp, _ = check_against_rules(zdev, aba, [])
    runs = b["runs"].tolist()
    assert [k & 0xffffffff for k, _, _ in runs] == [585, 585, 4681, 4681, 4681]
    assert runs[0][1] < runs[1][1] and runs[2][1] < runs[3][1] < runs[4][1]                          # a bin's chunks in file order
    assert (runs[3][1], runs[3][2]) == (exp[2][2], exp[3][3])
    tail = [one(0, 5, 0), one(0, 6, 1)] + [K.rec(-1, -1, [], flag=0x4, name=f"u{k}") for k in range(4)]
    b, exp, _ = check_against_rules(zdev, tail, [])                                                  # the unplaced tail opens no run
    assert b["runs"].shape[0] == 1 and b["runs"][0, 2] == exp[1][3]
    b, _, _ = check_against_rules(zdev, tail[2:], [])
    assert b["runs"].shape[0] == 0 and b["n"] == 4


def test_the_carry_joins_the_first_chunk_to_the_run_before(zdev):
    recs = [K.rec(0, 5 + k, [(K.M, 10)], name=f"r{k}") for k in range(6)] + [K.rec(0, 16384 * 3 + k, [(K.M, 10)], name=f"s{k}") for k in range(3)]
    raw, hlen, starts = K.stream_of(recs)
    r, b, mem, foff = tables(zdev, B.reblock(raw, []))
    from sniffles_amd import abi
    for prev_bin, head in ((4681, 6), (4682, 0)):
        c = abi.snf_bai_carry_t(count=100, have_prev=1, prev_ref=0, prev_pos=3, prev_bin=prev_bin)
        _, got, _, _ = tables(zdev, B.reblock(raw, []), c)
        assert got["head_n"] == head and got["runs"].shape[0] == (1 if head else 2)
        assert got["head_end"] == (int(b["vend"][5]) if head else 0) and got["carry"].count == 109
        assert (got["carry"].prev_ref, got["carry"].prev_pos, got["carry"].prev_bin) == (0, 16384 * 3 + 2, 4684)
    c = abi.snf_bai_carry_t(count=100, have_prev=1, prev_ref=0, prev_pos=6, prev_bin=4681)
    with pytest.raises(ValueError, match=r"BAM not coordinate-sorted: record 100 \(reference 0, position 5\) lies before its predecessor's position"):
        tables(zdev, B.reblock(raw, []), c)


# --------------------------------------------------------------------------------------------------------- 6. refusals
@pytest.mark.parametrize("grid", ["1", "n", "thread"])
def test_refusals_name_the_first_record_in_file_order(zdev, grid, monkeypatch):
    good = [K.rec(0, 100 + k, [(K.M, 10)], name=f"g{k}") for k in range(8)] + [K.rec(1, 50 + k, [(K.M, 10)], name=f"h{k}") for k in range(4)]
    if grid == "thread":
        monkeypatch.setenv("SNF_BAI_THREAD", "1")
    else:
        monkeypatch.setenv("SNF_BAI_GRID", {"n": "16"}.get(grid, grid))
    def refused(recs, match):
        raw, hlen, starts = K.stream_of(recs)
        with pytest.raises(ValueError, match=match):
            tables(zdev, B.reblock(raw, [starts[2] + 7]))
        return starts
    un = K.rec(-1, -1, [], flag=0x4, name="u")
    x = list(good); x[3] = K.rec(0, 99, [(K.M, 10)], name="b"); x[6] = K.rec(0, 3, [(K.M, 10)], name="b2")      # two offenders: the first is named
    refused(x, r"not coordinate-sorted: record 3 \(reference 0, position 99\) lies before its predecessor's position")
    x = list(good); x[9] = K.rec(0, 5000, [(K.M, 10)], name="b"); x[11] = K.rec(0, 6000, [(K.M, 10)], name="b2")
    refused(x, r"not coordinate-sorted: record 9 \(reference 0, position 5000\) follows a record of a later reference")
    x = good[:5] + [un] + good[5:]
    refused(x, r"not coordinate-sorted: record 6 \(reference 0, position 105\) follows an unplaced record")
    x = list(good); x[4] = K.rec(7, 104, [(K.M, 10)], name="b")
    refused(x, r"not coordinate-sorted: record 4 \(reference 7, position 104\) names a reference the header does not have")
    for field, value in ((16, 2000), (12, 255)):      # n_cigar_op / l_read_name reach past block_size
        x = list(good)
        for k in (5, 10):
            bad = bytearray(x[k])
            if field == 16:
                struct.pack_into("<H", bad, 16, value)
            else:
                bad[12] = value
                bad = bad[:4 + 32 + 20]
                struct.pack_into("<i", bad, 0, len(bad) - 4)
            x[k] = bytes(bad)
        starts = K.stream_of(x)[2]
        refused(x, f"truncated BAM record at byte {starts[5]}$")
    raw, hlen, starts = K.stream_of(good)
    _, b, _, _ = tables(zdev, B.reblock(raw, [starts[2] + 7]))      # the handle stays usable
    assert b["n"] == len(good) and b["runs"].shape[0] == 2


# -------------------------------------------------------------------------------------- 7. several runs, 9. round trip
@functools.lru_cache(None)
def sample():
    return K.sample_file()


@functools.lru_cache(None)
def sample_host():
    data, names, lens, recs = sample()
    raw, hlen, starts = K.stream_of(recs, names, lens)
    mem = bam.bgzf_members(data)
    return raw, hlen, starts, mem, bam.member_file_offsets(mem), bam.parse_bam(raw)


def test_several_runs_give_the_index_of_one(tier, tmp_path):
    data, names, lens, recs = sample()
    raw, hlen, starts, mem, foff, _ = sample_host()
    p = tmp_path / "s.bam"
    p.write_bytes(data)
    st = {}
    one = bamindex.bai_bytes(bam.index_bam(str(p), stats=st))
    assert st["runs"] == 1 and st["peak_stream_len"] == len(raw)
    # a member table whose borders lie inside a block_size field, on a record border and inside a record's data: a run that ends
    # at each of them (run_bytes = the file offset of the member that begins there), then sizes that cut anywhere
    small = B.reblock(raw, sorted([starts[40] + 2, starts[80], starts[120] + 200] + list(range(700, len(raw), 700))))
    p2 = tmp_path / "s2.bam"
    p2.write_bytes(small)
    one2 = bamindex.bai_bytes(bam.index_bam(str(p2)))
    m2 = bam.bgzf_members(small)
    f2 = bam.member_file_offsets(m2)
    cuts = []
    for pos in (starts[40] + 2, starts[80], starts[120] + 200):
        j = int(np.searchsorted(m2["out_off"], pos, side="left"))
        assert int(m2["out_off"][j]) == pos
        cuts.append(int(f2[j]))
    for run_bytes in cuts + [1, 1500, 9000]:
        st = {}
        out = tmp_path / "x.bai"
        ix = bam.index_bam(str(p2), out=str(out), run_bytes=run_bytes, stats=st)
        assert out.read_bytes() == one2, run_bytes
        assert st["runs"] > 1 and st["peak_stream_len"] < len(raw)
        assert bamindex.read_index(str(out)) == ix                      # 9. write_bai / read_index reproduce the index
    # members smaller than a record, a member per run: most runs hold no whole record and have to grow
    tiny = B.reblock(raw, list(range(120, len(raw), 120)))
    assert np.median([len(r) for r in recs]) > 120
    p3 = tmp_path / "s3.bam"
    p3.write_bytes(tiny)
    st = {}
    want = bamindex.bai_bytes(bam.index_bam(str(p3)))
    assert bamindex.bai_bytes(bam.index_bam(str(p3), run_bytes=1, stats=st)) == want and st["runs"] > 100


def test_truncated_and_unsorted_files_are_refused_by_index_bam(tier, tmp_path):
    data, names, lens, recs = sample()
    raw = sample_host()[0]
    p = tmp_path / "t.bam"
    last = len(raw) - len(recs[-1])
    for cut in (raw[:-1], raw[:last + 20]):
        p.write_bytes(B.reblock(cut, list(range(700, len(cut), 700))))
        with pytest.raises(ValueError) as a:
            bam.parse_bam(cut)
        for rb in (256 << 20, 1500):
            with pytest.raises(ValueError) as b:
                bam.index_bam(str(p), run_bytes=rb)
            assert str(a.value) == str(b.value) == f"truncated BAM record at byte {last}"
    p.write_bytes(B.reblock(raw[:last + 2], list(range(700, last, 700))))      # (cut inside the block_size field: the host fails in struct)
    for rb in (256 << 20, 1500):
        with pytest.raises(ValueError, match=f"truncated BAM record at byte {last}$"):
            bam.index_bam(str(p), run_bytes=rb)
    swapped = list(recs)
    swapped[150], swapped[151] = swapped[151], swapped[150]
    assert K.fields(swapped[150])[:2] > K.fields(swapped[151])[:2]
    raw2 = K.stream_of(swapped, names, lens)[0]
    p.write_bytes(B.reblock(raw2, list(range(700, len(raw2), 700))))
    for rb in (256 << 20, 1500):
        with pytest.raises(ValueError, match="BAM not coordinate-sorted: record 151 "):
            bam.index_bam(str(p), run_bytes=rb)
    with pytest.raises(ValueError, match="BAI cannot hold reference 1 of 536870913 bases"):
        bamindex.bai_bytes(bamindex.BamIndex([bamindex.RefIndex(linear=np.zeros(0, np.uint64))] * 2, ref_lens=[1 << 29, (1 << 29) + 1]))


# ------------------------------------------------------------------------------------------------------ 8. completeness
def test_every_query_is_complete_and_reads_only_what_it_needs(tier, tmp_path):
    data, names, lens, recs = sample()
    raw, hlen, starts, mem, foff, host = sample_host()
    assert 250 <= len(recs) <= 400
    p = tmp_path / "s.bam"
    p.write_bytes(data)
    bam.index_bam(str(p), out=str(p) + ".bai", run_bytes=3000)
    ix = bamindex.read_index(str(p) + ".bai")
    flags = bam.record_flags(host)
    mapped = (host.ref_id >= 0) & ((flags & 4) == 0)
    exp = K.expected_tables(recs, starts, mem, foff)
    ends, vbeg = np.array([e[0] for e in exp]), np.array([e[2] for e in exp], np.uint64)
    assert ix.mapped == int(mapped.sum()) and np.max(ends - host.pos) > 3 * 16384
    offsets = host.rec_off[:-1]
    f = bam.open_indexed(str(p))
    try:
        assert f.index == ix
        whole = []
        for rid, contig in enumerate(names):
            sel = host.ref_id == rid
            assert sel.sum() > 50 and ix.contig_mapped(rid) == int((sel & mapped).sum())
            lo, hi = int(host.pos[sel].min()), int(ends[sel].max())
            special = [(None, None), (0, 0), (5, 5), (lens[rid] - 10, lens[rid] + 10 ** 6), (lens[rid] + 5, lens[rid] + 9), (hi, hi + 50000), (0, lo)]
            windows = list(range(lo >> 14, (hi >> 14) + 2))
            border = lambda w: [(w * 16384 + d, w * 16384 + d + 1) for d in (-1, 0, 1)] + \
                               [(max(0, w * 16384 - 20000), w * 16384 + d) for d in (-1, 0, 1)] + \
                               [(w * 16384 + d, w * 16384 + 40000) for d in (-1, 0, 1)]
            qs = special + [q for w in windows for q in border(w)]
            # Every query goes through `fetch_device` on the GPU.  On the host tier a fetch costs about 25 ms (the stand-in inflates
            # the members a fibre per lane), 400 of them per contig are half a minute: there the chunk contract below is still checked
            # for every query, and the fetch for the special intervals and, with each of -1 / 0 / +1 in all three shapes, for the
            # first and the last window of the covered range, the windows around the contig's longest stretch without reads (the
            # last covered one, the first and the last empty one, the first covered one behind it) and the window in the middle.
            covered = np.zeros(windows[-1] + 2, bool)
            for i in np.nonzero(sel & mapped)[0].tolist():
                covered[int(host.pos[i]) >> 14:((int(ends[i]) - 1) >> 14) + 1] = True
            gaps, w = [], windows[0]
            while w <= windows[-1]:
                if not covered[w]:
                    e = w
                    while e + 1 <= windows[-1] and not covered[e + 1]:
                        e += 1
                    if e < windows[-1] - 1:      # (the windows behind the last read are not a stretch between reads)
                        gaps.append((e - w + 1, w, e))
                    w = e + 1
                else:
                    w += 1
            assert gaps and max(gaps)[0] >= 2, gaps
            _, g0, g1 = max(gaps)
            chosen = {windows[0], windows[-1], g0 - 1, g0, g1, g1 + 1, windows[len(windows) // 2]}
            fetched = set(special) | {q for w in chosen for q in border(w)} if tier == "emu" else set(qs)
            for beg, end in qs:
                if beg is not None and beg < 0:
                    continue
                b0, e0 = (0, 1 << 40) if beg is None else (beg, end)
                want = np.nonzero(sel & mapped & (host.pos < e0) & (ends > b0))[0] if e0 > b0 else np.zeros(0, np.int64)
                ch = ix.query(rid, b0, None if beg is None else e0)
                for i in want.tolist():      # the contract: every overlapping record starts inside a chunk
                    assert any(a <= int(vbeg[i]) < b for a, b in ch.tolist()), (contig, beg, end, i)
                if (beg, end) not in fetched:
                    continue
                d = f.fetch_device(contig, beg, end)
                assert (d.n == 0) == (ch.shape[0] == 0)
                if d.n:      # offsets in the file's record table: the first record fetched is the one at the first chunk's beginning
                    first = int(np.nonzero(vbeg == ch[0, 0])[0][0])
                    got = d.rec_off[:-1] + int(offsets[first])
                    assert set(got.tolist()) <= set(offsets.tolist()) and np.array_equal(got, offsets[first:first + d.n])
                    kept = set(got[d.keep & (d.pos < e0) & (ends[first:first + d.n] > b0)].tolist())
                    assert kept == set(offsets[want].tolist()), (contig, beg, end)
                else:
                    assert want.shape[0] == 0
                d.close()
            # the whole contig: exactly the members of [off_beg, off_end)
            ob, oe = ix.refs[rid].meta[:2]
            d = f.fetch_device(contig)
            stop = oe >> 16
            if oe & 0xffff:
                stop = int(foff[int(np.searchsorted(foff, oe >> 16, side="left")) + 1])
            assert d.info["bytes_read"] == stop - (ob >> 16) and d.n == int(sel.sum()) and d.keep.sum() == int((sel & mapped).sum())
            assert int(np.searchsorted(foff, stop, side="left")) - int(np.searchsorted(foff, ob >> 16, side="left")) >= 20
            whole.append(d.info["bytes_read"])
            d.close()
            mid = (lo + hi) // 2
            d = f.fetch_device(contig, mid, mid + 1)
            assert 0 < d.info["bytes_read"] < whole[-1] and d.keep.sum() >= 1
            d.close()
        assert sum(whole) <= len(data)
    finally:
        f.close()


def test_a_bai_with_holes_in_its_linear_index_answers_completely(tmp_path):
    """An index as older writers leave it: windows no record overlaps hold 0.  Host only: the query never drops what it must keep."""
    W = 16384
    recs = [K.rec(0, 100, [(K.M, 50)], name="a"), K.rec(0, 200, [(K.M, 6 * W)], name="long"), K.rec(0, 9 * W + 5, [(K.M, 50)], name="b"),
            K.rec(0, 20 * W + 5, [(K.M, 50)], name="c")]
    raw, hlen, starts = K.stream_of(recs)
    data = B.reblock(raw, [starts[1], starts[2], starts[3]])
    mem = bam.bgzf_members(data)
    foff = bam.member_file_offsets(mem)
    exp = K.expected_tables(recs, starts, mem, foff)
    bins = {}
    for e, bn, vb, ve in exp:
        bins.setdefault(bn, []).append([vb, ve])
    lin = np.zeros(21, np.uint64)
    for k, v in K.naive_linear(recs, exp, [0]).items():
        lin[k] = v
    assert (lin == 0).sum() >= 10
    ix = bamindex.BamIndex([bamindex.RefIndex({b: np.array(c, np.uint64) for b, c in bins.items()}, lin, None,
                                              (exp[0][2], exp[-1][3], 4, 0))], ref_lens=[1 << 29])
    path = tmp_path / "h.bai"
    bamindex.write_bai(ix, str(path))
    back = bamindex.read_index(str(path))
    assert back == ix and back.mapped == 4
    for beg in range(0, 22 * W, W // 2):
        for end in (beg + 1, beg + W, beg + 5 * W):
            q = back.query(0, beg, end)
            for (e, bn, vb, ve), r in zip(exp, recs):
                if K.fields(r)[1] < end and e > beg:
                    assert any(a <= vb < b for a, b in q.tolist()), (beg, end, vb)
    assert back.query(0, 7 * W, 8 * W).shape[0] == 0 or back.query(0, 7 * W, 8 * W)[0, 0] >= exp[1][2]


def test_only_fetched_records_free_their_handle(tier, tmp_path):
    """`close` on a whole-file table or a contig view of it (they share the file's handle) does nothing; on a fetch it frees the contig."""
    data, names, lens, recs = sample()
    d = bam.bam_device(data)
    try:
        v = bam.contig_records(d, "chr21")
        assert not d.owns_handle and not v.owns_handle
        v.close(); d.close()
        assert d.handle.read_stream(0, 4) == b"BAM\x01"
    finally:
        d.handle.close()
    p = tmp_path / "s.bam"
    p.write_bytes(data)
    f = bam.open_indexed(str(p), index=bam.index_bam(str(p)))
    try:
        r = f.fetch_device("chr21")
        v = r.contig_view("chr21")
        assert r.owns_handle and not v.owns_handle and v.n == r.n
        v.close()
        assert len(r.handle.read_stream(0, 4)) == 4
        r.close()
        with pytest.raises(Exception):
            r.handle.read_stream(0, 4)
    finally:
        f.close()


# ------------------------------------------------------------------------------------------------------- 10. end to end
def run_sample(recs, cfg, tmp_path, objects=True, snf_out=True):
    buf = io.StringIO()
    snf_path = tmp_path / "sample.snf"
    res = pipeline.call_sample(recs, cfg, vcf_handle=buf, snf_path=str(snf_path) if snf_out else None, objects=objects)
    blocks = b""
    if snf_out:
        f = snf.SNFile.open(str(snf_path), sample_config())
        blocks = snf_path.read_bytes().split(b"\n", 1)[0] + json.dumps({c: su.file_record(f, c, sv.TYPES) for c, _ in res.contig_lengths},
                                                                        sort_keys=True).encode()
        f.close()
    return buf.getvalue(), blocks, res.read_count, cfg.task_read_id_offset_mult


@functools.lru_cache(None)
def e2e_sample():
    from sniffles_amd import synth_bam
    names, lens, recs = synth_bam.gen_sample(21, ref_names=("chr20", "chr21", "chr22"), ref_lens=(80_000, 70_000, 60_000), cov=8.0,
                                             read_len_mean=6000, site_spacing=9000)[:3]
    raw, hlen, starts = K.stream_of(recs, names, lens)
    first = [starts[k] for k in range(1, len(recs)) if K.fields(recs[k])[0] != K.fields(recs[k - 1])[0]]      # (a member border where the contig changes)
    return B.reblock(raw, sorted(first + list(range(15000, len(raw), 15000)))), len(raw)


_E2E_BAI = {}


def e2e_files(tier, tmp_path):
    """The sample and its BAI (built once per tier by `index_bam`, in several runs) as files; (path, inflated size, file size)."""
    data, raw_len = e2e_sample()
    path = tmp_path / "sample.bam"
    path.write_bytes(data)
    if tier not in _E2E_BAI:
        st = {}
        _E2E_BAI[tier] = bamindex.bai_bytes(bam.index_bam(str(path), run_bytes=60_000, stats=st))
        assert st["runs"] > 2
    (tmp_path / "sample.bam.bai").write_bytes(_E2E_BAI[tier])
    return str(path), raw_len, len(data)


def e2e_config(name):
    cfg = sample_config()
    if name == "regions":
        cfg.regions_by_contig = {"chr20": [("chr20", 10000, 30000), ("chr20", 45000, 70000)], "chr22": [("chr22", 5000, 40000)]}
    if name == "contig":
        cfg.contig = ["chr21"]
    return cfg


@pytest.mark.parametrize("name", ["default", "regions", "contig", "no_objects"])
def test_call_sample_through_the_index_writes_the_same_vcf_and_snf(tier, tmp_path, name):
    path, raw_len, file_len = e2e_files(tier, tmp_path)
    objects = snf_out = name != "no_objects"
    want = run_sample(bam.read_bam(path), e2e_config(name), tmp_path, objects, snf_out)
    f = bam.open_indexed(path)
    try:
        got = run_sample(f, e2e_config(name), tmp_path, objects, snf_out)
        assert want == got
        assert want[2] > 20 and want[0].count("\n") > want[0].count("\n#")          # (reads were counted, records were written)
        read = {}
        for i in f.fetches:
            read[i["contig"]] = read.get(i["contig"], 0) + i["bytes_read"]
        assert max(i["stream_len"] for i in f.fetches) < raw_len / 2                 # three contigs of similar size: below half the file
        if name == "contig":
            assert set(read) == {"chr21"} and len(f.fetches) == 1                    # a filtered-out contig is never read
        elif name == "regions":
            assert set(read) == {"chr20", "chr22"} and len(f.fetches) == 2           # one fetch per contig, over the hull of its regions
            assert sum(read.values()) < file_len
        else:
            assert set(read) == {"chr20", "chr21", "chr22"} and len(f.fetches) == 3 and sum(read.values()) <= file_len
    finally:
        f.close()


@pytest.mark.parametrize("name", ["default", "regions", "contig"])
def test_genotype_vcf_through_the_index(tier, tmp_path, name):
    """`name`: the configurations of the test above.  With regions the fetch goes over the hull of a contig's regions and the
    extraction over the regions themselves; contigs without regions (or outside the filter) are never read."""
    path, raw_len, _ = e2e_files(tier, tmp_path)
    host = bam.read_bam(path)
    buf = io.StringIO()
    pipeline.call_sample(host, sample_config(), vcf_handle=buf)      # (the targets: this sample's own calls on all three contigs)
    out = []
    for make in (lambda: host, lambda: bam.open_indexed(path)):
        recs = make()
        o = io.StringIO()
        cfg = e2e_config(name)
        n = pipeline.genotype_vcf(recs, cfg, io.StringIO(buf.getvalue()), o)
        out.append((n, o.getvalue(), cfg.task_read_id_offset_mult))
        if recs is not host:
            want = {"default": ["chr20", "chr21", "chr22"], "regions": ["chr20", "chr22"], "contig": ["chr21"]}[name]
            assert [i["contig"] for i in recs.fetches] == want and max(i["stream_len"] for i in recs.fetches) < raw_len / 2
            if name == "regions":
                assert [(i["start"], i["end"]) for i in recs.fetches] == [(10000, 70000), (5000, 40000)]
            recs.close()
    assert out[0] == out[1] and out[0][0] > (0 if name == "contig" else 3)
