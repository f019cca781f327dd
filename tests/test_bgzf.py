"""BGZF inflate, record chain and record heads on the device (csrc/snf_bgzf.h, bam.read_bam_device) against the host path
(bam.bgzf_inflate + bam.parse_bam, i.e. zlib): exact comparisons.  Every case runs on the host tier (the unchanged kernels on the
fibre stand-in) and, marked gpu, through the real library.  Builders: tests/bgzf_cases.py."""
import functools
import io
import json
import struct
import zlib

import numpy as np
import pytest

import bgzf_cases as B
import cases
import snf_util as su
from sniffles_amd import bam, extract, lib, pipeline, snf, sv, synth_bam
from sniffles_amd.config import SnifflesConfig


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def tier(request, monkeypatch):
    for k in ("SNF_BGZF_GRID", "SNF_BGZF_THREAD"):
        monkeypatch.delenv(k, raising=False)
    if request.param == "emu":
        import emu.emu as E
        E.lib()
    return request.param


@functools.lru_cache(None)
def good_cases():
    return B.all_good()


@functools.lru_cache(None)
def malformed_cases():
    return B.malformed()


def inflate(z, members):
    """The members as one file through the device: (inflated bytes, result).  The chain skips the whole stream (it is no BAM)."""
    data = b"".join(members)
    mem = bam.bgzf_members(data)
    total = int(mem["isize"].sum())
    r = z.inflate(data, mem, header_len=total)
    assert r["stream_len"] == total and r["n"] == 0 and r["carry"].skip == 0
    return z.read_stream(0, total)


@pytest.fixture
def zdev(tier):
    z = bam.BgzfDevice(0)
    yield z
    z.close()


# ------------------------------------------------------------------------------------------------------ deflate edges
@pytest.mark.parametrize("form", ["wave", "thread"])
def test_every_deflate_edge_one_member_at_a_time(zdev, form, monkeypatch):
    """zlib at levels 0 / 1 / 6 / 9 and with the four strategies over the data kinds, the member sizes, several blocks per member,
    the hand-written streams: each member alone, against zlib.decompress(payload, -15)."""
    if form == "thread":
        monkeypatch.setenv("SNF_BGZF_THREAD", "1")
    names = [n for n, _, _ in good_cases()]
    for want in ("acgt_l0", "bam_l1", "equal_l6", "period63_l9", "period64_rle", "period65_filtered", "random_fixed", "acgt_huff", "size0",
                 "size1", "size65536", "several_blocks", "max_bits", "one_distance_code", "no_distance_code", "repeat16_across_border",
                 "repeat17_across_border", "repeat18_across_border", "repeat16_first_distance", "distance_32768_to_the_end",
                 "match_after_token_62", "match_after_token_63", "match_after_token_64", "tokens_63", "tokens_64", "tokens_65", "tokens_128"):
        assert want in names, want
    wrong = []
    for name, m, raw in good_cases():
        got = inflate(zdev, [m])
        if got != raw:
            k = next((i for i in range(min(len(got), len(raw))) if got[i] != raw[i]), min(len(got), len(raw)))
            wrong.append((name, len(got), len(raw), k))
    assert not wrong, wrong


@functools.lru_cache(None)
def grid_file():
    """The full-length (0xff00 bytes) zlib cases, about 40 members, with empty and tiny members between them."""
    pick = [(n, m, raw) for n, m, raw in good_cases() if len(raw) == 0xff00 and n.rsplit("_", 1)[-1] in ("l1", "l6", "rle", "fixed")]
    pick += [c for c in good_cases() if c[0] in ("size0", "size1", "size65", "size65536", "distance_32768_to_the_end", "several_blocks")]
    assert 38 <= len(pick) <= 44, len(pick)
    return [m for _, m, _ in pick], b"".join(raw for _, _, raw in pick)


@pytest.mark.parametrize("grid", ["1", "2", "7", "n-1", "n", "unset", "thread"])
def test_grids(zdev, grid, monkeypatch):
    """One file of about 40 members; a capped grid makes a wave take several members (its window and tables are reused)."""
    members, raw = grid_file()
    n = len(members)
    if grid == "thread":
        monkeypatch.setenv("SNF_BGZF_THREAD", "1")
    elif grid != "unset":
        monkeypatch.setenv("SNF_BGZF_GRID", str({"n-1": n - 1, "n": n}.get(grid, grid)))
    assert inflate(zdev, members) == raw


# -------------------------------------------------------------------------------------------------- malformed members
@pytest.mark.parametrize("form", ["wave", "thread"])
def test_malformed_members_are_named_and_the_handle_goes_on(zdev, form, monkeypatch):
    if form == "thread":
        monkeypatch.setenv("SNF_BGZF_THREAD", "1")
    g = good_cases()
    filler = [g[1][1], g[40][1], g[2][1]]
    for name, m in malformed_cases():
        members = filler[:2] + [m] + filler[2:]
        with pytest.raises((ValueError, zlib.error)):
            bam.bgzf_inflate(b"".join(members))
        with pytest.raises(lib.SnifflesAmdError, match=r"BGZF member 2: ") as e:
            inflate(zdev, members)
        if name in ("longer_than_isize", "shorter_than_isize"):
            assert "BGZF block size mismatch" in str(e.value)
        assert inflate(zdev, filler) == g[1][2] + g[40][2] + g[2][2], name      # the same handle inflates a good file afterwards
    with pytest.raises(ValueError):      # (zlib.error is not a ValueError: the host path's own refusals are)
        bam.bgzf_inflate(b"".join(filler + [malformed_cases()[4][1]]))


@pytest.mark.parametrize("grid", ["1", "2", "3", "unset"])
def test_the_first_bad_member_in_file_order_is_named(zdev, grid, monkeypatch):
    """Two bad members; under a capped grid the wave that holds the later one may meet it first."""
    if grid != "unset":
        monkeypatch.setenv("SNF_BGZF_GRID", grid)
    g = good_cases()
    bad = dict(malformed_cases())
    members = [g[1][1], g[2][1], g[3][1], bad["distance_before_start"], g[1][1], bad["block_type_3"], g[2][1]]
    with pytest.raises(lib.SnifflesAmdError, match=r"BGZF member 3: invalid distance too far back"):
        inflate(zdev, members)


def test_bgzf_members_raises_what_bgzf_inflate_raises():
    m = good_cases()[1][1]
    for data in (b"\x1f\x8b\x08\x00" + m[4:], m[:12] + b"XY" + m[14:]):
        with pytest.raises(ValueError) as a:
            bam.bgzf_inflate(data)
        with pytest.raises(ValueError) as b:
            bam.bgzf_members(data)
        assert str(a.value) == str(b.value)
    assert bam.bgzf_members(b"").shape == (0,)


# -------------------------------------------------------------------------------------------------------- record chain
def host_tables(raw):
    h = bam.parse_bam(raw)
    return h, bam.record_flags(h), bam.qname_ranks(h)


def same_as_host(d, raw):
    h, flags, ranks = host_tables(raw)
    assert d.n == h.n and (d.ref_names, d.ref_lens) == (h.ref_names, h.ref_lens)
    assert np.array_equal(d.rec_off, h.rec_off) and np.array_equal(d.ref_id, h.ref_id) and np.array_equal(d.pos, h.pos)
    assert np.array_equal(bam.record_flags(d), flags)
    dr = bam.qname_ranks(d)
    assert np.array_equal(dr[0], ranks[0]) and dr[1] == ranks[1]
    assert all(d.qname(i) == h.qname(i) for i in range(0, h.n, max(1, h.n // 7)))
    assert d.handle.read_stream(0, len(raw)) == raw
    return h


def through_device(raw, borders):
    data = B.reblock(raw, borders)
    assert bam.bgzf_inflate(data) == raw
    d = bam.bam_device(data)
    try:
        return same_as_host(d, raw)
    finally:
        d.handle.close()


@functools.lru_cache(None)
def stream30():
    return B.chain_stream(30)


def test_block_size_field_split_by_a_member_border(tier):
    raw, hlen, starts = stream30()
    k = 11
    for delta in range(-4, 5):      # -3 / -2 / -1: the field is split 3/1, 2/2, 1/3
        through_device(raw, [starts[4], starts[k] - delta, starts[20] + 2])


def test_records_across_members_and_members_of_many_records(tier):
    raw, hlen, starts = stream30()
    longest = max(range(30), key=lambda i: starts[i + 1] - starts[i])
    a, b = starts[longest], starts[longest + 1]
    assert b - a > 400
    through_device(raw, [a + 50, a + 50 + (b - a - 100) // 2, b - 50])                    # one record over three members (and a fourth)
    through_device(raw, list(range(hlen + 7, len(raw), 97)))                              # most records over several small members
    extra = [B.short_record(i) for i in range(200)]
    raw2, hlen2, st2 = B.chain_stream(3, extra=extra)
    assert st2[4] - st2[3] < 48
    borders, at = [], 3
    for cnt in (1, 2, 3, 7, 64, 123):                                                     # members of 1 ... 123 short records,
        at += cnt
        borders.append(st2[at])
    h = through_device(raw2, borders)                                                     # the last one of the remaining 0
    assert h.n == 203
    through_device(raw2, [st2[3]])                                                        # ... and one member of 200


def test_header_borders_empty_member_and_no_records(tier):
    raw, hlen, starts = stream30()
    through_device(raw, [hlen])                                   # the header ends exactly on a member border
    through_device(raw, [hlen - 1, hlen + 1])
    through_device(raw, [10, 20, 30, starts[5]])                  # the header over several members
    through_device(raw, [starts[9], starts[9], starts[15] + 1, starts[15] + 1, starts[15] + 1])      # empty members in the middle
    raw0 = bam.bam_stream(*B.REFS, [])
    h = through_device(raw0, [])
    assert h.n == 0
    through_device(raw0, [len(raw0)])


def test_truncated_streams_are_refused_in_parse_bam_s_words(tier):
    raw, hlen, starts = stream30()
    for cut, borders in ((raw[:-1], [starts[7]]), (raw[:starts[29] + 20], [starts[29] + 1])):
        with pytest.raises(ValueError) as a:
            bam.parse_bam(cut)
        with pytest.raises(ValueError) as b:
            bam.bam_device(B.reblock(cut, borders))
        assert str(a.value) == str(b.value) and "truncated BAM record at byte" in str(b.value)
    with pytest.raises((ValueError, struct.error)):      # one byte behind the last record: the host fails in struct.unpack_from
        bam.parse_bam(raw + b"\0")
    with pytest.raises(ValueError, match=f"truncated BAM record at byte {len(raw)}"):
        bam.bam_device(B.reblock(raw + b"\0", [starts[7]]))
    small = bytearray(raw)
    small[starts[13]:starts[13] + 4] = struct.pack("<i", 31)
    for borders in ([starts[7]], [starts[13] + 2]):
        with pytest.raises(ValueError) as a:
            bam.parse_bam(bytes(small))
        with pytest.raises(ValueError) as b:
            bam.bam_device(B.reblock(bytes(small), borders))
        assert str(a.value) == str(b.value) == f"truncated BAM record at byte {starts[13]}"
    d = bam.bam_device(B.reblock(raw, [starts[7]]))      # (and a good file afterwards)
    same_as_host(d, raw)
    d.handle.close()


def test_a_file_in_two_runs_through_the_carry(zdev):
    """The same file cut at every member border: the second run starts from the carry of the first."""
    raw, hlen, starts = stream30()
    borders = [hlen - 3, starts[2] + 1, starts[2] + 2, starts[9] - 2, starts[9] - 2, starts[17], starts[25] + 30]
    data = B.reblock(raw, borders)
    mem = bam.bgzf_members(data)
    h = bam.parse_bam(raw)
    for cut in range(len(mem) + 1):
        offs, got, carry, heads = [], b"", None, []
        for part in (mem[:cut], mem[cut:]):
            part = part.copy()
            if part.shape[0]:
                part["out_off"] -= part["out_off"][0]
            r = zdev.inflate(data, part, carry=carry, header_len=hlen)
            carry = r["carry"]
            offs += r["rec_off"][:-1].tolist()
            heads += r["heads"].tolist()
            got += zdev.read_stream(0, r["stream_len"])
        assert got == raw and offs == h.rec_off[:-1].tolist(), cut
        assert carry.count == h.n and carry.skip == 0 and carry.n_part == 0 and carry.stream_pos == len(raw)
        for i, hd in enumerate(heads):      # a head that the end of the first run cuts stays zero, every other one is the record's
            o = hlen + int(h.rec_off[i])
            assert hd == [0] * 6 or hd == list(struct.unpack_from("<6I", raw, o)), (cut, i)
        assert sum(hd == [0] * 6 for hd in heads) <= 1


# ---------------------------------------------------------------------------------------------------------- end to end
FIELDS = ("contig", "contig_len", "qc_nm_threshold", "qnames", "ps_names", "contig_names")


def task_inputs_equal(a, b):
    for k in a.leads:
        assert np.array_equal(a.leads[k], b.leads[k], equal_nan=a.leads[k].dtype.kind == "f"), k
    for k in ("seq_pool", "read_start", "read_end", "read_hp"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    for k in FIELDS:
        assert getattr(a, k) == getattr(b, k), k


EXTRACT_CASES = sorted(n for n, c in cases.EXTRACT.items() if "fixture" in c) + ["extract_fuzz_a", "extract_other_contig"]


@pytest.mark.parametrize("name", EXTRACT_CASES)
def test_extraction_over_a_device_view_equals_the_host_path(name, tier):
    case = cases.EXTRACT[name]
    recs = cases.extract_records(case)
    offs = recs.rec_off.tolist()
    raw = bam.bam_stream(recs.ref_names, recs.ref_lens, [recs.blob[a:b].tobytes() for a, b in zip(offs[:-1], offs[1:])])
    d = bam.bam_device(bam.bgzf_deflate(raw))
    try:
        same_as_host(d, raw)
        start, end = case["region"]
        cfg = type("Cfg", (), dict(case["cfg"]))()
        want, wi = extract.extract_region(bam.contig_records(recs, case["contig"]), case["contig"], start, end, cfg,
                                          read_id_offset=case["read_id_offset"])
        view = bam.contig_records(d, case["contig"])
        assert isinstance(view, bam.DeviceBamRecords) and view.handle is d.handle
        got, gi = extract.extract_region(view, case["contig"], start, end, cfg, read_id_offset=case["read_id_offset"])
        task_inputs_equal(want, got)
        assert (gi.read_id, gi.read_count) == (wi.read_id, wi.read_count)
        ti, _, x = extract.extract_region_device(view, case["contig"], start, end, cfg, read_id_offset=case["read_id_offset"])
        assert (ti.n_leads, ti.n_reads) == (want.n_leads, want.n_reads)
        x.close()
    finally:
        d.handle.close()


@functools.lru_cache(None)
def small_sample():
    names, lens, recs = synth_bam.gen_sample(21, ref_names=("chr20", "chrM_short", "chr21"), ref_lens=(150_000, 16_000, 120_000), cov=10.0,
                                             read_len_mean=6000, site_spacing=9000)[:3]
    return bam.bgzf_deflate(bam.bam_stream(names, lens, recs))


def sample_config():
    import vcf_util as vu
    cfg = SnifflesConfig(all_contigs=True)
    for k, v in vu.FIXED.items():      # (command line and start date of the VCF header)
        setattr(cfg, k, v)
    return cfg


def test_call_sample_writes_the_same_vcf_and_snf(tier, tmp_path):
    path = tmp_path / "sample.bam"
    path.write_bytes(small_sample())
    out = {}
    for kind, read in (("host", bam.read_bam), ("device", bam.read_bam_device)):
        recs = read(str(path))
        buf = io.StringIO()
        snf_path = tmp_path / "sample.snf"      # (the path is part of the SNF header)
        res = pipeline.call_sample(recs, sample_config(), vcf_handle=buf, snf_path=str(snf_path))
        # (the gzip members of an SNF carry their time of writing: the header line and the decoded blocks are compared)
        f = snf.SNFile.open(str(snf_path), sample_config())
        blocks = json.dumps({c: su.file_record(f, c, sv.TYPES) for c, _ in res.contig_lengths}, sort_keys=True)
        f.close()
        out[kind] = (buf.getvalue(), snf_path.read_bytes().split(b"\n", 1)[0] + blocks.encode(), res.read_count)
        buf = io.StringIO()
        pipeline.call_sample(recs, sample_config(), vcf_handle=buf)
        out[kind] += (buf.getvalue(),)
        if kind == "device":
            recs.handle.close()
    assert out["host"][2] > 100 and out["host"][3].count("\n") > out["host"][3].count("\n#") + 3      # (there are calls)
    assert out["host"] == out["device"]


def test_an_unsorted_file_is_refused(tier):
    names, lens = ["c1", "c2"], [100000, 50000]
    recs = [B.short_record(1, 0), B.short_record(2, 1), B.short_record(3, 0)]
    d = bam.bam_device(bam.bgzf_deflate(bam.bam_stream(names, lens, recs)))
    try:
        with pytest.raises(ValueError, match="not coordinate-sorted.*read_bam serves"):
            bam.contig_records(d, "c1")
        assert bam.contig_records(d, "c2").n == 1
    finally:
        d.handle.close()


def test_attach_refuses_what_upload_refuses(tier):
    """The record-table checks of snf_extract_upload (tests/test_extract.py::test_record_table_is_validated), from the heads."""
    qlen = 2000
    rec = synth_bam.make_record(0, 1000, 60, 0, "r1", [(0, qlen)], np.full(qlen, 1, np.uint8), b"")
    names, lens = ["c1", "c2"], [100000, 50000]
    host = bam.records_from_list(names, lens, [rec, rec])
    d = bam.bam_device(bam.bgzf_deflate(bam.bam_stream(names, lens, [rec, rec])))
    try:
        def both(match, host_recs, dev_view):
            msgs = []
            for r in (host_recs, dev_view):
                with pytest.raises(lib.SnifflesAmdError, match=match) as e:
                    extract.extract_region(r, "c1", 0, 100000)
                msgs.append(str(e.value))
            assert msgs[0] == msgs[1]
        view = bam.contig_records(d, "c1")
        h = bam.records_from_list(names, lens, [rec, rec]); h.blob[len(rec):len(rec) + 4] = np.frombuffer(struct.pack("<i", len(rec)), np.uint8)
        view.heads = view.heads.copy(); view.heads[1, 0] = len(rec)
        both("block_size of record 1 disagrees", h, view)
        view = bam.contig_records(d, "c1")
        h = bam.records_from_list(names, lens, [rec, rec]); h.blob[20:24] = np.frombuffer(struct.pack("<i", 10 ** 6), np.uint8)
        view.heads = view.heads.copy(); view.heads[0, 5] = 10 ** 6
        both("record 0 shorter than its fixed fields say", h, view)
        view = bam.contig_records(d, "c1")
        view.device = 1
        with pytest.raises(lib.SnifflesAmdError, match="on device 1, the handle on device 0"):
            extract.extract_region(view, "c1", 0, 100000)
        ti, _ = extract.extract_region(bam.contig_records(d, "c1"), "c1", 0, 100000)      # ... and the untouched view extracts
        assert ti.n_reads == 2
        assert host.n == 2
    finally:
        d.handle.close()
