"""BGZF deflate on the device (csrc/snf_deflate.h, sniffles_amd/bgzfout.py): every member against zlib's decoder, the file against
gzip, bam.bgzf_members and the device's own inflate; the `.vcf.gz` writer and its tabix index against a restatement of the tabix
specification written here; SNF blocks through the device.  Every case runs on the host tier (the unchanged kernels on the fibre
stand-in) and, marked gpu, through the real library.  Builders: tests/deflate_cases.py."""
import functools
import gzip
import io
import json
import struct
import zlib

import numpy as np
import pytest

import cases
import deflate_cases as D
import golden_util as gu
import snf_util as su
import vcf_util as vu
from sniffles_amd import bam, bgzfout, lib, pipeline, snf, sv
from sniffles_amd.config import SnifflesConfig

FF00 = D.FF00


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def tier(request, monkeypatch):
    for k in ("SNF_DEFLATE_GRID", "SNF_DEFLATE_MAXBITS", "SNF_BGZF_GRID", "SNF_BGZF_THREAD"):
        monkeypatch.delenv(k, raising=False)
    if request.param == "emu":
        import emu.emu as E
        E.lib()
    return request.param


@pytest.fixture
def zdev(tier):
    z = bgzfout.DeflateDevice(0)
    yield z
    z.close()


@functools.lru_cache(None)
def kernel_cases():
    return D.all_cases()


def case(name):
    return dict(kernel_cases())[name]


def device_inflate(image):
    z = bam.BgzfDevice(0)
    try:
        mem = bam.bgzf_members(image)
        total = int(mem["isize"].sum())
        r = z.inflate(image, mem, header_len=total)
        assert r["stream_len"] == total
        return z.read_stream(0, total)
    finally:
        z.close()


def check_run(image, off, inputs, inflate=True):
    """The exact checks for every member produced: `inputs` are the members' input bytes."""
    assert len(off) == len(inputs) + 1 and off[0] == 0 and off[-1] == len(image)
    mem = D.members_of(image)
    assert len(mem) == len(inputs)
    for i, ((p, size, payload, crc, isize), raw) in enumerate(zip(mem, inputs)):
        assert (p, p + size) == (off[i], off[i + 1]), i                      # BSIZE agrees with member_off
        assert zlib.decompress(payload, -15) == raw, i
        assert crc == zlib.crc32(raw) and isize == len(raw), i
        assert size <= len(raw) + 31, (i, size, len(raw))                    # never longer than the stored form
    whole = b"".join(inputs)
    assert (gzip.decompress(image) if image else b"") == whole               # CRC-32 and ISIZE once more, by gzip
    data = image + D.EOF
    walk = bam.bgzf_members(data)
    assert walk.shape[0] == len(inputs) + 1 and walk["isize"].tolist() == [len(r) for r in inputs] + [0]
    assert (walk["payload_off"] - 18).tolist() == list(off[:-1]) + [len(image)] and data[-28:] == D.EOF
    assert bam.bgzf_inflate(data) == whole
    if inflate:
        assert device_inflate(data) == whole


# ------------------------------------------------------------------------------------------------------------- the kernel
def test_every_case_one_member_at_a_time(zdev):
    names = [n for n, _ in kernel_cases()]
    for want in ("len0", "len1", "len2", "len3", "len4", "len5", "len63", "len64", "len65", "len65279", "len65280", "len255", "len256", "len257",
                 "len1023", "len1024", "len1025", "equal258", "equal259", "equal260", "equal261", "equal262", "equal65280", "period2", "period3",
                 "period4", "period5", "period63", "period64", "period65", "period257", "period258", "period259", "period300",
                 "period_ends_on_last_byte", "period_cut_by_the_end", "distance32768", "distance32769", "fibonacci",
                 "literals_200_distinct", "literals_de_bruijn", "single_byte", "random_full", "random_full_minus_1", "acgt_full", "long_tokens"):
        assert want in names, want
    assert sum(len(d) >= FF00 - 1 for _, d in kernel_cases()) <= 12      # (the full-size members: the fibre stand-in stays usable)
    wrong = []
    for name, raw in kernel_cases():
        image, off = zdev.compress(raw, [len(raw)])
        try:
            check_run(image, off.tolist(), [raw], inflate=False)
        except (AssertionError, zlib.error, OSError, ValueError) as e:
            wrong.append((name, repr(e)[:200]))
    assert not wrong, wrong


def test_all_cases_as_one_file_through_the_device_inflate(zdev):
    inputs = [d for _, d in kernel_cases()]
    image, off = zdev.compress(b"".join(inputs), [len(d) for d in inputs])
    check_run(image, off.tolist(), inputs)


def block_head(payload):
    """(BTYPE, HLIT, HDIST) of a member's first block."""
    bits = int.from_bytes(payload[:4], "little")
    return (bits >> 1) & 3, ((bits >> 3) & 31) + 257, ((bits >> 8) & 31) + 1


def test_corner_forms_and_the_stored_fallback(zdev):
    def payload(name):
        image, _ = zdev.compress(case(name), [len(case(name))])
        return D.members_of(image)[0][2]
    bt, hlit, hdist = block_head(payload("literals_de_bruijn"))
    assert bt == 2 and hdist == 1 and hlit == 257                 # a dynamic block without a distance code
    p = payload("equal65280")
    assert block_head(p)[0] == 2 and block_head(p)[2] == 1        # exactly one distance code: distance 1
    for name in ("random_full", "random_full_minus_1", "single_byte", "len2"):
        p = payload(name)
        n = len(case(name))
        assert p[0] == 1 and len(p) == n + 5 and p[1:5] == struct.pack("<HH", n, n ^ 0xffff) and p[5:] == case(name), name
    assert payload("len0") == b"\x03\x00"                         # the empty member is the EOF marker
    image, _ = zdev.compress(b"", [0])
    assert image == D.EOF == bgzfout.EOF_MEMBER
    assert zdev.compress(b"")[0] == b"" and zdev.compress(b"")[1].tolist() == [0]


@functools.lru_cache(None)
def fixture_text():
    with gzip.open(gu.GOLDEN_DIR + "/vcf_text.json.gz") as f:
        t = json.load(f)["combine"]["combine_task_8samples_dense"]["text"]["fasta"].encode()
    assert len(t) == 232462
    return t


def test_size_caps(zdev):
    """Caps that keep a broken coder from passing as valid but useless; zlib at levels 1 and 6 stays inside each."""
    def size(data):
        image, off = zdev.compress(data)
        check_run(image, off.tolist(), [data[i:i + FF00] for i in range(0, len(data), FF00)], inflate=False)
        return len(image)
    sizes = dict(equal=size(case("equal65280")), period300=size(case("period300_full")), acgt=size(case("acgt_full")), vcf=size(fixture_text()))
    print("deflate sizes", sizes)
    assert sizes["equal"] <= 2048              # distance 1 and length-258 matches
    assert sizes["period300"] <= 4096          # matches beyond a wave's width
    assert sizes["acgt"] <= 0.40 * FF00        # dynamic codes (fixed: 0.426, stored: 1.0)
    assert sizes["vcf"] <= 0.40 * 232462       # matching (Huffman only: 0.532)


LIMIT_INPUTS = ("skewed_literals", "fibonacci", "long_tokens", "acgt_full")


def deepest_codes(z):
    out = {}
    for name in LIMIT_INPUTS:
        raw = case(name)
        image, off = z.compress(raw, [len(raw)])
        check_run(image, off.tolist(), [raw], inflate=False)
        ll, dl = D.header_code_lengths(D.members_of(image)[0][2])
        out[name] = max(ll + dl)
    return out


def test_code_lengths_stay_inside_the_limit(zdev, monkeypatch):
    """The histograms of inputs of this size are at most 13 bits deep in this coder (a plain Huffman code of `skewed_literals` is 13 deep;
    bytes skewed enough for 16 repeat, and repeats become matches), so deflate's 15 bits never bind: SNF_DEFLATE_MAXBITS lowers the limit until
    the limiter is entered.  At every limit the members decode and no code is longer than the limit."""
    natural = deepest_codes(zdev)
    print("deepest codes", natural)
    assert 12 <= natural["skewed_literals"] <= 15 and max(natural.values()) <= 15
    for limit in (12, 11, 10, 9):
        monkeypatch.setenv("SNF_DEFLATE_MAXBITS", str(limit))
        got = deepest_codes(zdev)
        print("limit", limit, got)
        assert max(got.values()) <= limit, (limit, got)
        assert all(got[n] == natural[n] for n in got if natural[n] <= limit), (limit, got)      # a code that fits is left as it is
    monkeypatch.setenv("SNF_DEFLATE_MAXBITS", "16")      # out of range: deflate's limit
    assert deepest_codes(zdev) == natural


def test_mixed_member_lengths_in_one_run(zdev):
    a, b = case("acgt_full"), case("period300_full")
    inputs = [b"", b"x", a, b"hello", b, b""]
    image, off = zdev.compress(b"".join(inputs), [len(d) for d in inputs])
    assert [len(d) for d in inputs] == [0, 1, FF00, 5, FF00, 0]
    check_run(image, off.tolist(), inputs)


@functools.lru_cache(None)
def grid_file():
    """Twelve members: long ones before short ones with the same period (what a strided workgroup's LDS still holds behind a short
    member's end continues its last match), members with and without distance codes, stored ones, empty ones."""
    pick = ["period300_full", "period_cut_by_the_end", "acgt_full", "literals_de_bruijn", "equal65280", "len5", "random_full", "len0",
            "distance32769", "period_ends_on_last_byte", "fibonacci", "equal259"]
    return [case(n) for n in pick]


@pytest.mark.parametrize("grid", ["1", "2", "7", "n-1", "n", "unset"])
def test_grids_give_identical_bytes(zdev, grid, monkeypatch):
    inputs = grid_file()
    n = len(inputs)
    data, ml = b"".join(inputs), [len(d) for d in inputs]
    want = b"".join(zdev.compress(d, [len(d)])[0] for d in inputs)      # every member alone, default grid
    if grid != "unset":
        monkeypatch.setenv("SNF_DEFLATE_GRID", str({"n-1": n - 1, "n": n}.get(grid, grid)))
    image, off = zdev.compress(data, ml)
    assert image == want
    check_run(image, off.tolist(), inputs, inflate=(grid == "2"))


def test_a_handle_is_reused_and_runs_are_deterministic(tier, monkeypatch):
    inputs = grid_file()
    data, ml = b"".join(inputs), [len(d) for d in inputs]
    other = [case("len1025"), case("long_tokens"), case("len64")]
    z = bgzfout.DeflateDevice(0)
    first = z.compress(data, ml)[0]
    assert z.compress(data, ml)[0] == first                              # two runs on one handle
    second = z.compress(b"".join(other), [len(d) for d in other])[0]     # a second, different (smaller) input on the same handle
    z.close()
    with bgzfout.DeflateDevice(0) as fresh:
        assert fresh.compress(b"".join(other), [len(d) for d in other])[0] == second
        if tier == "emu":      # the lanes and the workgroups in a shuffled order: the same bytes
            monkeypatch.setenv("SNF_SIMT_ORDER", "random:7")
            monkeypatch.setenv("SNF_DEFLATE_GRID", "5")
        assert fresh.compress(data, ml)[0] == first


def test_refusals_of_the_entry_point(zdev):
    with pytest.raises(lib.SnifflesAmdError, match=r"member 1 has 65281 bytes.*65280"):
        zdev.compress(b"a" * (5 + FF00 + 1), [5, FF00 + 1])
    with pytest.raises(lib.SnifflesAmdError, match=r"add up to 7, the data has 8 bytes"):
        zdev.compress(b"a" * 8, [3, 4])
    image, off = zdev.compress(b"abcabcabc", [9])      # the handle goes on
    check_run(image, off.tolist(), [b"abcabcabc"], inflate=False)


# ----------------------------------------------------------------------------------------------- tabix, restated from the specification
def spec_reg2bin(beg, end):
    end -= 1
    if beg >> 14 == end >> 14: return ((1 << 15) - 1) // 7 + (beg >> 14)
    if beg >> 17 == end >> 17: return ((1 << 12) - 1) // 7 + (beg >> 17)
    if beg >> 20 == end >> 20: return ((1 << 9) - 1) // 7 + (beg >> 20)
    if beg >> 23 == end >> 23: return ((1 << 6) - 1) // 7 + (beg >> 23)
    if beg >> 26 == end >> 26: return ((1 << 3) - 1) // 7 + (beg >> 26)
    return 0


def spec_reg2bins(beg, end):
    end -= 1
    out = [0]
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out += list(range(first + (beg >> shift), first + (end >> shift) + 1))
    return out


def parse_tbi(raw):
    """The fields of a tabix index as the specification lists them."""
    assert raw[:4] == b"TBI\x01"
    n_ref, fmt, col_seq, col_beg, col_end, meta, skip, l_nm = struct.unpack_from("<8i", raw, 4)
    p = 36
    names = raw[p:p + l_nm].split(b"\0")
    assert names.pop() == b"" and len(names) == n_ref
    p += l_nm
    refs = []
    for _ in range(n_ref):
        n_bin = struct.unpack_from("<i", raw, p)[0]; p += 4
        bins = {}
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", raw, p); p += 8
            bins[b] = [struct.unpack_from("<QQ", raw, p + 16 * k) for k in range(n_chunk)]; p += 16 * n_chunk
        n_intv = struct.unpack_from("<i", raw, p)[0]; p += 4
        lin = list(struct.unpack_from(f"<{n_intv}Q", raw, p)); p += 8 * n_intv
        refs.append((bins, lin))
    n_no_coor = struct.unpack_from("<Q", raw, p)[0] if p < len(raw) else None
    assert p + 8 == len(raw)
    return dict(header=(fmt, col_seq, col_beg, col_end, meta, skip), names=names, refs=refs, n_no_coor=n_no_coor)


def spec_interval(line):
    f = line.split(b"\t")
    beg = int(f[1]) - 1
    end = beg + len(f[3])
    for item in f[7].split(b";"):
        if item.startswith(b"END=") and int(item[4:]) > beg:
            end = int(item[4:])
    return f[0], beg, end


def records_of(text, data):
    """[(contig, beg, end, virtual offset of the line's first byte, line)] from the text and the member walk of the file."""
    mem = bam.bgzf_members(data)
    starts, foff = mem["out_off"].tolist(), (mem["payload_off"] - 18).tolist()
    out, u = [], 0
    for ln in text.split(b"\n")[:-1]:
        if not ln.startswith(b"#"):
            m = max(k for k in range(len(starts)) if starts[k] <= u and (mem["isize"][k] or starts[k] == u))
            out.append(spec_interval(ln) + (foff[m] << 16 | (u - starts[m]), ln))
        u += len(ln) + 1
    return out


def read_chunk(data, vbeg, vend):
    """The bytes of a chunk, by seeking to its virtual offsets with zlib."""
    out, co = b"", vbeg >> 16
    while co <= vend >> 16 and co < len(data):
        z = zlib.decompressobj(31)
        raw = z.decompress(data[co:])
        size = len(data) - co - len(z.unused_data)
        lo = vbeg & 0xffff if co == vbeg >> 16 else 0
        hi = vend & 0xffff if co == vend >> 16 else len(raw)
        out += raw[lo:hi]
        co += size
    return out


HAND_VCF = (b"##fileformat=VCFv4.2\n##contig=<ID=chrA,length=3000000>\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS\n"
            b"chrA\t100\tdel1\tN\t<DEL>\t60\tPASS\tPRECISE;SVTYPE=DEL;SVLEN=-40000;END=40100;SUPPORT=9\tGT\t0/1\n"          # symbolic ALT, END= over three windows
            b"chrA\t16384\tins1\tN\tNACGTACGT\t60\tPASS\tEND=16384;SVTYPE=INS\tGT\t1/1\n"                                  # END= at the start of INFO, not above beg + 1
            b"chrA\t16390\tdel2\tACGTACGTAC\tA\t60\tPASS\tSVTYPE=DEL;SVLEN=-9\tGT\t0/1\n"                                   # no END=: beg + len(REF)
            b"chrA\t20000\tbnd1\tN\tN]chrB:5000]\t60\tPASS\tSVTYPE=BND;CHR2=chrB;SUPPORT=4\tGT\t0/1\n"                      # BND
            b"chrA\t2000000\tdel3\tN\t<DEL>\t60\tPASS\tSVTYPE=DEL;XEND=5;END=2200000\tGT\t0/1\n"                            # END= behind a ';' (XEND= is not it)
            b"chrB\t5000\tbnd2\tN\t[chrA:20000[N\t60\tPASS\tSVTYPE=BND;CHR2=chrA\tGT\t0/1\n"
            b"chrB\t5000\tinv1\tN\t<INV>\t60\tPASS\tSVTYPE=INV;END=140000\tGT\t0/1\n")


def written(tmp_path, text, run_bytes=64 << 20, pieces=977):
    path = str(tmp_path / "out.vcf.gz")
    w = bgzfout.VcfGzWriter(path, run_bytes=run_bytes)
    for i in range(0, len(text), pieces):      # (the writer sees fragments, not lines)
        w.write(text[i:i + pieces] if i % 2 else text[i:i + pieces].decode())
    w.close()
    w.close()
    with open(path, "rb") as f:
        data = f.read()
    with open(path + ".tbi", "rb") as f:
        tbi = f.read()
    assert gzip.decompress(data) == text and data[-28:] == D.EOF and tbi[-28:] == D.EOF
    bam.bgzf_members(tbi)      # the index file is BGZF itself
    return data, parse_tbi(gzip.decompress(tbi))


def check_structure(text, data, idx):
    recs = records_of(text, data)
    assert idx["header"] == (2, 1, 2, 0, ord("#"), 0) and idx["n_no_coor"] == 0
    names = []
    for r in recs:
        if r[0] not in names:
            names.append(r[0])
    assert idx["names"] == names
    for tid, (bins, lin) in enumerate(idx["refs"]):
        mine = [r for r in recs if r[0] == names[tid]]
        meta = bins.pop(37450)
        assert meta[1] == (len(mine), 0) and meta[0][0] == mine[0][3]
        runs = []      # a chunk: a run of consecutive records with the same bin
        for r in mine:
            b = spec_reg2bin(r[1], r[2])
            if runs and runs[-1][0] == b:
                runs[-1][2] = r
            else:
                runs.append([b, r, r])
        want = {}
        for b, first, last in runs:
            want.setdefault(b, []).append(first[3])
        assert {b: [c[0] for c in ch] for b, ch in bins.items()} == want
        for b, ch in bins.items():
            assert all(c[1] > c[0] for c in ch)
        bins[37450] = meta
    return recs, names


def test_tbi_structure_of_bnd_end_and_symbolic_records(tier, tmp_path):
    data, idx = written(tmp_path, HAND_VCF)
    recs, names = check_structure(HAND_VCF, data, idx)
    assert [(r[1], r[2]) for r in recs] == [(99, 40100), (16383, 16384), (16389, 16399), (19999, 20000), (1999999, 2200000), (4999, 5000), (4999, 140000)]
    assert names == [b"chrA", b"chrB"]
    bins, lin = idx["refs"][0]
    assert sorted(b for b in bins if b != 37450) == sorted({spec_reg2bin(r[1], r[2]) for r in recs if r[0] == b"chrA"})
    first = recs[0][3]
    assert lin[:3] == [first, first, first] and len(lin) == (2200000 - 1 >> 14) + 1      # END= reaches the linear index: the deletion's three windows
    assert lin[3] == lin[(1999999 >> 14)] == recs[4][3]                                  # holes take the next window's offset


@functools.lru_cache(None)
def big_text():
    """The dense combine fixture (232 kB, 4 members, END= on every record), shifted by a header line so that one record ends exactly
    on a member border."""
    t = fixture_text()
    ends = [i + 1 for i in range(len(t)) if t[i] == 10]
    e = next(x for x in ends if x > FF00 and not t[t.rfind(b"\n", 0, x - 1) + 1:x].startswith(b"#"))
    pad = (-e) % FF00
    pad += FF00 if pad < 8 else 0
    line = b"##pad=" + b"x" * (pad - 7) + b"\n"
    assert len(line) == pad
    out = line + t
    assert (e + pad) % FF00 == 0
    return out


def test_every_overlapping_record_starts_inside_a_returned_chunk(tier, tmp_path):
    text = big_text()
    data, idx = written(tmp_path, text, run_bytes=2 * FF00)      # (two runs of two members)
    assert bam.bgzf_members(data).shape[0] >= 4
    recs, names = check_structure(text, data, idx)
    mem = bam.bgzf_members(data)
    borders = set(mem["out_off"].tolist())
    u, on_border, straddles = 0, 0, 0
    for ln in text.split(b"\n")[:-1]:
        a, b = u, u + len(ln) + 1
        u = b
        if not ln.startswith(b"#"):
            on_border += b in borders
            straddles += any(a < x < b for x in borders)
    assert on_border >= 1 and straddles >= 2
    for tid, name in enumerate(names):
        mine = [r for r in recs if r[0] == name]
        bins, lin = idx["refs"][tid]
        top = max(r[2] for r in mine)
        queries = {(max(0, w + d), max(0, w + d) + 1) for w in range(0, top + (1 << 14), 1 << 14) for d in (-1, 0, 1)}
        queries |= {(0, top + 5), (mine[len(mine) // 2][1], mine[len(mine) // 2][1] + 40000)}
        for qb, qe in sorted(queries):
            lo = lin[qb >> 14] if qb >> 14 < len(lin) else lin[-1]
            chunks = [c for b in spec_reg2bins(qb, qe) if b in bins and b != 37450 for c in bins[b] if c[1] > lo]
            hits = [r for r in mine if r[1] < qe and r[2] > qb]
            for r in hits:
                assert any(c[0] <= r[3] < c[1] for c in chunks), (name, qb, qe, r[:3])
        # read back: the chunks of the whole contig hold exactly its lines
        got = b"".join(read_chunk(data, c[0], c[1]) for c in sorted(c for b, ch in bins.items() if b != 37450 for c in ch))
        assert sorted(got.split(b"\n")[:-1]) == sorted(r[4] for r in mine)


def test_unsorted_input_and_a_returning_contig_are_refused(tier, tmp_path):
    head, rows = HAND_VCF.split(b"#CHROM")[0], HAND_VCF.split(b"\n")[3:-1]
    for bad, msg in ((rows[:3] + [rows[1]], r"VCF line 6: position 16384 of chrA is below"),
                     (rows[:2] + [rows[5]] + [rows[2]], r"VCF line 6: contig chrA returns after another one")):
        w = bgzfout.VcfGzWriter(str(tmp_path / "bad.vcf.gz"))
        with pytest.raises(ValueError, match=msg):
            w.write(head + b"\n".join(bad) + b"\n")
        w.close()


# ------------------------------------------------------------------------------------------------------------ the drivers
def config_for(args=(), **kw):
    from test_pipeline import config_for as cf
    cfg = cf(args)
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def through_writer(tmp_path, name, run):
    """`run(handle)` into a plain handle and into a VcfGzWriter: the same characters; the index describes the records."""
    plain = io.StringIO()
    run(plain)
    path = str(tmp_path / (name + ".vcf.gz"))
    with bgzfout.VcfGzWriter(path) as w:
        run(w)
    with gzip.open(path, "rt", newline="") as f:
        assert f.read() == plain.getvalue()
    text = plain.getvalue().encode()
    with open(path, "rb") as f:
        data = f.read()
    with open(path + ".tbi", "rb") as f:
        idx = parse_tbi(gzip.decompress(f.read()))
    recs, _ = check_structure(text, data, idx)
    assert len(recs) > 3
    return plain.getvalue()


@functools.lru_cache(None)
def small_population():
    """Two samples that share their SV sites, contigs of 150 kb (the builder of cases.POPULATIONS at a size a test can afford twice)."""
    return [cases._sample(30 + s, ref_names=("chr8", "chr9"), ref_lens=(150_000, 120_000), cov=12.0, site_seed=77, site_spacing=9000)
            for s in range(2)]


@functools.lru_cache(None)
def splits_sample():
    return cases.SAMPLES["sample_splits_14x"][0]()


def test_call_sample_writes_vcf_gz(tier, tmp_path):
    recs = splits_sample()
    tr = getattr(recs, "tandem_repeats", None)
    text = through_writer(tmp_path, "calls", lambda h: pipeline.call_sample(recs, config_for(()), vcf_handle=h, tandem_repeats=tr))
    assert "SVTYPE=BND" in text and "END=" in text


def test_genotype_vcf_writes_vcf_gz(tier, tmp_path):
    name = "sample_splits_14x"
    recs = splits_sample()
    # (the fixture's input has two breakend lines in front of their neighbours, and genotype_vcf keeps the input's order: the records sorted,
    # as the reference needs them for a .gz - it refuses --no-sort there)
    lines = gu.load("genotype_vcf")[name]["vcf_in"].split("\n")
    head = [ln for ln in lines if ln.startswith("#")]
    body = [ln for ln in lines if ln and not ln.startswith("#")]
    order = {c: k for k, c in enumerate(dict.fromkeys(ln.split("\t")[0] for ln in body))}
    body.sort(key=lambda ln: (order[ln.split("\t")[0]], int(ln.split("\t")[1])))
    vcf_in = "\n".join(head + body) + "\n"
    through_writer(tmp_path, "genotyped", lambda h: pipeline.genotype_vcf(recs, config_for(()), io.StringIO(vcf_in), h))


def test_snf_blocks_through_the_device_and_combine(tier, tmp_path):
    samples = small_population()
    paths = {"host": [], "device": []}
    with bgzfout.DeflateDevice(0) as z:
        for s, recs in enumerate(samples):
            for kind in paths:
                (tmp_path / kind).mkdir(exist_ok=True)
                path = str(tmp_path / kind / f"sample{s}.snf")      # (the file's name is the sample's name in the merged VCF)
                pipeline.call_sample(recs, config_for(("--all-contigs",)), snf_path=path, tandem_repeats=getattr(recs, "tandem_repeats", None),
                                     snf_deflater=z if kind == "device" else None)
                paths[kind].append(path)
    n_blocks = 0
    for h, d in zip(paths["host"], paths["device"]):
        fh, fd = snf.SNFile.open(h, SnifflesConfig()), snf.SNFile.open(d, SnifflesConfig())
        assert sorted(fh.index) == sorted(fd.index)
        for c in fh.index:
            assert json.dumps(su.file_record(fh, c, sv.TYPES), sort_keys=True) == json.dumps(su.file_record(fd, c, sv.TYPES), sort_keys=True)
        raw_h, raw_d = open(h, "rb").read().split(b"\n", 1)[1], open(d, "rb").read().split(b"\n", 1)[1]
        for c in fh.index:      # every indexed range is what gzip.decompress reads: the block's pickle, and a run of BGZF members
            assert sorted(fh.index[c]) == sorted(fd.index[c])
            for b in fh.index[c]:
                for (oh, lh), (od, ld) in zip(fh.index[c][b], fd.index[c][b]):
                    assert gzip.decompress(raw_d[od:od + ld]) == gzip.decompress(raw_h[oh:oh + lh])
                    assert int(bam.bgzf_members(raw_d[od:od + ld])["isize"].sum()) == len(gzip.decompress(raw_h[oh:oh + lh]))
                    n_blocks += 1
        fh.close(); fd.close()
    assert n_blocks >= 4
    host_text = io.StringIO()
    pipeline.combine(paths["host"], config_for(("--all-contigs",)), vcf_handle=host_text)
    device_text = through_writer(tmp_path, "merged", lambda h: pipeline.combine(paths["device"], config_for(("--all-contigs",)), vcf_handle=h))
    assert device_text == host_text.getvalue() and device_text.count("\n") > device_text.count("\n#") + 3


@pytest.mark.skipif(not __import__("make_ref").ref_root(), reason="needs the reference (its checkout, or the staged build oracle/_ref that make_ref.py compiles)")
def test_the_reference_reads_a_device_written_snf(tmp_path):
    import emu.emu as E
    import ref_harness as rh
    E.lib()
    recs = small_population()[0]
    path = str(tmp_path / "device.snf")
    with bgzfout.DeflateDevice(0) as z:
        pipeline.call_sample(recs, config_for(("--all-contigs",)), snf_path=path, tandem_repeats=getattr(recs, "tandem_repeats", None), snf_deflater=z)
    ours = snf.SNFile.open(path, SnifflesConfig())
    theirs = rh.open_reference_snf(path)
    n = 0
    for c in ours.index:
        a, b = su.file_record(ours, c, sv.TYPES), su.file_record(theirs, c, sv.TYPES)
        assert json.dumps(a, sort_keys=True) == json.dumps(b, sort_keys=True)
        n += len(a["blocks"])
    assert n >= 2
    ours.close(); theirs.close()
