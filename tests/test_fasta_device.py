"""The device-resident reference (sniffles_amd/csrc/snf_fasta.h, sniffles_amd/fasta.py DeviceFasta): the `.fai` table, the runs of
'N' and the batched fetches against `fasta.FastaFile` on the same bytes and `soa.paint_nmask` over it; the record-table writer with a
device reference against the unmodified reference's own text (tests/golden/vcf_text.json.gz) and against `write_call`; the drivers
against their object path.  The device path is never compared with itself.  Every case runs on the host tier (the unchanged kernels
on the fibre stand-in) and, marked gpu, through the real library.  Builders: tests/fasta_cases.py."""
import functools
import gzip
import io
import os
import re

import numpy as np
import pytest

import cases
import fasta_cases as F
import golden_util as gu
import vcf_util as vu
from sniffles_amd import abi, bam, fasta, leadprov, lib, parallel, pipeline, soa, sv, vcf

S = F.chunk_sizes()
VEC, WAVE, CHUNK, STEP = S["FA_VEC"], S["FA_WAVE_BYTES"], S["FA_CHUNK"], S["FA_GATHER_STEP"]


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def tier(request, monkeypatch):
    for k in ("SNF_FASTA_GRID", "SNF_BGZF_GRID", "SNF_BGZF_THREAD"):
        monkeypatch.delenv(k, raising=False)
    if request.param == "emu":
        import emu.emu as E
        E.lib()
    return request.param


def put(tmp_path, data: bytes, name="ref.fa"):
    p = tmp_path / name
    p.write_bytes(data)
    for stale in (str(p) + ".fai",):
        if os.path.exists(stale):
            os.unlink(stale)
    return str(p)


def outcome(fn, *a):
    """What a call returns, or the type and text of what it raises."""
    try:
        return fn(*a)
    except Exception as e:  # noqa: BLE001 - the exception is the result
        return (type(e).__name__, str(e))


def assert_same_index(path, text=None, **kw):
    host = fasta.FastaFile(path)
    with fasta.open_device(path, **kw) as dev:
        assert dev._index == host._index, (path, dev._index, host._index)
        assert list(dev._index) == list(host._index) and dev.references == host.references      # dict order
        for c in host.references:
            assert dev.get_reference_length(c) == host.get_reference_length(c)
        if text is not None:
            assert dev.text_len == len(text) and dev.read_text(0, len(text)) == text
        return dict(host._index), dict(dev.timing)


# ------------------------------------------------------------------------------------------------------ A. text and index
@functools.lru_cache(None)
def index_texts():
    rng = np.random.default_rng(17)
    R, B = F.record, F.bases
    out = {}
    for w in (1, 7, 60):
        out[f"width{w}"] = R(b"c1 first", B(rng, 301), w) + R(b"c2", B(rng, 60), w) + R(b"c3\tx", B(rng, 59), w)
    out["crlf"] = R(b"a x", B(rng, 130), 60, b"\r\n") + R(b"b", B(rng, 60), 60, b"\r\n") + R(b"c", B(rng, 7), 7, b"\r\n")
    out["crlf_no_final_newline"] = out["crlf"][:-2]
    out["cr_at_the_end"] = out["crlf"][:-1]                                  # the text ends in '\r'
    out["no_final_newline"] = out["width60"][:-1]
    out["gt_inside_header"] = R(b"a >b >c", B(rng, 100), 60) + R(b">", B(rng, 10), 60) + R(b"d", B(rng, 61), 60)
    out["empty_records"] = R(b"a", B(rng, 70), 60) + b">empty one\n" + R(b"b", B(rng, 5), 60) + b">empty_last\n"
    out["empty_last_no_newline"] = R(b"a", B(rng, 70), 60) + b">e"
    out["only_header"] = b">lonely"
    out["single_line_last_no_newline"] = R(b"a", B(rng, 70), 60) + b">z\nACGTN"
    out["nameless_and_duplicate"] = R(b"", B(rng, 9), 60) + R(b"dup", B(rng, 61), 60) + R(b" lead", B(rng, 3), 60) + R(b"dup", B(rng, 5), 60)
    out["blank_first_line"] = b">a\n\nACGT\n>b\nAC\n"
    out["short_records_1000"] = b"".join(R(b"s%d" % k, B(rng, 1 + k % 5), 60) for k in range(1000))      # more headers than a scan block
    for name, b in (("thread", VEC), ("wave", WAVE), ("workgroup", CHUNK), ("workgroup2", 2 * CHUNK)):
        for d in (-1, 0, 1):
            out[f"header_at_{name}{d:+d}"] = F.text_with_header_at(b + d, rng)
            out[f"crlf_header_at_{name}{d:+d}"] = F.text_with_header_at(b + d, rng, nl=b"\r\n")
        # a header line that straddles the border: its '>' five bytes in front of it
        out[f"header_across_{name}"] = F.text_with_header_at(b - 5, rng, head=b"straddles the border " + b"w" * 40)
    for d in (-1, 0, 1):
        out[f"length_workgroup{d:+d}"] = F.text_of_length(CHUNK + d, rng)
        out[f"length_workgroup3{d:+d}"] = F.text_of_length(3 * CHUNK + d, rng)
    out["not_fasta"] = b"hello\nworld, no header here\n"
    out["empty_file"] = b""
    return out


@pytest.mark.parametrize("grid", [None, "1", "2", "7"])
def test_index_equals_scan_bytes(tier, tmp_path, monkeypatch, grid):
    if grid:
        monkeypatch.setenv("SNF_FASTA_GRID", grid)
    seen = {}
    for name, text in index_texts().items():
        seen[name], _ = assert_same_index(put(tmp_path, text), text)
    assert seen["not_fasta"] == {} and seen["empty_file"] == {}
    assert seen["empty_records"]["empty"][0] == 0 and seen["empty_records"]["empty_last"] == (0, len(index_texts()["empty_records"]), 1, 1)
    assert len(seen["short_records_1000"]) == 1000
    assert seen["header_at_workgroup+0"]["second"][1] == CHUNK + len(b">second extra words\n")


def test_index_of_one_line_of_a_million_bases(tier, tmp_path):
    rng = np.random.default_rng(5)
    text = F.record(b"one", F.bases(rng, 1_000_000, b"ACGTN"), 1_000_000) + F.record(b"two", F.bases(rng, 99), 1_000_000)
    idx, _ = assert_same_index(put(tmp_path, text), text)
    assert idx["one"] == (1_000_000, 5, 1_000_000, 1_000_001)
    host = fasta.FastaFile(put(tmp_path, text))
    with fasta.open_device(put(tmp_path, text)) as dev:
        for a, b in ((0, 70), (999_990, 1_000_050), (123_456, 123_457)):
            assert dev.fetch("one", a, b) == host.fetch("one", a, b)
        assert dev.fetch("two") == host.fetch("two")


def test_fai_is_used_as_fastafile_uses_it(tier, tmp_path):
    text = index_texts()["width7"]
    path = put(tmp_path, text)
    want = dict(fasta.FastaFile(path)._index)
    with open(path + ".fai", "w") as f:
        f.write("short\t1\t2\n")                                             # fewer than five columns: ignored
        for k, v in want.items():
            f.write("\t".join([k] + [str(x) for x in v] + ["a sixth column"]) + "\n")
    host = fasta.FastaFile(path)
    with fasta.open_device(path) as dev:
        assert dev._index == host._index == want and dev.timing["index_ms"] == 0.0      # no fa_index ran
        for c in want:
            assert dev.fetch(c) == host.fetch(c) and dev.fetch(c, 3, 20) == host.fetch(c, 3, 20)
    with open(path + ".fai", "w") as f:                                      # an index of another file: refused with the reason
        f.write("c1\t100000\t10\t60\t61\n")
    with pytest.raises(lib.SnifflesAmdError, match=r"contig 0: its last base lies at byte \d+, the text has \d+ bytes"):
        fasta.open_device(path)
    os.unlink(path + ".fai")


def test_bgzf_and_gzip_load_the_same_text(tier, tmp_path):
    texts = index_texts()
    rng = np.random.default_rng(23)
    big = b"".join(F.record(b"big%d" % k, F.bases(rng, 70_000 + k, b"ACGTN"), 60) for k in range(3))      # several full members
    for name, text in [(n, texts[n]) for n in ("width60", "crlf_no_final_newline", "short_records_1000", "header_at_workgroup+0", "empty_file")] + [("big", big)]:
        plain, _ = assert_same_index(put(tmp_path, text, "plain.fa"), text)
        forms = {"bgzf": bam.bgzf_deflate(text), "gzip": gzip.compress(text)}
        if text:
            forms.update(cut1=F.bgzf_cut(text[:300], [1]) if name == "width60" else F.bgzf_cut(text, [17]),
                         cut17=F.bgzf_cut(text, [17, 1, 0xff00]), cut_empty_middle=F.bgzf_cut(text, [0xff00, 0, 17, 0, 1]))
        for form, data in forms.items():
            want = text[:300] if (form == "cut1" and name == "width60") else text
            path = put(tmp_path, data, f"{form}.fa.gz")
            with fasta.open_device(path) as dev:
                assert dev.text_len == len(want) and dev.read_text(0, len(want)) == want, (name, form)
                if want is text:
                    assert dev._index == plain == fasta.FastaFile(path)._index, (name, form)
    path = put(tmp_path, bam.bgzf_deflate(big), "runs.fa.gz")
    with fasta.open_device(path, run_bytes=40_000) as dev:                  # at least three runs appended into the one buffer
        assert dev.timing["runs"] >= 3 and dev.read_text(0, len(big)) == big and dev._index == fasta.FastaFile(path)._index
    with fasta.open_device(path, run_bytes=1) as dev:                       # a run holds at least one member
        assert dev.timing["runs"] == len(bam.bgzf_members(bam.bgzf_deflate(big))) and dev.read_text(0, len(big)) == big


def test_a_truncated_member_is_the_inflates_message(tier, tmp_path):
    rng = np.random.default_rng(2)
    text = F.record(b"a", F.bases(rng, 9000), 60)
    with pytest.raises(lib.SnifflesAmdError, match=r"^BGZF member 1: "):
        fasta.open_device(put(tmp_path, F.bgzf_truncated(text), "cut.fa.gz"))
    with pytest.raises(ValueError, match="truncated BGZF block"):          # the container itself cut short: the member walk says so
        fasta.open_device(put(tmp_path, bam.bgzf_deflate(text)[:-40], "short.fa.gz"))


# ------------------------------------------------------------------------------------------------------------- B. nmask
def nmask_contigs(nl: bytes):
    """[(header, sequence, width)]: the first base of the k-th contig lies at a chosen text offset modulo 16; singles on either side of
    every thread / wave / workgroup border, runs across them and across line ends."""
    out, pos = [], 0
    W = 60
    per = W + len(nl)

    def add(name, make_seq, mod=None, width=W):
        nonlocal pos
        head = name
        if mod is not None:                                                  # pad the name until the first base sits at `mod` (mod 16)
            while (pos + 1 + len(head) + len(nl)) % VEC != mod:
                head += b"_"
        first = pos + 1 + len(head) + len(nl)
        seq = make_seq(first)
        out.append((head, seq, width))
        pos = first + len(seq) + ((len(seq) + width - 1) // width) * len(nl)

    L = 3 * CHUNK

    def at_offsets(offsets_of_border, first):
        runs = []
        for b in range(VEC, first + L + L // W * len(nl), VEC):
            for off, ln in offsets_of_border(b):
                k = F.base_of_text_offset(off, first, W, len(nl))
                if k is not None:
                    runs.append((k, k + ln))
        return F.sequence_with_runs(L, runs)
    add(b"before", lambda first: at_offsets(lambda b: [(b - 1, 1)], first), mod=0)      # a single in the last byte of every word
    add(b"behind", lambda first: at_offsets(lambda b: [(b, 1)], first), mod=1)          # ... in the first byte of every word
    add(b"across", lambda first: at_offsets(lambda b: [(b - 3, 7)] if b % WAVE == 0 else [], first), mod=15)      # over wave and workgroup borders
    add(b"line_ends", lambda first: F.sequence_with_runs(L, [(W * k - 1, W * k + 1) for k in range(1, L // W, 3)] + [(W * 7 - 5, W * 9 + 5)]))
    add(b"ends", lambda first: F.sequence_with_runs(5000, [(0, 1), (4999, 5000), (100, 2300)]))
    add(b"ends_long", lambda first: F.sequence_with_runs(5000, [(0, 70), (4900, 5000)]))
    add(b"all_N", lambda first: b"N" * 4321)
    add(b"no_N", lambda first: F.sequence_with_runs(4321, []))
    add(b"lower", lambda first: F.sequence_with_runs(600, [(10, 20)], fill=b"ACnnGTn"))
    add(b"NANANA", lambda first: b"NA" * 5000)                                # the most intervals a range can hold
    add(b"narrow", lambda first: F.sequence_with_runs(700, [(0, 3), (50, 52), (698, 700)]), width=7)
    add(b"tiny", lambda first: b"N")
    return out


def regions_for(L):
    k = L // 3
    regs = [[(0, L)], [(k, k)], [(k, k + 1)], [(0, L + 50)], [(L, L + 5)], [(L + 3, L + 9)], [(0, 1)], [(L - 1, L)],
            [(k + 7, 2 * k), (5, k + 100), (k // 2, k // 2 + 900), (0, 40), (2 * k - 30, L)],      # unsorted, overlapping: the paint order
            [(0, L), (k, 2 * k)], None]
    return regs


def check_nmask(host, dev, contig, regions, contig_len):
    want = outcome(soa.paint_nmask, host.fetch, contig, regions, contig_len)
    got = outcome(dev.nmask, contig, regions, contig_len)
    if isinstance(want, tuple) and isinstance(want[0], np.ndarray):
        assert isinstance(got[0], np.ndarray), (contig, regions, got)
        for a, b in zip(got, want):
            assert a.dtype == b.dtype == np.int32 and a.shape == b.shape and np.array_equal(a, b), (contig, regions, contig_len, a[:8], b[:8])
    else:
        assert got == want, (contig, regions, contig_len)
    return want


@pytest.mark.parametrize("nl", [b"\n", b"\r\n"], ids=["lf", "crlf"])
@pytest.mark.parametrize("grid", [None, "1", "2", "7"])
def test_nmask_equals_paint_nmask(tier, tmp_path, monkeypatch, grid, nl):
    if grid:
        monkeypatch.setenv("SNF_FASTA_GRID", grid)
    contigs = nmask_contigs(nl)
    text = b"".join(F.record(h, s, w, nl) for h, s, w in contigs)[:-len(nl)]      # (the last contig without a newline)
    path = put(tmp_path, text)
    host = fasta.FastaFile(path)
    n_intervals = {}
    with fasta.open_device(path) as dev:
        assert dev._index == host._index
        assert sorted(host._index[h.decode()][1] % VEC for h, _, _ in contigs[:3]) == [0, 1, 15]
        for h, seq, _ in contigs:
            c, L = h.decode(), len(seq)
            runs = dev.nruns(c, 0, L)                                        # the kernel itself, not the fallback through fetch: these lines are regular
            assert runs is not None and all(np.array_equal(a, b) and a.dtype == np.int32 for a, b in zip(runs, soa.nmask_intervals(seq))), c
            for regions in regions_for(L):
                got = check_nmask(host, dev, c, regions, L)
                if regions == [(0, L)]:
                    n_intervals[c.rstrip("_")] = len(got[0])
            run = [(s, e) for s, e in zip(*soa.nmask_intervals(seq)) if e - s > 4]
            if run:                                                          # start / end inside a run
                s, e = int(run[0][0]), int(run[0][1])
                check_nmask(host, dev, c, [(s + 1, e - 1)], L)
                check_nmask(host, dev, c, [(max(0, s - 9), s + 2), (e - 2, min(L, e + 9))], L)
            for d in (-1, 1):                                                # a FASTA contig longer / shorter than the coverage vector
                check_nmask(host, dev, c, [(0, L)], L + d)
                check_nmask(host, dev, c, None, L + d)
                check_nmask(host, dev, c, [(L // 2, L // 2 + 1)], L + d)
        want = check_nmask(host, dev, "no_such_contig", [(0, 10)], 100)
        assert want[0] == "KeyError"
        assert check_nmask(host, dev, "no_N", [(-5, 10)], 4321)[0] == "ValueError"      # not the plain case: what fetch raises
    assert n_intervals["NANANA"] == 5000 and n_intervals["all_N"] == 1 and n_intervals["no_N"] == 0 and n_intervals["lower"] == 1
    assert min(n_intervals["before"], n_intervals["behind"]) > 0.9 * 3 * CHUNK / VEC and n_intervals["across"] >= 3 * CHUNK // WAVE


def test_nmask_of_irregular_lines_goes_through_fetch(tier, tmp_path):
    """Lines of another width than the first one's (no faidx-valid file): the range does not hold hi - lo bases, fa_nruns says so and
    `nmask` is `paint_nmask(self.fetch, ...)` - FastaFile's answer, whatever it is."""
    path = put(tmp_path, b">odd\nACGTNNAC\nNN\nACGTNNACGT\nNNNA\n>fine\nNNAC\nGTNN\n")
    host = fasta.FastaFile(path)
    with fasta.open_device(path) as dev:
        assert dev._index == host._index
        L = host.get_reference_length("odd")
        assert dev.nruns("odd", 0, L) is None and dev.nruns("fine", 0, 8) is not None
        for regions in ([(0, L)], [(2, 9)], None):
            check_nmask(host, dev, "odd", regions, L)
        check_nmask(host, dev, "fine", [(0, 8)], 8)


# -------------------------------------------------------------------------------------------------- C. fetch / fetch_many
@functools.lru_cache(None)
def fetch_text():
    rng = np.random.default_rng(31)
    return (F.record(b"long", F.bases(rng, 60_123, b"ACGTNNn"), 60) + F.record(b"crlf", F.bases(rng, 777, b"ACGTN"), 60, b"\r\n") +
            F.record(b"narrow", F.bases(rng, 400, b"ACGTN"), 1) + F.record(b"empty", b"", 60) + F.record(b"last", F.bases(rng, 131, b"ACGTN"), 60)[:-1])


def same_fetch(host, dev, contig, a, b):
    want, got = outcome(host.fetch, contig, a, b), outcome(dev.fetch, contig, a, b)
    assert got == want, (contig, a, b, got if not isinstance(got, str) else got[:40])
    return want


def test_fetch_equals_fastafile(tier, tmp_path):
    path = put(tmp_path, fetch_text())
    host = fasta.FastaFile(path)
    with fasta.open_device(path) as dev:
        L = host.get_reference_length("long")
        for n in (0, 1, STEP - 1, STEP, STEP + 1, 255, 256, 257, 50_000, 50_001):
            for a in (0, 59, 1234):                                          # (59: the last base of a line)
                s = same_fetch(host, dev, "long", a, a + n)
                assert len(s) == n
        for a, n in ((59, 1), (59, 2), (30, 31), (30, 61 + 30), (7, 100 * 60)):      # across 0, 1, 1, 2 and 100 line ends
            same_fetch(host, dev, "long", a, a + n)
        for c in host.references:
            Lc = host.get_reference_length(c)
            assert dev.fetch(c) == host.fetch(c)
            for a, b in ((0, Lc + 9), (Lc - 1, Lc + 9), (Lc, Lc + 3), (Lc, Lc), (Lc + 1, Lc + 3), (Lc + 5, 2), (-1, 5), (-3, -1), (7, 3), (3, -2),
                         (0, 0), (None, 5), (5, None), (2 ** 40, 2 ** 41), (0, 2 ** 70)):
                same_fetch(host, dev, c, a, b)
        assert same_fetch(host, dev, "chrZ", 0, 5)[0] == "KeyError" and outcome(dev.fetch, "chrZ") == outcome(host.fetch, "chrZ")
        assert same_fetch(host, dev, "long", 10, 5) == ("ValueError", "invalid coordinates: start (10) > stop (5)")
        assert same_fetch(host, dev, "long", -1, 5) == ("ValueError", "start out of range (-1)")
        assert dev.get_reference_length("last") == 131 and outcome(dev.get_reference_length, "chrZ") == outcome(host.get_reference_length, "chrZ")


def check_batch(host, dev, contig, starts, ends):
    pool, off, status, n_count = dev.fetch_many(contig, starts, ends)
    assert off.dtype == np.int64 and status.dtype == np.int32 and n_count.dtype == np.int32 and pool.dtype == np.uint8
    assert off[0] == 0 and len(off) == len(starts) + 1 and len(pool) == off[-1]
    raw = pool.tobytes()
    for k, (a, b) in enumerate(zip(starts, ends)):
        want = outcome(host.fetch, contig, int(a), int(b))
        got = raw[int(off[k]):int(off[k + 1])].decode()
        if isinstance(want, str):
            assert status[k] == abi.FASTA_OK and got == want and n_count[k] == want.count("N"), (contig, k, a, b)
        else:
            code = abi.FASTA_KEY_ERROR if want[0] == "KeyError" else abi.FASTA_START_NEGATIVE if "out of range" in want[1] else abi.FASTA_START_ABOVE_END
            assert status[k] == code and got == "" and n_count[k] == 0, (contig, k, a, b, want)


@pytest.mark.parametrize("grid", [None, "1", "2", "7"])
def test_fetch_many_keeps_order_offsets_and_counts(tier, tmp_path, monkeypatch, grid):
    if grid:
        monkeypatch.setenv("SNF_FASTA_GRID", grid)
    path = put(tmp_path, fetch_text())
    host = fasta.FastaFile(path)
    rng = np.random.default_rng(4)
    with fasta.open_device(path) as dev:
        L = host.get_reference_length("long")
        starts = rng.integers(-3, L + 5, 5000)
        ends = starts + rng.integers(-2, 200, 5000)
        starts[:6], ends[:6] = [0, L - 1, L, 59, 0, 5], [STEP, L + 70, L, 60, 0, STEP + 5 - 1]
        check_batch(host, dev, "long", starts, ends)
        for c in ("crlf", "narrow", "empty", "last", "nobody"):
            Lc = host.get_reference_length(c) if c in host.references else 50
            s = rng.integers(-1, Lc + 3, 150)
            check_batch(host, dev, c, s, s + rng.integers(-1, 3 * STEP, 150))
        check_batch(host, dev, "long", np.zeros(0, np.int64), np.zeros(0, np.int64))
        check_batch(host, dev, "long", [0, 2 ** 65], [2 ** 66, 2 ** 67])     # Python ints beyond 64 bits are clipped, not refused


def write_table_case(tmp_path, width, gz, fai):
    """The file of tests/test_fasta.py::test_fetch_equals_slicing."""
    rng = np.random.default_rng(3)
    seqs = {"chrA": "".join(rng.choice(list("ACGTN"), 1234)), "chrB desc": "".join(rng.choice(list("acgtN"), 61)), "chrC": "ACGT" * 30}
    text, index, pos = "", [], 0
    for k, v in seqs.items():
        head = f">{k}\n"
        body = "".join(v[i:i + width] + "\n" for i in range(0, len(v), width))
        index.append((k.split()[0], len(v), pos + len(head), width, width + 1))
        text += head + body
        pos += len(head) + len(body)
    p = tmp_path / ("ref.fa.gz" if gz else "ref.fa")
    p.write_bytes(gzip.compress(text.encode()) if gz else text.encode())
    if fai:
        (tmp_path / "ref.fa.fai").write_text("".join("\t".join(map(str, r)) + "\n" for r in index))
    return str(p), {k.split()[0]: v for k, v in seqs.items()}


@pytest.mark.parametrize("width,gz,fai", [(60, False, False), (7, False, True), (1000000, False, False), (50, True, False)])
def test_fetch_equals_slicing_on_the_device(tier, tmp_path, width, gz, fai):
    path, seqs = write_table_case(tmp_path, width, gz, fai)
    with fasta.open_device(path) as f:
        assert f.references == list(seqs)
        for c, s in seqs.items():
            assert f.fetch(c) == s and f.get_reference_length(c) == len(s)
            for a, b in [(0, 1), (5, 70), (59, 61), (60, 120), (len(s) - 3, len(s) + 50), (len(s), len(s) + 5), (17, 17)]:
                assert f.fetch(c, a, b) == s[a:b], (c, a, b)
        with pytest.raises(KeyError):
            f.fetch("chrZ")
        with pytest.raises(ValueError):
            f.fetch("chrA", 10, 5)


def test_refusals_carry_their_reason(tier, tmp_path):
    path = put(tmp_path, index_texts()["width60"])
    with fasta.open_device(path) as dev:
        with pytest.raises(lib.SnifflesAmdError, match=r"snf_fasta_nruns: \[5, 400\) is not a clipped range of a contig of 301 bases"):
            dev.nruns("c1", 5, 400)
        with pytest.raises(lib.SnifflesAmdError, match="snf_fasta_read_text: range outside the text"):
            dev.read_text(10, 10 ** 9)
        assert dev.fetch("c1", 0, 4) == fasta.FastaFile(path).fetch("c1", 0, 4)      # the handle goes on
    dev.close()                                                              # closing twice is fine


# --------------------------------------------------------------------------- D. the writer, against the reference's own text
def fake_fasta_file(tmp_path, contig, length, width=60):
    """vcf_util.FakeFasta's sequence for one contig as a FASTA file (its formula, vectorised)."""
    path = str(tmp_path / f"{contig}_{length}.fa")
    if not os.path.exists(path):
        i = np.arange(length, dtype=np.uint64)
        seq = np.frombuffer(vu.FakeFasta.ALPHABET.encode(), np.uint8)[((i * np.uint64(2654435761)) >> np.uint64(9)) & np.uint64(31)]
        out = np.full(length + (length + width - 1) // width, 10, np.uint8)
        out[np.arange(length) + np.arange(length) // width] = seq
        with open(path, "wb") as f:
            f.write(f">{contig} FakeFasta\n".encode() + out.tobytes())
        probe = vu.FakeFasta({contig: length})
        assert fasta.FastaFile(path).fetch(contig, 1000, 1100) == probe.fetch(contig, 1000, 1100)
    return path


def records_of_case(name, variant):
    build, kw, _ = cases.ALL[name]
    _, overrides, _ = vu.VARIANTS[variant]
    ti = build()
    cfg = gu.make_config({**kw, **overrides}, ti)
    for k, v in vu.FIXED.items():
        setattr(cfg, k, v)
    from test_dropin_api import leads_of
    lp = leadprov.LeadProvider(cfg, 0, ti.contig, contig_len=ti.contig_len)
    for ld in leads_of(ti):
        lp.record_lead(ld, int(ld.ref_start / cfg.cluster_binsize) * cfg.cluster_binsize)
    for s, e, hp in zip(ti.read_start.tolist(), ti.read_end.tolist(), ti.read_hp.tolist()):
        lp.record_read(s, e, hp)
    task = parallel.CallTask(id=ti.task_id, sv_id=ti.sv_id_start, contig=ti.contig, start=0, end=ti.contig_len, config=cfg, lead_provider=lp)
    task.tandem_repeats = None if ti.tr_start is None else list(zip(ti.tr_start.tolist(), ti.tr_end.tolist()))
    res, ti_used = task.call_records(cfg)
    return ti, cfg, task, res, ti_used


def text_from_records_with_device_fasta(tmp_path, name, variant):
    """tests/test_vcf.py::single_sample_text_from_records with a device-resident reference attached."""
    ti, cfg, task, res, ti_used = records_of_case(name, variant)
    with fasta.open_device(fake_fasta_file(tmp_path, ti.contig, ti.contig_len)) as ref:
        buf = io.StringIO()
        w = vcf.VCF(cfg, buf)
        w.reference_handle = ref
        assert w.can_write_records()
        w.write_header([(ti.contig, ti.contig_len)])
        keep = np.arange(len(res.calls)) if cfg.no_qc else np.flatnonzero(res.calls["qc"] != 0)
        keep = keep[np.argsort(res.calls["pos"][keep], kind="stable")]
        n = w.write_records(res, ti_used, keep)
        task.close()
        assert n == w.call_count
    return buf.getvalue()


def gold():
    from test_vcf import gold as g
    return g()


FASTA_VARIANTS = ["fasta", "symbolic_fasta"]
EMU_CASES = [c for c in vu.CASES if not c.startswith("chr")] + ["chr18_20x_auto_nm"]      # (as tests/test_vcf.py)


@pytest.mark.parametrize("variant", FASTA_VARIANTS)
@pytest.mark.parametrize("name", EMU_CASES)
def test_records_with_device_fasta_write_the_references_text_emu(tmp_path, name, variant):
    import emu.emu as E
    from test_vcf import assert_same_text
    E.lib()
    assert_same_text(text_from_records_with_device_fasta(tmp_path, name, variant), gold()["single"][name]["text"][variant])


@pytest.mark.gpu
@pytest.mark.parametrize("variant", FASTA_VARIANTS)
@pytest.mark.parametrize("name", vu.CASES)
def test_records_with_device_fasta_write_the_references_text_gpu(tmp_path, name, variant):
    from test_vcf import assert_same_text
    assert_same_text(text_from_records_with_device_fasta(tmp_path, name, variant), gold()["single"][name]["text"][variant])


def test_only_a_device_fasta_opens_the_record_writer(tmp_path):
    cfg = gu.make_config({}, cases.ALL["phase_rescue"][0]())
    for k, v in vu.FIXED.items():
        setattr(cfg, k, v)
    w = vcf.VCF(cfg, io.StringIO())
    assert w.can_write_records()
    for handle in (vu.FakeFasta({"c": 10}), fasta.FastaFile(put(tmp_path, b">c\nACGT\n"))):
        w.reference_handle = handle
        assert not w.can_write_records()


def features(text, plain=None):
    """What a compared text exercises of `_resolve_sequences`."""
    f = set()
    rows = [ln.split("\t") for ln in text.split("\n") if ln and ln[0] != "#"]
    for c in rows:
        ref, alt, info = c[3], c[4], c[7]
        if "SVTYPE=DEL" in info and len(ref) > 1 and len(alt) == 1 and alt == ref[0]:
            f.add("del_resolved")
        if "SVTYPE=DEL" in info and alt == "<NEL>" and len(ref) == 1:
            f.add("del_left_symbolic")
        if "SVTYPE=INS" in info and not alt.startswith("<") and ref != "N" and alt[0] == ref:
            f.add("ins_prepended")
        if "SVTYPE=BND" in info:
            m = re.fullmatch(r"(\w?)([\[\]])[^\[\]]+[\[\]](\w?)", alt)
            f.add("bnd_" + ("first" if m.group(1) else "second") + m.group(2))
        if alt.startswith("<") and alt not in ("<INS>", "<DEL>", "<DUP>", "<INV>", "<BND>"):
            f.add("symbolic_rewritten")
    if plain is not None:
        ids = {c[2] for c in rows}
        if any(".DEL." in ln.split("\t")[2] and ln.split("\t")[2] not in ids for ln in plain.split("\n") if ln and ln[0] != "#"):
            f.add("del_dropped")
    return f


FROM_GOLDENS = {"del_resolved", "ins_prepended", "bnd_first[", "bnd_second]", "symbolic_rewritten"}
FROM_DIRECTED = {"del_left_symbolic", "del_dropped", "bnd_first]", "bnd_second["}


def test_the_goldens_alone_hold_what_is_asserted_of_them():
    """Guard against a vacuous pass: the texts the cases above compare hold these forms (on both tiers' case lists); the forms no
    default configuration produces come from the directed cases below, whose test asserts them."""
    for names in (EMU_CASES, vu.CASES):
        seen = set()
        for name in names:
            t = gold()["single"][name]["text"]
            seen |= features(t["fasta"], t["plain"])
            assert features(t["symbolic_fasta"]) <= {"bnd_first[", "bnd_second]", "bnd_first]", "bnd_second["}      # nothing fetched under --symbolic
        assert FROM_GOLDENS <= seen, FROM_GOLDENS - seen


# ---- directed cases: write_records and write_call over the same hand-built records
DIRECTED_LEN = 5000


def directed_sequence():
    a = np.resize(np.frombuffer(b"ACGT", np.uint8), DIRECTED_LEN).copy()
    a[99:104] = 78          # [99, 109): five N of ten - exactly max_unknown_pct
    a[199:205] = 78         # [199, 209): six of ten - one above
    a[0] = ord("R")         # base 0 is an IUPAC letter
    a[449] = 78             # the base in front of pos 450 is N
    a[DIRECTED_LEN - 1] = ord("Y")
    return a.tobytes()


def directed_result(max_del_seq_len=None):
    """The finalized records of a small case, replaced by hand-built rows (the remaining fields are a real record's)."""
    ti, cfg, task, res, ti_used = records_of_case("single_leads_noqc", "fasta")
    task.close()
    assert ti.contig_len == DIRECTED_LEN
    base = res.calls[res.calls["svtype"] == soa.SVT["DEL"]][0]
    pool = b"ACRYGTKMACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTAC" + b"GATTACA" * 8
    rows = []

    def row(svtype, pos, svlen, **kw):
        r = base.copy()
        r["svtype"], r["pos"], r["svlen"], r["end"] = soa.SVT[svtype], pos, svlen, pos + abs(svlen) if svtype != "INS" else pos
        r["alt_len"], r["alt_off"], r["sv_id"], r["qc"], r["filter"], r["precise"] = -1, 0, len(rows) + 1, 1, 0, len(rows) % 2
        for k, v in kw.items():
            r[k] = v
        rows.append(r)
    row("DEL", 100, -9)                                   # N share exactly at max_unknown_pct: kept
    row("DEL", 200, -9)                                   # one N above it: dropped
    row("DEL", 0, -20)                                    # pos 0: start -1, the ValueError branch, then the base at 0 (an IUPAC letter)
    row("DEL", 1, -20)                                    # pos 1: the first base is part of REF
    row("DEL", DIRECTED_LEN - 5, -20)                     # reaches past the contig end: clipped
    row("DEL", DIRECTED_LEN, -3)                          # only the last base is left (an IUPAC letter; not "N": no one-base branch)
    row("DEL", 300, -10)                                  # around a lowered max_del_seq_len
    row("DEL", 320, -11)
    row("DEL", 340, -60_000)                              # above the default max_del_seq_len: left symbolic
    row("INS", 400, 54, alt_off=0, alt_len=54)            # a consensus with IUPAC letters
    row("INS", 1, 20, alt_off=54, alt_len=20)
    row("INS", 0, 56, alt_off=54, alt_len=56)
    row("INS", 450, 70, alt_off=0, alt_len=-1)            # "<INS>" stays symbolic and is rewritten; the fetched base is N
    row("INS", 460, 5, alt_off=3, alt_len=5)              # below minsvlen after SVLEN follows the sequence: not written
    row("DUP", 500, 300)
    row("INV", 600, 300)
    for k, (first, rev) in enumerate(((1, 0), (1, 1), (0, 0), (0, 1))):
        row("BND", 700 + 10 * k, 0, bnd_is_first=first, bnd_is_reverse=rev, mate_contig=0, mate_ref_start=1234 + k)
    row("BND", 0, 0, bnd_is_first=1, bnd_is_reverse=0, mate_contig=0, mate_ref_start=7)
    res.calls = np.array(rows, abi.CALL_DTYPE)
    res.alt_pool = np.frombuffer(pool, np.uint8).copy()
    if max_del_seq_len is not None:
        cfg.max_del_seq_len = max_del_seq_len
    return ti_used, cfg, res


def texts_of_both_writers(ti, cfg, res, host_ref, dev_ref):
    """(write_call over the materialised objects with the host reference, write_records with the device reference); an exception's
    type stands for the text it prevented."""
    def objects():
        calls = sv.materialize_candidates(res, ti, 0, len(res.calls))
        sv.apply_final(calls, res, ti, finalize=True)
        buf = io.StringIO()
        w = vcf.VCF(cfg, buf)
        w.reference_handle = host_ref
        n = sum(w.write_call(c) for c in calls)
        return buf.getvalue(), n

    def records():
        buf = io.StringIO()
        w = vcf.VCF(cfg, buf)
        w.reference_handle = dev_ref
        assert w.can_write_records()
        n = w.write_records(res, ti, np.arange(len(res.calls)))
        return buf.getvalue(), n
    out = []
    for fn in (objects, records):
        try:
            out.append(fn())
        except Exception as e:  # noqa: BLE001
            out.append(type(e).__name__)
    return out


def test_directed_records_equal_write_call(tier, tmp_path):
    seen = set()
    for max_del, symbolic in ((None, False), (10, False), (None, True)):
        ti, cfg, res = directed_result(max_del)
        cfg.symbolic = symbolic
        path = put(tmp_path, F.record(ti.contig.encode(), directed_sequence(), 60) + F.record(b"other", b"ACGT" * 10, 60))
        with fasta.open_device(path) as dev:
            a, b = texts_of_both_writers(ti, cfg, res, fasta.FastaFile(path), dev)
        assert not isinstance(a, str) and a == b, (max_del, symbolic)
        text, n = a
        assert ti.contig_name(0) == "chrT"
        rows = {ln.split("\t")[2].split(".")[2].split("S")[0]: ln.split("\t") for ln in text.split("\n") if ln}      # by sv_id (hex)
        ra = {k: (v[3], v[4]) for k, v in rows.items()}
        assert "E" not in rows and "B" not in rows and n == len(rows)      # INS below minsvlen
        if symbolic:                                                        # nothing is fetched: no line is dropped for its N share
            assert all(r[0] == "N" for r in ra.values()) and ra["1"] == ra["2"] == ("N", "<DEL>") and ra["11"] == ("N", "N[chrT:1234[")
            continue
        assert "2" not in rows and n == 18                                  # one N above max_unknown_pct: dropped and not counted
        seen |= features(text) | {"del_dropped"}
        assert ra["1"] == ("NNNNNACGTA", "N")                               # five N of ten: exactly max_unknown_pct, kept
        assert ra["3"] == ("N", "<NEL>")                                    # pos 0: the fetch fails, then base 0 ('R') through the IUPAC table
        assert ra["5"] == ("GTACGY", "G") if max_del is None else ra["5"] == ("G", "<NEL>")      # clipped at the contig end; a resolved REF is not translated
        assert ra["6"] == ("Y", "Y") and ra["7"] == ("TACGTACGTAC", "T")    # |svlen| 10 is resolved under either limit
        assert ra["8"] == (("TACGTACGTACG", "T") if max_del is None else ("T", "<NEL>"))      # |svlen| 11 around max_del_seq_len 10
        assert ra["4"] == (("RCGTACGTACGTACGTACGTA", "R") if max_del is None else ("N", "<NEL>"))
        assert ra["9"] == ("T", "<NEL>")                                    # above the default max_del_seq_len
        assert ra["A"][0] == "T" and ra["A"][1].startswith("TACNNGTNNACGT") and ra["C"][0] == "N" and ra["C"][1].startswith("NGATTACA")
        assert ra["D"] == ("N", "<INN>") and ra["F"] == ("T", "<NUP>") and ra["10"] == ("T", "<INN>")
        assert [ra[k] for k in ("11", "12", "13", "14", "15")] == [("T", "T[chrT:1234["), ("C", "C]chrT:1235]"), ("T", "[chrT:1236[T"),
                                                                   ("C", "]chrT:1237]C"), ("N", "N[chrT:7[")]
    assert FROM_DIRECTED <= seen, FROM_DIRECTED - seen
    # a contig the FASTA does not have: every fetch is the KeyError branch
    ti, cfg, res = directed_result()
    path = put(tmp_path, F.record(b"somebody_else", directed_sequence(), 60))
    with fasta.open_device(path) as dev:
        a, b = texts_of_both_writers(ti, cfg, res, fasta.FastaFile(path), dev)
    assert not isinstance(a, str) and a == b and a[1] == 19
    cols = [ln.split("\t") for ln in a[0].split("\n") if ln]
    assert all(c[3] == "N" for c in cols) and {c[4] for c in cols if ".DEL." in c[2]} == {"<NEL>"}
    # an empty fetch for a DEL: call.ref[0] fails on both paths
    ti, cfg, res = directed_result()
    res.calls["pos"][0] = DIRECTED_LEN + 10
    path = put(tmp_path, F.record(ti.contig.encode(), directed_sequence(), 60))
    with fasta.open_device(path) as dev:
        assert texts_of_both_writers(ti, cfg, res, fasta.FastaFile(path), dev) == ["IndexError", "IndexError"]


# ------------------------------------------------------------------------------------------------------------- E. drivers
@functools.lru_cache(None)
def two_contigs():
    return cases.SAMPLES["sample_two_contigs_12x"][0](), cases.SAMPLES["sample_two_contigs_12x"][1]


def fasta_with_N_blocks(recs, seed=11, frac=0.35):
    """FASTA text over the sample's contigs: random bases, IUPAC letters here and there, runs of 'N' of 200-6000 bp over about `frac`
    of every contig (many of a call's five coverage samples fall on masked positions), 60-base lines."""
    rng = np.random.default_rng(seed)
    out = []
    for name, n in zip(recs.ref_names, recs.ref_lens):
        n = int(n)
        a = rng.choice(np.frombuffer(b"ACGTACGTACGTRYKM", np.uint8), n)
        covered = 0
        while covered < frac * n:
            w = int(rng.integers(200, 6000))
            s = int(rng.integers(0, max(1, n - w)))
            a[s:s + w] = 78
            covered += w
        out.append(F.record(name.encode(), a.tobytes(), 60))
    return b"".join(out)


def driver_config(regions=None):
    from test_pipeline import config_for
    recs, args = two_contigs()
    cfg = config_for(args)
    if regions:
        cfg.regions_by_contig = {c: [(c, a, b) for a, b in rs] for c, rs in regions.items()}
    return recs, cfg


def sample_text(reference, objects, regions=None):
    recs, cfg = driver_config(regions)
    buf = io.StringIO()
    res = pipeline.call_sample(recs, cfg, vcf_handle=buf, tandem_repeats=getattr(recs, "tandem_repeats", None), objects=objects, reference=reference)
    return buf.getvalue(), res


def overlapping_regions(recs):
    c0, c1 = recs.ref_names[0], recs.ref_names[1]
    n0, n1 = int(recs.ref_lens[0]), int(recs.ref_lens[1])
    return {c0: [(n0 // 3, n0 - 100), (50, n0 // 2)], c1: [(0, n1 // 2)]}      # unsorted, overlapping


@pytest.mark.parametrize("with_regions", [False, True], ids=["whole", "regions"])
def test_call_sample_records_path_with_device_fasta(tier, tmp_path, with_regions):
    recs, _ = two_contigs()
    path = put(tmp_path, fasta_with_N_blocks(recs))
    regions = overlapping_regions(recs) if with_regions else None
    want, res_obj = sample_text(fasta.FastaFile(path), True, regions)
    with fasta.open_device(path) as dev:
        got, res = sample_text(dev, False, regions)
        assert got == want and res.vcf_records == res_obj.vcf_records > 3 and res.calls == {}      # the records path ran: no objects
        fallback, res_fb = sample_text(dev, True, regions)                  # objects=True with a DeviceFasta: the object path, the same text
        assert fallback == want and sum(len(v) for v in res_fb.calls.values()) >= res_fb.vcf_records
    if not with_regions:
        plain, _ = sample_text(None, False)
        assert plain != want and "\tN\t" in plain                            # the reference changed REF / ALT and the N mask the calls
    body = [ln.split("\t") for ln in want.split("\n") if ln and ln[0] != "#"]
    assert any(len(c[3]) > 1 for c in body) and all(c[3] != "" for c in body)


def test_genotype_vcf_with_device_fasta(tier, tmp_path):
    recs, _ = two_contigs()
    path = put(tmp_path, fasta_with_N_blocks(recs))
    targets, _ = sample_text(None, True)

    def run(reference):
        _, cfg = driver_config()
        out = io.StringIO()
        n = pipeline.genotype_vcf(recs, cfg, io.StringIO(targets), out, reference=reference)
        return out.getvalue(), n
    want = run(fasta.FastaFile(path))
    with fasta.open_device(path) as dev:
        assert run(dev) == want and want[1] > 3
    assert run(None) != want                                                 # the mask reached the genotypes


@pytest.mark.skipif(not __import__("make_ref").ref_root(), reason="needs the reference (its checkout, or the staged build oracle/_ref that make_ref.py compiles)")
def test_live_reference_writes_the_device_fasta_text(tmp_path):
    import emu.emu as E
    import ref_harness as rh
    from test_vcf import assert_same_text
    E.lib()
    recs, args = two_contigs()
    text = fasta_with_N_blocks(recs)
    path = put(tmp_path, text)
    host = fasta.FastaFile(path)
    exp = rh.run_reference_call_sample(recs, args, fixed=dict(vu.FIXED), fasta={c: host.fetch(c) for c in host.references})
    _, cfg = driver_config()
    cfg.reference = "reference.fa"
    buf = io.StringIO()
    with fasta.open_device(path) as dev:
        res = pipeline.call_sample(recs, cfg, vcf_handle=buf, tandem_repeats=getattr(recs, "tandem_repeats", None), objects=False, reference=dev)
    assert res.read_count == exp["read_count"]
    assert_same_text(buf.getvalue(), exp["vcf"])
