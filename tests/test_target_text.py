"""The target VCF of force calling resident on the device (sniffles_amd/csrc/snf_vcftext.h, `lib.VcfText`, `VCF.read_target_table_device`,
`VCF.rewrite_genotype_device`, `pipeline.genotype_vcf(targets_on_device=True)`).  The judge is always the host parser over the same
bytes - `read_target_table` / `read_svs_iter` / `rewrite_genotype_records` - and, where a golden exists (tests/golden/genotype_vcf.json.gz),
the unmodified reference's text; the device path is never compared with itself.  Every case runs on the host tier (the unchanged kernels
on the fibre stand-in) and, marked gpu, through the real library.  Builders: tests/target_text_cases.py."""
import functools
import gzip
import io
import types

import numpy as np
import pytest

import cases
import fasta_cases as F
import golden_util as gu
import target_text_cases as T
from sniffles_amd import abi, bam, bgzfout, fasta, lib, parallel, pipeline, sv, vcf
from sniffles_amd.config import SnifflesConfig
from test_genotype_records import GOOD, MALFORMED

GRIDS = [0, 1, 2, 7]


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def tier(request):
    if request.param == "emu":
        import emu.emu as E
        E.lib()
    return request.param


def host_table(text: bytes):
    r = vcf.VCF(SnifflesConfig(), io.BytesIO(text))
    return r.read_target_table(), r.header_str


def assert_same_table(text: bytes, source=None, **kw):
    """Every key of every contig's table, `header_str`, and `lines[i]` for all i; returns the device reader."""
    want, want_header = host_table(text)
    dev = vcf.VCF(SnifflesConfig(), None)
    got = dev.read_target_table_device(text if source is None else source, **kw)
    try:
        assert dev.header_str == want_header
        assert list(got) == list(want)                                     # contigs in order of first appearance
        for c in want:
            w, g = want[c], got[c]
            assert list(g) == list(w), c                                   # the same keys in the same order
            for k in w:
                if k == "lines":
                    assert len(g[k]) == len(w[k]) and [g[k][i] for i in range(len(w[k]))] == w[k], (c, k)
                elif isinstance(w[k], list):
                    assert g[k] == w[k], (c, k, g[k], w[k])
                else:
                    assert g[k].dtype == w[k].dtype and g[k].shape == w[k].shape and (g[k] == w[k]).all(), (c, k, g[k], w[k])
    finally:
        for t in got.values():
            t["lines"].close()
    return dev


# ----------------------------------------------------------------------------------------- 1. well-formed texts: nothing goes to the host
@pytest.mark.parametrize("name", ["sample_splits_14x", "sample_two_contigs_12x"])
def test_golden_target_texts(tier, name):
    text = gu.load("genotype_vcf")[name]["vcf_in"].encode()
    dev = assert_same_table(text)
    assert dev.n_host_lines == 0 and dev.host_lines == []
    assert sum(len(t["pos"]) for t in host_table(text)[0].values()) > 50


def test_the_directed_lines_need_no_fallback_on_the_host():
    """The reference parser alone reads every directed line, and reads what the case's name says."""
    rows = {}
    for what, ln in T.directed_lines():
        out = vcf.VCF._parse_target(ln.decode())
        rows[what] = out
    assert rows["ins_by_length"][7:10] == ("INS", 5, 99) and rows["del_by_length"][7:10] == ("DEL", -5, 94) and rows["equal_lengths"][7] == "DEL"
    assert rows["duplicate_keys"][7:10] == ("DEL", -5, 4) and rows["duplicate_bad_then_good"][8:10] == (50, 15)
    assert rows["tra"][7] == "BND" and rows["tra"][10] == ("chr2", 500, True, False)
    assert rows["prefix_keys"][7:10] == ("INS", 5, 99) and rows["prefix_then_real"][8:10] == (-6, 40)
    assert rows["eight_columns_svtype_last"][7] == "INS\n" and rows["eight_columns_flag_last"][8] == 4 and rows["eight_columns_end_last"][9] == 321
    assert rows["eight_columns_svlen_last_crlf"][8] == -44
    assert rows["bnd_]p]t"][10] == ("chr5", 300, False, True) and rows["bnd_[p[t"][10] == ("chr7", 400, False, False)
    assert rows["bnd_t]p]"][10] == ("chr6", 200, True, True) and rows["bnd_mixed_brackets"][10] == ("chr6", 5, True, True)
    assert rows["eighteen_digits"][1] == int("9" * T.DIGITS) - 1


@pytest.mark.parametrize("grid", GRIDS)
def test_directed_table(tier, grid):
    text = T.directed_text()
    dev = assert_same_table(text, max_grid=grid)
    assert dev.n_host_lines == 0
    want, _ = host_table(text)
    assert list(want) == ["chr1", "chr 1", "chr2", "chr3"]
    assert want["chr3"]["mate_names"] == ["chr5", "chr9"] and want["chr3"]["mate_contig"].tolist() == [0, 1, 0, -1]
    assert want["chr2"]["mate_names"][-1] == "chr9" and -1 in want["chr1"]["svtype"].tolist()
    assert want["chr1"]["line_index"][-1] > want["chr3"]["line_index"][0]                  # chr1 came back behind chr3
    dev = assert_same_table(text + b"\n", max_grid=grid)                                   # the last line with its '\n'
    assert dev.n_host_lines == 0


# ----------------------------------------------------------------------------------------- 2. the edges of the work units
@functools.lru_cache(None)
def edge_texts():
    out = dict(T.line_start_texts())
    keys = T.key_split_lines()
    out["keys_at_borders"] = T.aligned(keys)
    out["keys_at_borders_mod15"] = T.aligned(keys[::3], mod=15)
    out["keys_at_borders_mod1"] = T.aligned(keys[1::3], mod=1)
    out["lengths"] = T.aligned(T.length_lines())
    out["lengths_mod9"] = T.aligned(T.length_lines(), mod=9)
    for n in (1, 63, 64, 65):
        out[f"lines_{n}"] = T.many_lines(n)
    out["lines_65_no_header"] = T.many_lines(65)[len(T.HEAD):]
    out["chrom_runs"] = T.chrom_run_text()
    out["empty"] = b""
    out["header_only"] = T.HEAD
    out["header_only_no_newline"] = T.HEAD[:-1]
    return out


@pytest.mark.parametrize("grid", GRIDS)
def test_edges_of_the_work_units(tier, grid):
    for name, text in edge_texts().items():
        dev = assert_same_table(text, max_grid=grid)
        assert dev.n_host_lines == 0, name
    want, header = host_table(edge_texts()["chrom_runs"])
    assert list(want) == ["chrA", "b1x", "b2x_", "b2x", "b2y", "b3x"] and len(want["chrA"]["pos"]) > T.CHROM_WG - 3      # chrA came back
    assert host_table(b"")[0] == {} and host_table(T.HEAD) == ({}, T.HEAD.decode())
    long_alt = host_table(edge_texts()["lengths"])[0]["chr1"]
    assert 70_001 in long_alt["svlen"].tolist() and 5 in long_alt["svlen"].tolist() and 88 in long_alt["svlen"].tolist()


# ----------------------------------------------------------------------------------------- 3. fallback and errors
FRAME = "##fileformat=VCFv4.2\n#CHROM\tPOS\n" + GOOD + "\n"


def raised(fn):
    with pytest.raises(ValueError) as e:
        fn()
    return str(e.value), type(e.value.__cause__)


@pytest.mark.parametrize("name", sorted(MALFORMED))
def test_malformed_lines_raise_what_read_svs_iter_raises(tier, name):
    text = (FRAME + MALFORMED[name] + "\n" + GOOD + "\n").encode()
    want = raised(lambda: list(vcf.VCF(SnifflesConfig(), io.BytesIO(text)).read_svs_iter()))
    dev = vcf.VCF(SnifflesConfig(), None)
    got = raised(lambda: dev.read_target_table_device(text))
    assert got == want and "Line 4:" in want[0]
    assert dev.host_lines == [4]                                                             # ... and only that line went to the host


def test_of_two_malformed_lines_the_earlier_one_raises(tier):
    text = (FRAME + MALFORMED["info_with_two_equal_signs"] + "\n" + GOOD + "\n" + MALFORMED["pos_not_an_integer"] + "\n").encode()
    want = raised(lambda: list(vcf.VCF(SnifflesConfig(), io.BytesIO(text)).read_svs_iter()))
    dev = vcf.VCF(SnifflesConfig(), None)
    assert raised(lambda: dev.read_target_table_device(text)) == want and "Line 4:" in want[0]
    assert dev.host_lines == [4, 6]
    other = (FRAME + MALFORMED["bnd_mate_without_a_position"] + "\n" + MALFORMED["empty_line"] + "\n").encode()
    want = raised(lambda: list(vcf.VCF(SnifflesConfig(), io.BytesIO(other)).read_svs_iter()))
    assert raised(lambda: vcf.VCF(SnifflesConfig(), None).read_target_table_device(other)) == want and "Line 4:" in want[0]
    # an undecodable byte: the decoder's error, at its line
    bad = (FRAME.encode() + T.rec(tail="GT\t0/1\t\xe9") + GOOD.encode() + b"\n")
    want = raised(lambda: vcf.VCF(SnifflesConfig(), io.BytesIO(bad)).read_target_table())
    assert raised(lambda: vcf.VCF(SnifflesConfig(), None).read_target_table_device(bad)) == want and want[1] is UnicodeDecodeError


def test_two_equal_signs_in_any_item_raise_wherever_they_lie(tier):
    """An item of another key with two '=' raises in the reference (`key, value = item.split("=")`): the second '=' in the same word, in
    the next lane's word, a step later, in the first item and in the last one of an 8-column line."""
    infos = ["AA=1=2", "AA=1;BB=2=", "PRECISE;CC==3;SVLEN=5", "AA=" + "q" * 20 + "=1", "SVLEN=5;RNAMES=" + "r" * (T.STEP + 30) + "=x;END=9",
             "AA=1;" + "p" * (2 * T.STEP) + ";Z=1=2"]
    for k, info in enumerate(infos):
        for tail in ("GT\t0/1", None):
            text = T.HEAD + T.rec() + T.aligned([T.rec(info=info, tail=tail)], start=b"") + T.rec()
            want = raised(lambda: list(vcf.VCF(SnifflesConfig(), io.BytesIO(text)).read_svs_iter()))
            dev = vcf.VCF(SnifflesConfig(), None)
            assert raised(lambda: dev.read_target_table_device(text)) == want and "too many values to unpack" in want[0], info
            assert len(dev.host_lines) == 1
    # ... and '=' signs that are one per item never do, however close
    ok = T.HEAD + T.rec(info="A=1;B=2;C=;=D;E=" + "e" * T.STEP + ";F=1")
    assert assert_same_table(ok).n_host_lines == 0


@pytest.mark.parametrize("grid", [0, 2])
def test_unusual_but_legal_lines_go_to_the_host_and_come_out_as_the_host_reads_them(tier, grid):
    lines, expect = [], []
    good = [T.rec(), T.rec(chrom="chr2", alt="N[chr5:9[", info="SVTYPE=BND"), T.rec(chrom="chr2", info="SVLEN=3", tail=None)]
    text = T.HEAD
    n = T.HEAD.count(b"\n")
    for k, (what, ln) in enumerate(T.unusual_lines()):
        text += good[k % 3] + ln
        n += 2
        expect.append(n)
    text += good[0]
    dev = assert_same_table(text, max_grid=grid)
    assert dev.host_lines == expect and dev.n_host_lines == len(expect)
    want, header = host_table(text)
    assert " ##indented header".strip() in header and "café" in header
    assert 6 in want["chr1"]["svlen"].tolist() or 7 in want["chr1"]["svlen"].tolist()      # "SVLEN= 7" was read


# ----------------------------------------------------------------------------------------- 4. load
def test_plain_bgzf_and_gzip_give_the_same_table(tier, tmp_path):
    text = T.directed_text() + b"\n" + T.aligned(T.length_lines()[:14], start=b"")
    cut_in_line = text.index(b"SVTYPE=DUP") + 3                           # a member ends inside `SVTYPE=`
    cut_at_newline = text.index(b"\n", 2000) + 1
    forms = {"plain": text, "bgzf": bam.bgzf_deflate(text), "gzip": gzip.compress(text),
             "cut_inside_a_key": F.bgzf_cut(text, [cut_in_line, 0xff00]), "cut_at_a_newline": F.bgzf_cut(text, [cut_at_newline, 17, 0, 0xff00]),
             "cut_inside_lines": F.bgzf_cut(text, [1000])}
    for form, data in forms.items():
        dev = assert_same_table(text, source=data)
        assert dev.n_host_lines == 0, form
        p = tmp_path / f"{form}.vcf.gz"
        p.write_bytes(data)
        assert_same_table(text, source=str(p))
    dev = assert_same_table(text, source=forms["cut_inside_lines"], run_bytes=1)      # a run per member
    assert dev.target_timing["runs"] == len(bam.bgzf_members(forms["cut_inside_lines"]))
    with pytest.raises(TypeError, match="not an open handle"):
        vcf.VCF(SnifflesConfig(), None).read_target_table_device(io.BytesIO(text))


def test_a_truncated_member_is_the_inflates_message(tier):
    text = T.many_lines(150)
    assert len(text) > 6000
    with pytest.raises(lib.SnifflesAmdError, match=r"^BGZF member 1: "):
        vcf.VCF(SnifflesConfig(), None).read_target_table_device(F.bgzf_truncated(text))
    with pytest.raises(ValueError, match="truncated BGZF block"):
        vcf.VCF(SnifflesConfig(), None).read_target_table_device(bam.bgzf_deflate(text)[:-40])


# ----------------------------------------------------------------------------------------- 5. writer
def hand_made_gt(n: int) -> np.ndarray:
    """[n, 8] rows as `execute_records` returns them (a, b, GQ, DR, DV, hp, ps, source): every source, unphased and both haplotypes, the
    phase set a name, NULL and none; most rows share a few tuples."""
    M, D, N = abi.GTSRC_MATCH, abi.GTSRC_DEPTH, abi.GTSRC_NONE
    kinds = [(0, 1, 30, 5, 6, -1, -1, M), (0, 1, 30, 5, 6, 1, 3, M), (0, 1, 30, 5, 6, 2, 3, M), (1, 1, 60, 0, 9, 1, -2, M), (1, 1, 60, 0, 9, 2, -1, M),
             (0, 0, 12, 8, 0, 1, 4, M), (0, 0, 0, 17, 0, -1, -1, D), (0, 0, 0, 0, 0, -1, -1, N), (0, 0, 0, 3, 0, -1, -1, D)]
    rows = [kinds[k % len(kinds)] if k % 4 else kinds[1] for k in range(n)]
    return np.asarray(rows, np.int32)


def tuples_of(cfg):
    task = types.SimpleNamespace(config=cfg, _ti=types.SimpleNamespace(ps_name=lambda code: str(7000 + code)))
    return lambda g: parallel.GenotypeTask.genotype_tuples(task, {"gt": g})


@pytest.mark.parametrize("phase", [False, True])
def test_rewrite_equals_rewrite_genotype_records(tier, tmp_path, phase):
    cfg = SnifflesConfig()
    cfg.phase = phase
    text = T.directed_text() + b"\n" + T.aligned([T.rec(tail=None, nl="\r\n"), T.rec(ident="L" * (T.STEP + 7)), T.length_lines()[12]], start=b"")
    want_tab, _ = host_table(text)
    to_tuples = tuples_of(cfg)
    got_tab = vcf.VCF(cfg, None).read_target_table_device(text)
    try:
        seen = set()
        for c in want_tab:
            n = len(want_tab[c]["lines"])
            gt = hand_made_gt(n)
            tuples = to_tuples(gt)
            seen |= set(tuples)
            a = io.StringIO()
            assert vcf.VCF(cfg, a).rewrite_genotype_records(want_tab[c]["lines"], tuples) == n
            for grid in (None, 1, 2, 7):
                b = io.StringIO()
                assert vcf.VCF(cfg, b).rewrite_genotype_device(got_tab[c]["lines"], None, gt, tuples=to_tuples, max_grid=grid) == n
                assert b.getvalue() == a.getvalue(), (c, grid)
            b = io.StringIO()                                                                 # the tuples themselves
            assert vcf.VCF(cfg, b).rewrite_genotype_device(got_tab[c]["lines"], None, tuples) == n and b.getvalue() == a.getvalue()
            # a selection in another order, as `select_targets` and `rows` give it
            pick = np.arange(n)[::-2]
            a = io.StringIO()
            vcf.VCF(cfg, a).rewrite_genotype_records([want_tab[c]["lines"][i] for i in pick.tolist()], [tuples[i] for i in pick.tolist()])
            b = io.StringIO()
            assert vcf.VCF(cfg, b).rewrite_genotype_device(got_tab[c]["lines"], pick, gt[pick], tuples=to_tuples) == len(pick)
            assert b.getvalue() == a.getvalue()
            sub = vcf.VCF.select_targets(got_tab[c], np.arange(n) % 2 == 0)
            assert [sub["lines"][i] for i in range(len(sub["lines"]))] == want_tab[c]["lines"][::2]
        assert cfg.genotype_none in seen and (0, 0, 0, 17, 0, (None, None)) in seen and (1, 1, 60, 0, 9, ("1", "NULL")) in seen
        assert "extra" not in a.getvalue() and "\t0/1:5" not in a.getvalue()
        # through the bgzipped writer, inflated back
        c = "chr1"
        gt = hand_made_gt(len(want_tab[c]["lines"]))
        a = io.StringIO()
        vcf.VCF(cfg, a).rewrite_genotype_records(want_tab[c]["lines"], to_tuples(gt))
        gz = str(tmp_path / "out.vcf.gz")
        with bgzfout.BgzfWriter(gz) as w:
            vcf.VCF(cfg, w).rewrite_genotype_device(got_tab[c]["lines"], None, gt, tuples=to_tuples)
        with gzip.open(gz, "rb") as f:
            assert f.read().decode() == a.getvalue()
    finally:
        for t in got_tab.values():
            t["lines"].close()


@pytest.mark.parametrize("index", ["tbi", "csi"])
def test_rewrite_through_vcf_gz_writer(tier, tmp_path, index):
    """`bgzfout.VcfGzWriter` reads the lines it is given (interval, sort order) to build its index: it gets one block of many lines
    per contig from the device writer and single strings from the host's.  Sorted tables: the golden targets and `many_lines`; the
    file inflated back is `rewrite_genotype_records`' text and the index beside it is the one the host writer's file gets."""
    cfg = SnifflesConfig()
    lines = gu.load("genotype_vcf")["sample_two_contigs_12x"]["vcf_in"].split("\n")
    body = [ln for ln in lines if ln and not ln.startswith("#")]
    order = {c: k for k, c in enumerate(dict.fromkeys(ln.split("\t")[0] for ln in body))}
    body.sort(key=lambda ln: (order[ln.split("\t")[0]], int(ln.split("\t")[1])))              # (the golden targets end in a few unsorted ones)
    golden = ("\n".join([ln for ln in lines if ln.startswith("#")] + body) + "\n").encode()
    for name, text in (("golden", golden), ("many_lines", T.many_lines(200, per=70))):
        want_tab, header = host_table(text)
        got_tab = vcf.VCF(cfg, None).read_target_table_device(text)
        try:
            assert len(want_tab) >= 2
            files = {}
            for who in ("host", "device"):
                gz = str(tmp_path / f"{name}_{who}.vcf.gz")
                with bgzfout.VcfGzWriter(gz, index=index) as w:
                    out = vcf.VCF(cfg, w)
                    w.write(header)
                    n = 0
                    for c in want_tab:
                        gt = hand_made_gt(len(want_tab[c]["lines"]))
                        if who == "host":
                            n += out.rewrite_genotype_records(want_tab[c]["lines"], tuples_of(cfg)(gt))
                        else:
                            n += out.rewrite_genotype_device(got_tab[c]["lines"], None, gt, tuples=tuples_of(cfg))
                with gzip.open(gz, "rb") as f:
                    files[who] = f.read()
                with open(gz + "." + index, "rb") as f:
                    files[who + "_index"] = gzip.decompress(f.read())
                assert n == sum(len(t["lines"]) for t in want_tab.values()) > 100
            assert files["device"] == files["host"] and files["device"].startswith(header.encode()) and files["device"].count(b"\n") == n + header.count("\n")
            assert files["device_index"] == files["host_index"] and files["device_index"][:4] == (b"TBI\x01" if index == "tbi" else b"CSI\x01")
        finally:
            for t in got_tab.values():
                t["lines"].close()
    # an unsorted table is refused by the writer, whoever writes: the contig of the directed text that comes back
    text = T.directed_text()
    got_tab = vcf.VCF(cfg, None).read_target_table_device(text)
    try:
        with pytest.raises(ValueError, match="a tabix index needs"):
            with bgzfout.VcfGzWriter(str(tmp_path / "unsorted.vcf.gz"), index=index) as w:
                for c in got_tab:
                    vcf.VCF(cfg, w).rewrite_genotype_device(got_tab[c]["lines"], None, hand_made_gt(len(got_tab[c]["lines"])), tuples=tuples_of(cfg))
    finally:
        got_tab["chr1"]["lines"].close()


def test_distinct_rows_is_the_row_wise_unique():
    """`vcf._distinct_rows` against `np.unique(axis=0, return_inverse=True)`: the same set of rows, `rows[inverse]` the input - on the
    fast path and on both ways into the fallback (cardinalities whose product passes 2^62; a table that is not of integers)."""
    rng = np.random.default_rng(4)
    tables = {"few_values": rng.integers(-3, 4, (500, 8)).astype(np.int32), "one_row": np.asarray([[1, 2, 3]], np.int64),
              "all_equal": np.zeros((9, 8), np.int32), "hand_made": hand_made_gt(300),
              "fallback_wide": rng.integers(-2 ** 31, 2 ** 31 - 1, (3000, 8)).astype(np.int32),      # 3000^8 > 2^62
              "fallback_float": rng.integers(0, 3, (40, 4)).astype(np.float64), "empty": np.zeros((0, 8), np.int32)}
    assert 3000 ** 6 >= 1 << 62
    for name, a in tables.items():
        rows, inverse = vcf._distinct_rows(a)
        want, want_inverse = np.unique(a, axis=0, return_inverse=True)
        assert (rows[np.asarray(inverse).reshape(-1)] == a).all(), name
        assert rows.shape == want.shape and (np.unique(rows, axis=0) == want).all(), name
        assert len(np.asarray(inverse).reshape(-1)) == len(a) == len(np.asarray(want_inverse).reshape(-1)), name


def test_errors_name_the_vcf_text(tier):
    """The text buffer and its loaders are shared with the device FASTA; what they refuse on this handle is reported as this handle's."""
    import ctypes as C
    with lib.VcfText(b"abc\n") as t:
        more = np.frombuffer(b"0123456789", np.uint8)
        assert t.lib.snf_vcftext_load_text(t._h, more.ctypes.data, 10) != 0
        assert t.lib.snf_vcftext_last_error().decode() == "snf_vcftext: 10 more bytes behind 4 do not fit the 4 bytes the handle was created for"
        assert t.lib.snf_vcftext_load_bgzf(t._h, None, 5, None, 0, C.byref(C.c_float())) != 0
        assert t.lib.snf_vcftext_last_error().decode() == "snf_vcftext_load_bgzf: null argument"
        assert t.strings([0], [4]) == [b"abc\n"]                                            # the handle is as it was


def test_rewrite_splices_the_rows_the_host_parsed(tier):
    cfg = SnifflesConfig()
    text = T.HEAD + T.rec() + T.rec(pos="+5", tail="GT:XX\t0/1:5\textra") + T.rec(info="SVLEN=9") + T.rec(info="SVLEN= 7", tail=None) + T.rec(pos="1_0")
    want_tab, _ = host_table(text)
    dev = vcf.VCF(cfg, None)
    got_tab = dev.read_target_table_device(text)
    try:
        assert dev.host_lines == [4, 6, 7]
        gt = hand_made_gt(5)
        a, b = io.StringIO(), io.StringIO()
        vcf.VCF(cfg, a).rewrite_genotype_records(want_tab["chr1"]["lines"], tuples_of(cfg)(gt))
        vcf.VCF(cfg, b).rewrite_genotype_device(got_tab["chr1"]["lines"], None, gt, tuples=tuples_of(cfg))
        assert b.getvalue() == a.getvalue() and a.getvalue().count("\n") == 5 and "extra" not in a.getvalue()
    finally:
        got_tab["chr1"]["lines"].text.close()


# ----------------------------------------------------------------------------------------- 6. driver
@pytest.mark.parametrize("name", ["sample_splits_14x", "sample_two_contigs_12x"])
def test_driver_writes_the_reference_text(tier, tmp_path, name):
    from test_pipeline import config_for, records_sha
    doc = gu.load("genotype_vcf")[name]
    recs = cases.SAMPLES[name][0]()
    assert records_sha(recs) == doc["input_sha"]
    plain = io.StringIO()
    n0 = pipeline.genotype_vcf(recs, config_for(()), io.StringIO(doc["vcf_in"]), plain, objects=False)
    assert plain.getvalue() == doc["vcf_out"]
    raw = doc["vcf_in"].encode()
    path, gz = tmp_path / "targets.vcf", tmp_path / "targets.vcf.gz"
    path.write_bytes(raw)
    gz.write_bytes(bam.bgzf_deflate(raw))
    for source in (str(path), raw, str(gz)):
        buf, tm = io.StringIO(), {}
        n = pipeline.genotype_vcf(recs, config_for(()), source, buf, objects=False, targets_on_device=True, timing=tm)
        assert buf.getvalue() == doc["vcf_out"] and n == n0 > 50
        assert tm["n_host_lines"] == 0 and tm["parse_kernel_ms"] > 0 and {"read", "extract", "pass_match", "text", "match_kernel_ms"} <= set(tm)


def test_driver_frees_the_text_when_a_contig_raises(tier, monkeypatch):
    doc = gu.load("genotype_vcf")["sample_splits_14x"]
    recs = cases.SAMPLES["sample_splits_14x"][0]()
    seen = []
    real = vcf.VCF.rewrite_genotype_device

    def failing(self, lines_obj, *a, **kw):
        seen.append(lines_obj.text)
        assert lines_obj.text._h
        raise RuntimeError("the writer failed")
    monkeypatch.setattr(vcf.VCF, "rewrite_genotype_device", failing)
    from test_pipeline import config_for
    with pytest.raises(RuntimeError, match="the writer failed"):
        pipeline.genotype_vcf(recs, config_for(()), doc["vcf_in"].encode(), io.StringIO(), objects=False, targets_on_device=True)
    assert len(seen) == 1 and not seen[0]._h                                                  # closed, not left to the collector
    monkeypatch.setattr(vcf.VCF, "rewrite_genotype_device", real)


def test_driver_refuses_a_handle_and_the_object_path(tier):
    recs = cases.SAMPLES["sample_splits_14x"][0]()
    with pytest.raises(TypeError, match="a path or the file's bytes, not an open handle"):
        pipeline.genotype_vcf(recs, SnifflesConfig(), io.StringIO("x"), io.StringIO(), objects=False, targets_on_device=True)
    with pytest.raises(ValueError, match="needs objects=False"):
        pipeline.genotype_vcf(recs, SnifflesConfig(), b"x", io.StringIO(), targets_on_device=True)


@pytest.mark.parametrize("variant", ["regions", "device_fasta"])
def test_driver_with_regions_and_with_a_device_reference(tier, tmp_path, variant):
    from test_pipeline import config_for
    name = "sample_splits_14x"
    doc = gu.load("genotype_vcf")[name]
    recs = cases.SAMPLES[name][0]()
    out = {}
    ref = None
    if variant == "device_fasta":
        rng = np.random.default_rng(3)
        fa = b"".join(F.record(c.encode(), F.sequence_with_runs(int(n), [(s, s + 2500) for s in range(3000, int(n) - 4000, 90_000)]), 60)
                      for c, n in zip(recs.ref_names, recs.ref_lens))
        p = tmp_path / "ref.fa"
        p.write_bytes(fa)
        ref = fasta.open_device(str(p))
    try:
        for on_device in (False, True):
            cfg = config_for(())
            if variant == "regions":
                big = [(c, int(n)) for c, n in zip(recs.ref_names, recs.ref_lens) if n >= 1_000_000]
                cfg.regions_by_contig = {c: [(c, n // 10, n // 2), (c, n // 3, n - 1000)] for c, n in big[:1]}
            buf = io.StringIO()
            src = doc["vcf_in"].encode() if on_device else io.StringIO(doc["vcf_in"])
            n = pipeline.genotype_vcf(recs, cfg, src, buf, objects=False, targets_on_device=on_device, reference=ref)
            out[on_device] = (n, buf.getvalue())
    finally:
        if ref is not None:
            ref.close()
    assert out[True] == out[False] and out[True][0] > 50
    assert out[True][1] != doc["vcf_out"]                                                    # (the option matters on this sample)
