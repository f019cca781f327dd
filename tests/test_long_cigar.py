"""CIGARs of more than 65 535 operations: the placeholder `kSmN` and the CG:B,I tag (SAM/BAM spec 4.2.2), through the extraction
kernels (csrc/snf_extract.hip), the index kernels and the containers.  Tables: tests/long_cigar_cases.py.

Every check is written once and run on the host tier (the kernels compiled for the CPU, tests/emu) and, marked gpu, on the MI355X.
What a CG record is judged against is the oracle (oracle/extract_oracle.py), which reads inline CIGARs only: it is asked about the
same alignments written inline - above 65 535 operations about the twin whose adjacent M / = / X operations are merged, which the
builders show to be equivalent on the oracle itself - never about another form of the kernels.

On the tree before the feature the cases 1 (existing edges in CG form), 2 (the 16-bit edge), 3 (where the tag lies), 5 (l_seq == 0),
6 (split reads), 7 (errors) and 8 (containers) fail, and so does the second half of 9 (the writer could not pack the count); case 4
(records that only look the part) and the first half of 9 pass there.

Case 7's clip error is not the issue's "S in the middle of the array": M S M is no error for pysam, the oracle or the kernels (the
`where` table holds one as a record that must pass).  The shape that raises XE_CLIP is a hard clip inside a soft one, S H M ...
(long_cigar_cases.error_specs).  In the wave form the placeholder-shaped records of every table here go through the launch of their
own (x_wave_cg), the look-alikes of case 4 included; the thread form resolves them in place."""
import functools
import io
import struct

import numpy as np
import pytest

import long_cigar_cases as lc
import size_classes as sc
from test_extract_edges import TABLES, WAVES, assert_same, dev_tuple, grids, oracle_tuple, set_form, table, want

T = sc.extract_thresholds()
FORMS = (("wave", None, None), ("wave", 1, None), ("wave", 2, 8), ("thread", None, None))


@pytest.fixture
def emu_lib():
    from emu import emu
    return emu.lib()


LONG = {
    "edge": (lc.edge_specs, {}),
    "among": (lc.among_specs, {}),
    "where": (lc.where_specs, lc.SPLIT_CFG),
    "look": (lc.look_alike_specs, lc.LOOK_CFG),
    "noseq": (lc.noseq_specs, {}),
    "split": (lc.split_specs, lc.SPLIT_CFG),
}


@functools.lru_cache(maxsize=None)
def tables(name):
    """(the table, its twin)"""
    specs = LONG[name][0]()
    return lc.real(specs), lc.twin(specs)


@functools.lru_cache(maxsize=None)
def expected(name):
    """the oracle on the twin (the live-reference leg of oracle_tuple reads through a stand-in that does not know CG: not asked)"""
    return oracle_tuple(tables(name)[1], "c1", lc.WHOLE, LONG[name][1])


def check_table(name, forms, monkeypatch):
    recs, exp = tables(name)[0], expected(name)
    for form, grid, waves in forms:
        set_form(monkeypatch, form, grid, waves)
        assert_same(dev_tuple(recs, "c1", lc.WHOLE, LONG[name][1]), exp, f"table {name}, {form} form, grid {grid}, instance {waves}")


# ---- the tables hold what they are named for ----------------------------------------------------------------------------------
def test_the_tables_hold_what_they_are_named_for():
    step = T["step"]
    recs, tw = tables("edge")
    n_real = [len(s.ops) for s in lc.edge_specs()]
    assert n_real[:9] == [65534, 65534, 65535, 65535, 65536, 65537, 65536 + step - 1, 65536 + step, 65536 + step + 1]
    assert lc.inline_counts(recs) == [65534, 2, 65535, 2] + [2] * 6
    assert lc.inline_counts(tw)[:4] == [65534, 65534, 65535, 65535] and max(lc.inline_counts(tw)[4:]) < 16
    ev = lc.edge_events(n_real[8], T)
    assert sorted(ev) == [1, 65534, 65535, 65536, 65536 + step - 1] and (65536 + step - 1) % step == step - 1
    only = lc.edge_specs()[9].ops
    assert [k for k, (op, n) in enumerate(only) if op in (lc.I, lc.D, lc.S)] == [65536 + 17 * step + 5]
    assert len(expected("edge")[0]) > 30 and len(expected("edge")[1]) == 10
    recs, _ = tables("among")
    c = lc.inline_counts(recs)
    assert len(c) == 301 and c[150] == 2 and sorted(set(c) - {2}) == [5]
    recs, _ = tables("where")
    assert [a % 4 for a in lc.cg_offsets(recs)[6:14]] == [0, 1, 2, 3, 0, 1, 2, 3] and len({int(recs.blob[int(o) + 12]) for o in recs.rec_off[6:14]}) > 1
    aux = lc.aux_lengths(recs)
    for total in sc.around(T["xauxcap"]):
        assert aux.count(total) == 3, (total, aux)
    assert all(a >= 0 for a in lc.cg_offsets(recs))
    recs, tw = tables("look")
    assert recs.blob.tobytes() == tw.blob.tobytes()                   # these stay as they are written
    recs, _ = tables("noseq")
    assert all(struct.unpack_from("<i", recs.blob, int(o) + 20)[0] == 0 for o in recs.rec_off[:-1]) and lc.inline_counts(recs) == [2] * 5


# ---- 1. the existing edges in the new form ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cigar_in_cg_form():
    return lc.table_to_cg(table("cigar"))


def check_edges_capped_grids(waves, monkeypatch):
    """every record of extract_edges.cigar_table() rewritten as `kSmN` + CG: the result is that of the inline table, which has a
    fixture from the unmodified reference."""
    _, contig, region, cfg, _ = TABLES["cigar"]
    recs, exp = cigar_in_cg_form(), want("cigar")
    assert recs.n == table("cigar").n and set(lc.inline_counts(recs)) == {1, 2}
    for grid in grids(recs.n):
        set_form(monkeypatch, "wave", grid, waves)
        assert_same(dev_tuple(recs, contig, region, cfg), exp, f"table cigar in CG form, SNF_EXTRACT_GRID={grid}, SNF_EXTRACT_WAVES={waves}")


def check_edges_thread_form(monkeypatch):
    _, contig, region, cfg, _ = TABLES["cigar"]
    set_form(monkeypatch, "thread")
    assert_same(dev_tuple(cigar_in_cg_form(), contig, region, cfg), want("cigar"), "table cigar in CG form, thread form")


@pytest.mark.parametrize("waves", WAVES)
def test_existing_edges_in_cg_form_emu(waves, emu_lib, monkeypatch):
    check_edges_capped_grids(waves, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("waves", WAVES)
def test_existing_edges_in_cg_form_gpu(waves, monkeypatch):
    check_edges_capped_grids(waves, monkeypatch)


def test_existing_edges_in_cg_form_thread_emu(emu_lib, monkeypatch):
    check_edges_thread_form(monkeypatch)


@pytest.mark.gpu
def test_existing_edges_in_cg_form_thread_gpu(monkeypatch):
    check_edges_thread_form(monkeypatch)


# ---- 2. the 16-bit edge; 3. where the tag lies; 4. look-alikes; 5. l_seq == 0; 6. split reads ---------------------------------------
CASES = [("edge", FORMS[0:1] + FORMS[3:]), ("among", (("wave", 1, None), ("wave", 2, None), ("wave", None, None), ("thread", None, None))),
         ("where", FORMS), ("look", FORMS), ("noseq", FORMS), ("split", FORMS)]


@pytest.mark.parametrize("name,forms", CASES, ids=[c[0] for c in CASES])
def test_table_emu(name, forms, emu_lib, monkeypatch):
    check_table(name, forms, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("name,forms", CASES, ids=[c[0] for c in CASES])
def test_table_gpu(name, forms, monkeypatch):
    check_table(name, forms, monkeypatch)


def check_edge_instances(monkeypatch):
    """the 16-bit edge in the other instances of the wave form, one wave for everything among them."""
    check_table("edge", (("wave", 1, 4), ("wave", 2, 5), ("wave", None, 8)), monkeypatch)


def test_edge_instances_emu(emu_lib, monkeypatch):
    check_edge_instances(monkeypatch)


@pytest.mark.gpu
def test_edge_instances_gpu(monkeypatch):
    check_edge_instances(monkeypatch)


def test_look_alikes_count_as_reads():
    """the guard is not empty: under LOOK_CFG the placeholders without a usable tag are reads of no aligned base."""
    exp = expected("look")
    n = len(lc.look_alike_specs())
    assert len(exp[1]) == n - 2      # all but the unmapped one and the one on the other contig
    assert not any(r[11] == "INS" and r[12] == 99 for r in exp[0])      # (what the tags say)


# ---- 7. errors ------------------------------------------------------------------------------------------------------------------
ERROR_CASES = [(k, f) for k in sorted(lc.ERRORS) for f in (True, False)]


def check_first_error(kind, cg_first, monkeypatch):
    import extract_oracle as eo
    from sniffles_amd import lib
    recs, tw, first = lc.error_records(kind, cg_first)
    if tw is not None:
        with pytest.raises((eo.ExtractError, ValueError), match=dict(cigarop="CIGAR op", clip="clipping")[kind] if cg_first else "HP outside"):
            oracle_tuple(tw, "c1", lc.WHOLE, {})
    text = lc.ERRORS[kind] if cg_first else "HP tag outside"
    texts = set()
    for form, grid, waves in (("wave", None, None), ("wave", 1, None), ("wave", 2, 8), ("wave", recs.n - 1, 5), ("thread", None, None)):
        set_form(monkeypatch, form, grid, waves)
        with pytest.raises(lib.SnifflesAmdError, match=text) as e:
            dev_tuple(recs, "c1", lc.WHOLE, {})
        texts.add(str(e.value))
    assert len(texts) == 1, texts
    assert texts.pop().startswith(f"alignment record {first}: ")


@pytest.mark.parametrize("kind,cg_first", ERROR_CASES)
def test_first_error_in_bam_order_emu(kind, cg_first, emu_lib, monkeypatch):
    check_first_error(kind, cg_first, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,cg_first", ERROR_CASES)
def test_first_error_in_bam_order_gpu(kind, cg_first, monkeypatch):
    check_first_error(kind, cg_first, monkeypatch)


# ---- 8. through the containers --------------------------------------------------------------------------------------------------
@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def tier(request, monkeypatch):
    for k in ("SNF_BGZF_GRID", "SNF_BGZF_THREAD", "SNF_BAI_GRID", "SNF_BAI_THREAD", "SNF_EXTRACT_THREAD", "SNF_EXTRACT_GRID", "SNF_EXTRACT_WAVES"):
        monkeypatch.delenv(k, raising=False)
    if request.param == "emu":
        import emu.emu as E
        E.lib()
    return request.param


def sample_config():
    import vcf_util as vu
    from sniffles_amd.config import SnifflesConfig
    cfg = SnifflesConfig(all_contigs=True)
    for k, v in vu.FIXED.items():      # (command line and start date of the VCF header)
        setattr(cfg, k, v)
    return cfg


def vcf_of(recs):
    from sniffles_amd import pipeline
    buf = io.StringIO()
    pipeline.call_sample(recs, sample_config(), vcf_handle=buf)
    return buf.getvalue()


def vcf_calls(text):
    out = []
    for line in text.splitlines():
        if line.startswith("#"):
            continue
        f = line.split("\t")
        info = dict(kv.split("=", 1) for kv in f[7].split(";") if "=" in kv)
        out.append((f[0], int(f[1]), info["SVTYPE"], int(info["SVLEN"]), int(info["SUPPORT"])))
    return out


def dv_of(text):
    out = []
    for line in text.splitlines():
        if not line.startswith("#"):
            f = line.split("\t")
            out.append((f[0], f[1], dict(zip(f[8].split(":"), f[9].split(":")))["DV"]))
    return out


def test_through_the_containers(tier, tmp_path):
    from sniffles_amd import bam, pipeline
    recs, twins = lc.sample_records()
    long_ones = [k for k, r in enumerate(recs) if b"CGBI" in r]
    assert len(long_ones) == 2 * lc.N_LONG and len(recs) == 2 * lc.CARRIERS
    for k in long_ones:
        n = struct.unpack_from("<i", recs[k], recs[k].index(b"CGBI") + 4)[0]
        assert n > 65536 and struct.unpack_from("<H", recs[k], 16)[0] == 2 and struct.unpack_from("<H", twins[k], 16)[0] == 3
    paths = {}
    for name, rr in (("real", recs), ("twin", twins)):
        raw = bam.bam_stream(lc.SAMPLE_NAMES, lc.SAMPLE_LENS, rr)
        data = bam.bgzf_deflate(raw)
        (tmp_path / name).mkdir()
        paths[name] = str(tmp_path / name / "sample.bam")
        with open(paths[name], "wb") as f:
            f.write(data)
        if name == "real":      # a member border inside a CG array
            at = raw.index(b"CGBI") + 8
            n = struct.unpack_from("<i", raw, at - 4)[0]
            borders = bam.bgzf_members(data)["out_off"].tolist()
            assert any(at < b < at + 4 * n for b in borders)
    path = paths["real"]
    want_text = vcf_of(bam.read_bam(paths["twin"]))
    # the calls the plan names: a deletion's lead starts where the deleted bases start, an insertion's at the base it follows; POS is
    # that 0-based position written as it is, like the reference writes it
    assert vcf_calls(want_text) == [("k1", lc.DEL_AT, "DEL", -lc.DEL_LEN, lc.CARRIERS), ("k2", lc.INS_AT, "INS", lc.INS_LEN, lc.CARRIERS)]
    host = bam.read_bam(path)
    assert vcf_of(host) == want_text
    dev = bam.read_bam_device(path)
    try:
        assert vcf_of(dev) == want_text
    finally:
        dev.close()
    bai = bam.index_bam(path, out=path + ".bai")
    csi = bam.index_bam(path, fmt="csi")
    for ix in (None, csi):      # None: the .bai beside the file
        f = bam.open_indexed(path, index=ix)
        try:
            assert vcf_of(f) == want_text
        finally:
            f.close()
    assert bai is not None
    # the index kernels: end and bin of every record as of its twin (the placeholder's mN is the reference span)
    z = bam.BgzfDevice(0)
    try:
        got = {}
        for name in ("real", "twin"):
            with open(paths[name], "rb") as f:
                data = f.read()
            mem = bam.bgzf_members(data)
            foff = bam.member_file_offsets(mem)
            _, lens, hlen = bam.leading_header(data)
            z.inflate(data, mem, header_len=hlen)
            b, c = z.bai_run(foff, bam.window_offsets(lens)), z.csi_run(foff, bam.window_offsets(lens))
            got[name] = (b["end"].tolist(), b["bin"].tolist(), c["end"].tolist(), c["bin"].tolist())
        assert got["real"] == got["twin"] and len(got["real"][0]) == len(recs)
        assert max(e - struct.unpack_from("<i", recs[k], 8)[0] for k, e in enumerate(got["real"][0]) if k in long_ones) > 100000
    finally:
        z.close()
    # genotyping against the two calls
    outs = []
    for p in (path, paths["twin"]):
        o = io.StringIO()
        n = pipeline.genotype_vcf(bam.read_bam(p), sample_config(), io.StringIO(want_text), o)
        outs.append((n, o.getvalue()))
    assert outs[0] == outs[1] and outs[0][0] == 2
    assert [d[2] for d in dv_of(outs[0][1])] == [str(lc.CARRIERS)] * 2


# ---- 9. the writer ----------------------------------------------------------------------------------------------------------------
def _old_make_record(ref_id, pos, mapq, flag, qname, ops, seq_codes, tags):
    """the record layout, written out here (SAM/BAM spec 4.2): what make_record gave before it knew CG."""
    l_seq = len(seq_codes)
    name = qname.encode("ascii") + b"\0"
    sc_ = np.asarray(seq_codes, np.uint8)
    if l_seq & 1:
        sc_ = np.concatenate([sc_, np.zeros(1, np.uint8)])
    body = struct.pack("<iiBBHHHiiii", ref_id, pos, len(name), mapq, 4680, len(ops), flag, l_seq, -1, -1, 0) + name + \
        struct.pack(f"<{len(ops)}I", *[(n << 4) | op for op, n in ops]) + ((sc_[0::2] << 4) | sc_[1::2]).astype(np.uint8).tobytes() + b"\xff" * l_seq + tags
    return struct.pack("<i", len(body)) + body


def test_the_writer():
    from sniffles_amd import bam, synth_bam
    rng = np.random.default_rng(9)
    tags = lc.int_tag("NM", "C", 3) + lc.sa_tag(lc.el() + ";")
    for n in (1, 7, 65535):
        ops = lc.long_ops(n, {n // 2: (lc.D, 50)} if n > 2 else {})
        codes = rng.choice(np.array([1, 2, 4, 8], np.uint8), sum(k for op, k in ops if op in lc.QRY))
        assert synth_bam.make_record(0, 1000, 60, 0x10, "w", ops, codes, tags) == _old_make_record(0, 1000, 60, 0x10, "w", ops, codes, tags)
    ops = lc.long_ops(65536, {40000: (lc.D, 50), 50001: (lc.I, 60)}, lead_clip=20)
    codes = rng.choice(np.array([1, 2, 4, 8], np.uint8), sum(k for op, k in ops if op in lc.QRY))
    rec = synth_bam.make_record(0, 1000, 60, 0, "w", ops, codes, tags)
    span = sum(k for op, k in ops if op in lc.REF)
    assert struct.unpack_from("<H", rec, 16)[0] == 2
    assert struct.unpack_from("<2I", rec, 36 + 2) == ((len(codes) << 4) | lc.S, (span << 4) | lc.N)
    tail = lc.cg_tag(ops)
    assert rec.endswith(tail) and rec[-len(tail) - len(tags):-len(tail)] == tags and struct.unpack_from("<i", tail, 4)[0] == 65536
    forced = synth_bam.make_record(0, 1000, 60, 0, "w", ops[:9], codes[:sum(k for op, k in ops[:9] if op in lc.QRY)], [tags[:4], tags[4:]], cg=True, cg_at=1)
    assert forced.index(b"CGBI") == forced.index(b"SAZ") - len(lc.cg_tag(ops[:9])) and struct.unpack_from("<H", forced, 16)[0] == 2
    back = bam.parse_bam(bam.bam_stream(lc.CONTIGS, lc.CONTIG_LENS, [rec, forced]))
    assert back.n == 2 and back.blob.tobytes() == rec + forced and back.pos.tolist() == [1000, 1000]
