"""Directed cases at the internal edges of the extraction kernels (csrc/snf_extract.hip; tables: tests/extract_edges.py, boundary
numbers: size_classes.extract_thresholds()): the wave form whose waves take several records (SNF_EXTRACT_GRID) in every instance
(SNF_EXTRACT_WAVES), the segment table, the chunks of the NM sum, the blocks of the thread form, the first error in BAM order, a
handle used for several tables.

Every check is written once (check_*) and run on the host tier (the kernels compiled for the CPU, tests/emu) and, marked gpu, on the
MI355X.  What a form is judged against is always the oracle (oracle/extract_oracle.py) - and the unmodified reference itself where its
checkout or staged build is there - never another form of the kernels."""
import functools

import numpy as np
import pytest

import extract_edges as xe
import extract_util as xu
import size_classes as sc
from test_extract import DevCfg

T = sc.extract_thresholds()
WAVES = T["wave_instances"]                # the instances x_launch_wave selects between
assert WAVES == (4, 5, 6, 8) and T["waves"] in WAVES
WHOLE = (0, 400000)                        # all of contig c1
MANY = dict(max_splits_base=100)


@pytest.fixture
def emu_lib():
    from emu import emu
    return emu.lib()


# ---- tables and what the oracle (and the reference) make of them: built once --------------------------------------------------
TABLES = {
    "cigar": (xe.cigar_table, "c1", xe.REGION, xe.CIGAR_CFG, ("--long-ins-length", "2501", "--dev-seq-cache-maxlen", "400")),
    "sa": (xe.sa_table, "c1", WHOLE, MANY, ("--max-splits-base", "100")),
    "tags": (xe.tags_table, "c1", WHOLE, {}, ()),
    "mixed": (xe.mixed_table, "c1", WHOLE, MANY, ("--max-splits-base", "100")),
}
READ_ID_OFFSET = 17


@functools.lru_cache(maxsize=None)
def table(name):
    return TABLES[name][0]()


def oracle_tuple(recs, contig, region, cfg, read_id_offset=READ_ID_OFFSET, args=None):
    """(rows, reads, qc_nm_threshold hex, read_id) of the oracle; with `args` (the same settings as reference arguments) and the
    reference at hand, the unmodified reference must say the same first."""
    import extract_oracle as eo
    import make_ref
    out = eo.extract_region(recs.blob, recs.rec_off, recs.ref_names, contig, region[0], region[1], eo.Cfg(**cfg), read_id_offset)
    if args is not None and make_ref.ref_root():
        import ref_harness as rh
        ref = rh.run_reference_extract(recs, contig, region[0], region[1], args, read_id_offset, {})
        assert "error" not in ref, ref
        assert ref["leads"] == out["rows"] and ref["qc_nm_threshold"] == out["qc_nm_threshold"] and ref["read_id"] == out["read_id"]
        assert len(out["reads"]) == ref["read_count"]
    return out["rows"], out["reads"], out["qc_nm_threshold"], out["read_id"]


@functools.lru_cache(maxsize=None)
def want(name):
    _, contig, region, cfg, args = TABLES[name]
    return oracle_tuple(table(name), contig, region, cfg, args=args)


def dev_tuple(recs, contig, region, cfg, read_id_offset=READ_ID_OFFSET):
    from sniffles_amd import extract
    ti, info = extract.extract_region(recs, contig, region[0], region[1], DevCfg(**cfg), read_id_offset)
    reads = list(zip(ti.read_start.tolist(), ti.read_end.tolist(), ti.read_hp.tolist()))
    assert np.all(np.diff(ti.leads["read_id"].astype(np.int64)) >= 0), "leads out of record order"
    assert info.read_count == len(reads)
    return xu.canon_leads(ti), reads, float(ti.qc_nm_threshold).hex(), info.read_id


def set_form(monkeypatch, form="wave", grid=None, waves=None):
    for k, v in (("SNF_EXTRACT_THREAD", "1" if form == "thread" else None), ("SNF_EXTRACT_GRID", grid), ("SNF_EXTRACT_WAVES", waves)):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, str(v))


def assert_same(got, exp, what):
    for part, g, e in zip(("leads", "reads", "qc_nm_threshold", "read_id"), got, exp):
        if part == "leads" and g != e:
            first = next((k for k, (a, b) in enumerate(zip(g, e)) if a != b), min(len(g), len(e)))
            raise AssertionError(f"{what}: {len(g)} leads, the oracle has {len(e)}; first difference at lead {first}: "
                                 f"{g[first] if first < len(g) else None} != {e[first] if first < len(e) else None}")
        assert g == e, f"{what}: {part} differs from the oracle"


def grids(n):
    """one wave for everything, two, a count that divides nothing, one short of a wave per record, a wave per record, the default."""
    assert n < T["grid_cap"]
    return (1, 2, 7, n - 1, n, None)


# ---- capped grids and instances ---------------------------------------------------------------------------------------------
def check_capped_grids(name, waves, monkeypatch):
    _, contig, region, cfg, _ = TABLES[name]
    recs, exp = table(name), want(name)
    assert len(exp[0]) > recs.n // 2
    for grid in grids(recs.n):
        set_form(monkeypatch, "wave", grid, waves)
        assert_same(dev_tuple(recs, contig, region, cfg), exp, f"table {name}, SNF_EXTRACT_GRID={grid}, SNF_EXTRACT_WAVES={waves}")


def check_thread_form(name, monkeypatch):
    _, contig, region, cfg, _ = TABLES[name]
    set_form(monkeypatch, "thread")
    assert_same(dev_tuple(table(name), contig, region, cfg), want(name), f"table {name}, thread form")


def test_the_tables_hold_what_they_are_named_for():
    """The builders' own arithmetic: the sizes the cases are about are the sizes the records have."""
    import struct
    recs = table("cigar")
    n_cig = [struct.unpack_from("<H", recs.blob, int(o) + 16)[0] for o in recs.rec_off[:-1]]
    for k in range(1, 6):
        assert set(sc.around(k * T["step"])) <= set(n_cig)
    l_name = sorted({int(recs.blob[int(o) + 12]) for o in recs.rec_off[:-1]})
    assert set(range(2, 18)) <= set(l_name)
    recs = table("tags")
    aux = []
    for o, e in zip(recs.rec_off[:-1], recs.rec_off[1:]):
        o, e = int(o), int(e)
        ln, nc, ls = int(recs.blob[o + 12]), struct.unpack_from("<H", recs.blob, o + 16)[0], struct.unpack_from("<i", recs.blob, o + 20)[0]
        aux.append(e - (o + 36 + ln + 4 * nc + (ls + 1) // 2 + ls))
    for total in sc.around(T["xauxcap"]):
        assert aux.count(total) == 6, (total, aux)
    assert max(aux) > 2000
    recs = table("sa")
    blob = recs.blob.tobytes()
    sa_lens = [blob.index(b"\0", blob.index(b"SAZ", int(o)) + 3) - blob.index(b"SAZ", int(o)) - 3 for o in recs.rec_off[:-1]]
    assert set(sc.around(T["sa_chunk"], 2 * T["sa_chunk"], T["xauxcap"])) | {T["xauxcap"] - 2} <= set(sa_lens)
    assert blob.index(b"\0", blob.rindex(b"SAZ")) == len(blob) - 1      # the SA string ends the blob ...
    assert T["blob_pad"] >= 2 * T["comma_word"]      # ... and the two aligned words x_ld8 reads around its last bytes stay inside the padding


@pytest.mark.parametrize("waves", WAVES)
@pytest.mark.parametrize("name", sorted(TABLES))
def test_capped_grids_and_instances_emu(name, waves, emu_lib, monkeypatch):
    check_capped_grids(name, waves, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("waves", WAVES)
@pytest.mark.parametrize("name", sorted(TABLES))
def test_capped_grids_and_instances_gpu(name, waves, monkeypatch):
    check_capped_grids(name, waves, monkeypatch)


@pytest.mark.parametrize("name", sorted(TABLES))
def test_thread_form_emu(name, emu_lib, monkeypatch):
    check_thread_form(name, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(TABLES))
def test_thread_form_gpu(name, monkeypatch):
    check_thread_form(name, monkeypatch)


# ---- XMAXSEG: the segment table -----------------------------------------------------------------------------------------------
FORMS = (("wave", None), ("wave", 1), ("thread", None))


def check_segment_table(monkeypatch):
    from sniffles_amd import lib
    full, over = T["xmaxseg"] - 1, T["xmaxseg"]
    recs = xe.segment_table_records(full)                      # with the primary alignment: exactly the table
    exp = oracle_tuple(recs, "c1", WHOLE, MANY, args=("--max-splits-base", "100"))
    assert sum(1 for r in exp[0] if r[10] in ("SPLIT_PRIM", "SPLIT_SUP")) > 20
    for form, grid in FORMS:
        set_form(monkeypatch, form, grid)
        assert_same(dev_tuple(recs, "c1", WHOLE, MANY), exp, f"{full} SA elements, {form} form, grid {grid}")
    recs = xe.segment_table_records(over)                      # one more: the reference takes it, the device table does not
    oracle_tuple(recs, "c1", WHOLE, MANY, args=("--max-splits-base", "100"))
    texts = set()
    for form, grid in FORMS:
        set_form(monkeypatch, form, grid)
        with pytest.raises(lib.SnifflesAmdError, match="more split alignments") as e:
            dev_tuple(recs, "c1", WHOLE, MANY)
        texts.add(str(e.value))
    assert len(texts) == 1 and "alignment record 1:" in texts.pop()
    for n in (over, over + 1, over + 6):                       # under the default limits the read's splits are dropped, silently
        recs = xe.segment_table_records(n)
        exp = oracle_tuple(recs, "c1", WHOLE, {}, args=())
        assert not any(r[10] in ("SPLIT_PRIM", "SPLIT_SUP") for r in exp[0])
        for form, grid in FORMS:
            set_form(monkeypatch, form, grid)
            assert_same(dev_tuple(recs, "c1", WHOLE, {}), exp, f"{n} SA elements under the default limits, {form} form, grid {grid}")
    recs = xe.segment_table_records(over, flag=0x800)          # a supplementary record: the break-end lead only
    exp = oracle_tuple(recs, "c1", WHOLE, MANY, args=("--max-splits-base", "100"))
    assert [r[10] for r in exp[0] if r[0] == READ_ID_OFFSET + 2 and r[10] != "INLINE"] == ["BND_SA"]
    for form, grid in FORMS:
        set_form(monkeypatch, form, grid)
        assert_same(dev_tuple(recs, "c1", WHOLE, MANY), exp, f"{over} SA elements on a supplementary record, {form} form, grid {grid}")


def test_segment_table_emu(emu_lib, monkeypatch):
    check_segment_table(monkeypatch)


@pytest.mark.gpu
def test_segment_table_gpu(monkeypatch):
    check_segment_table(monkeypatch)


# ---- x_nmsum ------------------------------------------------------------------------------------------------------------------
NM_SIZES = sc.around(T["nm_fold"], T["nm_chunk"], 2 * T["nm_chunk"]) + [3 * T["nm_chunk"] + 28]
NM_CASES = [(n, p) for n in NM_SIZES for p in ("all", "third")] + \
           [(n, "gap") for n in NM_SIZES if n >= 2 * T["nm_chunk"] - 1] + [(n, "zeros") for n in (T["nm_fold"] + 1, T["nm_chunk"] + 1, NM_SIZES[-1])]


def check_nm_sum(n, pattern, monkeypatch):
    """average_regional_nm: the NM ratios of the reads added in BAM order, bit for bit."""
    recs, ratios = xe.nm_records(n, pattern)
    exp = oracle_tuple(recs, "c1", WHOLE, {}, 0, args=())
    assert float(xe.ordered_mean(ratios)).hex() == exp[2] and len(exp[1]) == n
    assert float(xe.ordered_mean(ratios[::-1])).hex() != exp[2]      # a sum in another order would not pass: added backwards, other bits
    for form in ("wave", "thread"):
        set_form(monkeypatch, form)
        got = dev_tuple(recs, "c1", WHOLE, {}, 0)
        assert got[2] == exp[2], f"{n} records, NM on {pattern}, {form} form: {got[2]} != {exp[2]}"
        assert got[1] == exp[1] and got[0] == exp[0] == [] and got[3] == exp[3] == n


@pytest.mark.parametrize("n,pattern", NM_CASES)
def test_nm_sum_emu(n, pattern, emu_lib, monkeypatch):
    check_nm_sum(n, pattern, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("n,pattern", NM_CASES)
def test_nm_sum_gpu(n, pattern, monkeypatch):
    check_nm_sum(n, pattern, monkeypatch)


# ---- the blocks of the thread form ----------------------------------------------------------------------------------------------
def check_thread_blocks(n, monkeypatch):
    recs = xe.block_records(n)
    exp = oracle_tuple(recs, "c1", WHOLE, {}, args=())
    assert len(exp[0]) == len(exp[1]) == n
    set_form(monkeypatch, "thread")
    assert_same(dev_tuple(recs, "c1", WHOLE, {}), exp, f"{n} records, thread form")


@pytest.mark.parametrize("n", sc.around(T["thread_block"], 2 * T["thread_block"]))
def test_thread_blocks_emu(n, emu_lib, monkeypatch):
    check_thread_blocks(n, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("n", sc.around(T["thread_block"], 2 * T["thread_block"]))
def test_thread_blocks_gpu(n, monkeypatch):
    check_thread_blocks(n, monkeypatch)


# ---- the first error in BAM order ---------------------------------------------------------------------------------------------
ERROR_TEXT = dict(hp_then_nmz="HP tag outside", sa_then_hp="6 fields", aux_then_sa="malformed auxiliary")


def check_first_error(pairing, monkeypatch):
    import extract_oracle as eo
    from sniffles_amd import lib
    recs, first = xe.error_records(pairing)
    import make_ref
    with pytest.raises((eo.ExtractError, ValueError)):
        oracle_tuple(recs, "c1", WHOLE, {})
    if make_ref.ref_root():                      # the unmodified reference fails on the table too
        import ref_harness as rh
        assert "error" in rh.run_reference_extract(recs, "c1", WHOLE[0], WHOLE[1], (), READ_ID_OFFSET, {})
    texts = set()
    for form, grid, waves in (("wave", None, None), ("wave", 1, None), ("wave", 2, 8), ("wave", recs.n - 1, 5), ("thread", None, None)):
        set_form(monkeypatch, form, grid, waves)
        with pytest.raises(lib.SnifflesAmdError, match=ERROR_TEXT[pairing]) as e:
            dev_tuple(recs, "c1", WHOLE, {})
        texts.add(str(e.value))
    assert len(texts) == 1, texts
    assert texts.pop().startswith(f"alignment record {first}: ")


@pytest.mark.parametrize("pairing", sorted(ERROR_TEXT))
def test_first_error_in_bam_order_emu(pairing, emu_lib, monkeypatch):
    check_first_error(pairing, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("pairing", sorted(ERROR_TEXT))
def test_first_error_in_bam_order_gpu(pairing, monkeypatch):
    check_first_error(pairing, monkeypatch)


# ---- one handle, several tables -------------------------------------------------------------------------------------------------
def check_handle_reuse(monkeypatch):
    """The handle keeps its device blocks from run to run (they only grow) and the temporary storage of its scans per record count:
    a large table, a small one, one that fails, the large one again, a second run without an upload."""
    from sniffles_amd import extract, lib
    set_form(monkeypatch, "wave")
    cfg = DevCfg(**MANY)

    def result(x):
        ti, info = x.result()
        reads = list(zip(ti.read_start.tolist(), ti.read_end.tolist(), ti.read_hp.tolist()))
        assert np.all(np.diff(ti.leads["read_id"].astype(np.int64)) >= 0), "leads out of record order"
        assert info.read_count == len(reads)
        return xu.canon_leads(ti), reads, float(ti.qc_nm_threshold).hex(), info.read_id

    small = xe.segment_table_records(2)
    exp_small = oracle_tuple(small, "c1", WHOLE, MANY, args=("--max-splits-base", "100"))
    bad, first = xe.error_records("hp_then_nmz")
    x = extract.Extractor(cfg)
    try:
        with pytest.raises(lib.SnifflesAmdError, match="before snf_extract_upload"):
            x.run()
        for step, (recs, exp) in enumerate(((table("sa"), want("sa")), (small, exp_small), (bad, None), (table("sa"), want("sa")),
                                            (table("mixed"), want("mixed")), (small, exp_small))):
            x.upload(recs, "c1", WHOLE[0], WHOLE[1], READ_ID_OFFSET)
            if exp is None:
                with pytest.raises(lib.SnifflesAmdError, match=f"alignment record {first}: HP tag outside"):
                    x.run()
                with pytest.raises(lib.SnifflesAmdError, match="before a successful"):
                    x.result()
                continue
            x.run()
            assert_same(result(x), exp, f"upload {step} on one handle")
            assert_same(dev_tuple(recs, "c1", WHOLE, MANY), exp, f"upload {step} on a fresh handle")
            x.run()      # again, without an upload
            assert_same(result(x), exp, f"second run after upload {step}")
    finally:
        x.close()


def test_handle_reuse_emu(emu_lib, monkeypatch):
    check_handle_reuse(monkeypatch)


@pytest.mark.gpu
def test_handle_reuse_gpu(monkeypatch):
    check_handle_reuse(monkeypatch)
