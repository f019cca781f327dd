"""Force calling without `SVCall` objects: `GenotypeTask.execute_records` (match, coverage and genotype of the targets on the device,
against the task's candidates where they lie in HBM), `VCF.read_target_table`, `VCF.rewrite_genotype_records` and
`pipeline.genotype_vcf(objects=False)` - against what the UNMODIFIED reference recorded (tests/golden/genotype_targets.json.gz,
genotype_vcf.json.gz) and against the object path, on the host tier and on the GPU."""
import functools
import gzip
import io

import numpy as np
import pytest

import cases
import genotype_util as gutil
import golden_util as gu
from sniffles_amd import abi, bam, bgzfout, parallel, pipeline, sv, vcf
from sniffles_amd.config import SnifflesConfig

TIERS = ["host", pytest.param("gpu", marks=pytest.mark.gpu)]


@pytest.fixture(params=TIERS)
def tier(request):
    if request.param == "host":
        import emu.emu as E
        E.lib()                                          # the host tier becomes the library of this test
    return request.param


# ---------------------------------------------------------------------------------------------- execute_records against the reference
def table_of(specs, cov=None):
    """The column table `execute_records` takes, from the target specs of tests/genotype_util.py."""
    names = []
    mate = []
    for t in specs:
        if t["bnd"] is None:
            mate.append(-1)
        else:
            if t["bnd"][0] not in names:
                names.append(t["bnd"][0])
            mate.append(names.index(t["bnd"][0]))
    return dict(svtype=np.asarray([sv.TYPES.index(t["svtype"]) if t["svtype"] in sv.TYPES else -1 for t in specs], np.int32),
                pos=np.asarray([t["pos"] for t in specs], np.int64), svlen=np.asarray([t["svlen"] for t in specs], np.int64),
                mate_contig=np.asarray(mate, np.int32), mate_names=names,
                bnd_is_first=np.asarray([1 if (t["bnd"] is not None and t["bnd"][2]) else 0 for t in specs], np.uint8),
                cov=np.asarray([t["cov"] for t in specs] if cov is None else cov, np.int32).reshape(len(specs), 5))


def task_of(name):
    build, kw, _ = cases.ALL[name]
    ti = build()
    cfg = gu.make_config(kw, ti)
    task = parallel.GenotypeTask(id=ti.task_id, sv_id=ti.sv_id_start, contig=ti.contig, start=0, end=ti.contig_len, config=cfg)
    task.tandem_repeats = None if ti.tr_start is None else list(zip(ti.tr_start.tolist(), ti.tr_end.tolist()))
    task.lead_provider = pipeline._Extracted(ti)
    return ti, cfg, task


# (the largest case runs on the GPU only, like in tests/test_genotype.py)
RECORDED = [("host", n) for n in gutil.CASES + ["bnd_first"] if n != "chr20_30x_ont"] + \
           [pytest.param("gpu", n, marks=pytest.mark.gpu) for n in gutil.CASES + ["bnd_first"]]


@pytest.mark.parametrize("which,name", RECORDED)
def test_execute_records_matches_the_recorded_reference(which, name):
    """Per target: match id, dist, the five coverage values (pre-set ones that stay included) and the reference-allele genotype as the
    unmodified reference's GenotypeTask.execute left them; the genotype that is printed is the match's where it has one."""
    if which == "host":
        import emu.emu as E
        E.lib()                                          # the host tier becomes the library of this test
    doc = gu.load("genotype_targets")[name]
    case = doc.get("case", name)
    ti, cfg, task = task_of(case)
    assert gu.input_sha(ti) == doc["input_sha"]
    table = table_of(doc["specs"])
    exp = doc["expected"]
    try:
        if "error" in exp:
            with pytest.raises(UnboundLocalError):
                task.execute_records(table)
            return
        for form in (0, 1):
            got = task.execute_records(table, form=form)
            golden = gu.load(case)["expected"]
            cand, final = golden["candidates"], golden["final"]
            assert got["n_candidates"] == len(cand) and len(got["best"]) == len(exp["targets"])
            tuples = task.genotype_tuples(got)
            n_match_gt = 0
            for i, w in enumerate(exp["targets"]):
                b = int(got["best"][i])
                assert (None if b < 0 else cand[b]["id"]) == w["match"], (i, w)
                assert (None if b < 0 else float(got["dist"][i])) == w["dist"], (i, w)
                assert got["cov"][i].tolist() == w["cov"], (i, w)
                depth = int(got["depth"][i])
                ref_allele = [0, 0, 0, depth, 0, [None, None]] if depth > 0 else [list(x) if isinstance(x, tuple) else x for x in cfg.genotype_none]
                assert ref_allele == w["gt"], (i, w)
                printed = [list(x) if isinstance(x, tuple) else x for x in tuples[i]]
                if b >= 0 and final[b]["gt"] is not None:
                    assert final[b]["id"] == cand[b]["id"] and printed == final[b]["gt"] and got["gt"][i][7] == abi.GTSRC_MATCH
                    n_match_gt += 1
                else:
                    assert printed == w["gt"]
            if any(w["match"] for w in exp["targets"]):
                assert n_match_gt > 0
    finally:
        task.close()


def test_a_target_without_any_sample_yields_none(tier):
    """A target beyond the coverage vector whose coverage fields are unset has no sample: `execute` returns None for the whole task
    (parallel.py:362-363), and so does `execute_records`; with one field set it has a depth."""
    doc = gu.load("genotype_targets")["long_ins"]
    ti, cfg, task = task_of("long_ins")
    specs = doc["specs"][:3] + [dict(id="far", svtype="DEL", pos=3 * ti.contig_len, svlen=-100, bnd=None, cov=[0] * 5)]
    cov = [t["cov"] for t in specs]
    cov[-1] = [abi.NONE_I32] * 5
    try:
        assert task.execute_records(table_of(specs, cov)) is None
        cov[-1] = [abi.NONE_I32, abi.NONE_I32, 9, abi.NONE_I32, abi.NONE_I32]
        got = task.execute_records(table_of(specs, cov))
        assert got["cov"][-1].tolist() == cov[-1] and int(got["depth"][-1]) == 9 and task.genotype_tuples(got)[-1] == (0, 0, 0, 9, 0, (None, None))
        cov[-1] = [abi.NONE_I32, 2, 3, abi.NONE_I32, 0]            # round(2.5) = 2: halves go to the even neighbour
        got = task.execute_records(table_of(specs, cov))
        assert int(got["depth"][-1]) == 2
        cov[-1] = [0, 0, 0, 1, 0]                                  # round(1 / 3) = 0: genotype_none
        got = task.execute_records(table_of(specs, cov))
        assert int(got["depth"][-1]) == 0 and task.genotype_tuples(got)[-1] == cfg.genotype_none
    finally:
        task.close()


# ---------------------------------------------------------------------------------------------- the driver against the reference's text
@pytest.mark.parametrize("name", ["sample_splits_14x", "sample_two_contigs_12x"])
def test_genotype_vcf_records_writes_the_reference_text(tier, name):
    from test_pipeline import config_for, records_sha
    doc = gu.load("genotype_vcf")[name]
    recs = cases.SAMPLES[name][0]()
    assert records_sha(recs) == doc["input_sha"]
    buf = io.StringIO()
    n = pipeline.genotype_vcf(recs, config_for(()), io.StringIO(doc["vcf_in"]), buf, objects=False)
    assert buf.getvalue() == doc["vcf_out"]
    assert n == sum(1 for ln in doc["vcf_out"].split("\n") if ln and not ln.startswith("#")) > 50


# ---------------------------------------------------------------------------------------------- objects=False against objects=True
@functools.lru_cache(None)
def small_sample():
    """Three contigs of 60 - 80 kb as a BAM stream (raw, BGZF) and as a record table."""
    import bam_index_cases as K
    from sniffles_amd import synth_bam
    names, lens, recs = synth_bam.gen_sample(21, ref_names=("chr20", "chr21", "chr22"), ref_lens=(80_000, 70_000, 60_000), cov=8.0,
                                             read_len_mean=6000, site_spacing=9000)[:3]
    raw, _, _ = K.stream_of(recs, names, lens)
    return bam.bgzf_deflate(raw)


def small_config(**kw):
    import vcf_util as vu
    cfg = SnifflesConfig(all_contigs=True, **kw)
    for k, v in vu.FIXED.items():
        setattr(cfg, k, v)
    return cfg


_targets = {}


def small_targets(tier, path):
    """The sample's own calls, and a copy of them shifted by 180 bp so that near misses exist."""
    if tier not in _targets:
        buf = io.StringIO()
        pipeline.call_sample(bam.read_bam(path), small_config(), vcf_handle=buf)
        lines = buf.getvalue().split("\n")
        body = [ln for ln in lines if ln and not ln.startswith("#")]
        moved = []
        for ln in body:
            c = ln.split("\t")
            c[1] = str(int(c[1]) + 180)
            moved.append("\t".join(c))
        assert len(body) > 10
        order = {c: k for k, c in enumerate(dict.fromkeys(ln.split("\t")[0] for ln in body))}
        both = sorted(body + moved, key=lambda ln: (order[ln.split("\t")[0]], int(ln.split("\t")[1])))      # (a tabix index needs sorted records)
        _targets[tier] = "\n".join([ln for ln in lines if ln.startswith("#")] + both) + "\n"
    return _targets[tier]


class FastaWithN:
    """A reference with runs of 'N' (pysam's `fetch`)."""

    def __init__(self, names, lens):
        rng = np.random.default_rng(5)
        self.seq = {}
        for name, n in zip(names, lens):
            a = rng.choice(np.frombuffer(b"ACGT", np.uint8), int(n))
            for s in range(3000, int(n) - 4000, 9000):
                a[s:s + 2500] = ord("N")
            self.seq[name] = a.tobytes().decode("ascii")

    def fetch(self, contig, start=None, end=None):
        return self.seq[contig][start:end]


VARIANTS = ["plain", "phase", "mosaic", "regions", "reference_with_N", "read_bam_device", "open_indexed", "vcf_gz"]


@pytest.mark.parametrize("variant", VARIANTS)
def test_records_path_writes_what_the_object_path_writes(tier, tmp_path, variant):
    path = str(tmp_path / "sample.bam")
    with open(path, "wb") as f:
        f.write(small_sample())
    vcf_in = small_targets(tier, path)
    out = {}
    for objects in (True, False):
        cfg = small_config(**({"phase": True} if variant == "phase" else {"mosaic": True} if variant == "mosaic" else {}))
        if variant == "regions":
            cfg.regions_by_contig = {"chr20": [("chr20", 10000, 30000), ("chr20", 25000, 70000)], "chr22": [("chr22", 5000, 40000)]}
        if variant == "read_bam_device":
            recs = bam.read_bam_device(path)
        elif variant == "open_indexed":
            recs = bam.open_indexed(path, index=bam.index_bam(path))
        else:
            recs = bam.read_bam(path)
        reference = FastaWithN(recs.ref_names, recs.ref_lens) if variant == "reference_with_N" else None
        try:
            if variant == "vcf_gz":
                gz = str(tmp_path / f"out_{objects}.vcf.gz")
                with bgzfout.VcfGzWriter(gz) as w:
                    n = pipeline.genotype_vcf(recs, cfg, io.StringIO(vcf_in), w, objects=objects, reference=reference)
                with gzip.open(gz, "rt", newline="") as f:
                    text = f.read()
            else:
                buf = io.StringIO()
                n = pipeline.genotype_vcf(recs, cfg, io.StringIO(vcf_in), buf, objects=objects, reference=reference)
                text = buf.getvalue()
        finally:
            if hasattr(recs, "close"):
                recs.close()
        out[objects] = (n, text)
    assert out[True] == out[False]
    n, text = out[True]
    body = [ln for ln in text.split("\n") if ln and not ln.startswith("#")]
    assert n == len(body) > 10
    gts = {ln.split("\t")[9].split(":")[0] for ln in body}
    assert len(gts) >= 2, gts                                    # matched genotypes and reference-allele ones both occur
    if variant == "plain":
        _targets[(tier, "plain_out")] = text
    elif variant in ("read_bam_device", "open_indexed", "vcf_gz") and (tier, "plain_out") in _targets:
        assert text == _targets[(tier, "plain_out")]
    elif variant in ("regions", "reference_with_N") and (tier, "plain_out") in _targets:
        assert text != _targets[(tier, "plain_out")]              # (the option matters on this sample)


# ---------------------------------------------------------------------------------------------- parsing
def fields_of_call(c):
    b = getattr(c, "bnd_info", None)
    return (c.contig, c.raw_vcf_line_index, c.svtype, c.pos, c.svlen, c.end,
            None if b is None else (b.mate_contig, b.mate_ref_start, bool(b.is_first), bool(b.is_reverse)),
            (c.coverage_upstream, c.coverage_start, c.coverage_center, c.coverage_end, c.coverage_downstream), c.raw_vcf_line)


def fields_of_table(tables):
    out = []
    for contig, t in tables.items():
        for i in range(len(t["lines"])):
            m = int(t["mate_contig"][i])
            bnd = None if m < 0 else (t["mate_names"][m], int(t["mate_ref_start"][i]), bool(t["bnd_is_first"][i]), bool(t["bnd_is_reverse"][i]))
            assert (t["svtype"][i] >= 0) == (t["svtype_names"][i] in sv.TYPES) and (t["svtype"][i] < 0 or sv.TYPES[t["svtype"][i]] == t["svtype_names"][i])
            out.append((contig, int(t["line_index"][i]), t["svtype_names"][i], int(t["pos"][i]), int(t["svlen"][i]), int(t["end"][i]), bnd,
                        tuple(t["cov"][i].tolist()), t["lines"][i]))
    return out


@pytest.mark.parametrize("name", ["sample_splits_14x", "sample_two_contigs_12x"])
@pytest.mark.parametrize("as_bytes", [False, True])
def test_read_target_table_agrees_with_read_svs_iter(name, as_bytes):
    text = gu.load("genotype_vcf")[name]["vcf_in"]
    handle = (lambda: io.BytesIO(text.encode())) if as_bytes else (lambda: io.StringIO(text))
    cfg = SnifflesConfig()
    a, b = vcf.VCF(cfg, handle()), vcf.VCF(cfg, handle())
    calls = [fields_of_call(c) for c in a.read_svs_iter()]
    rows = fields_of_table(b.read_target_table())
    assert a.header_str == b.header_str and len(calls) > 50
    assert sorted(calls, key=lambda r: r[1]) == sorted(rows, key=lambda r: r[1])
    by_contig = {}
    for r in calls:
        by_contig.setdefault(r[0], []).append(r)
    assert [r for rs in by_contig.values() for r in rs] == rows      # contigs in order of first appearance, input order inside
    assert {r[2] for r in rows} >= {"INS", "DEL"}


GOOD = "chr1\t100\tid\tN\t<DEL>\t60\tPASS\tSVTYPE=DEL;SVLEN=-50;END=150\tGT\t0/1"
MALFORMED = {
    "empty_line": "",
    "seven_columns": "chr1\t100\tid\tN\t<DEL>\t60\tPASS",
    "pos_not_an_integer": GOOD.replace("\t100\t", "\t1e2\t"),
    "qual_not_an_integer": GOOD.replace("\t60\t", "\t60.5\t"),
    "svlen_not_an_integer": GOOD.replace("SVLEN=-50", "SVLEN=fifty"),
    "end_not_an_integer": GOOD.replace("END=150", "END=1.5e2"),
    "bnd_alt_without_a_mate": "chr1\t100\tid\tN\tN.\t60\tPASS\tSVTYPE=BND\tGT\t0/1",
    "tra_without_a_mate": "chr1\t100\tid\tN\t<TRA>\t60\tPASS\tSVTYPE=TRA\tGT\t0/1",
    "bnd_mate_without_a_position": "chr1\t100\tid\tN\tN[chr2[\t60\tPASS\tSVTYPE=BND\tGT\t0/1",
    "info_with_two_equal_signs": GOOD.replace("SVLEN=-50", "SVLEN=-50=3"),
}


@pytest.mark.parametrize("name", sorted(MALFORMED))
def test_malformed_lines_raise_what_read_svs_iter_raises(name):
    text = "##fileformat=VCFv4.2\n#CHROM\tPOS\n" + GOOD + "\n" + MALFORMED[name] + "\n" + GOOD + "\n"
    cfg = SnifflesConfig()
    with pytest.raises(ValueError) as want:
        list(vcf.VCF(cfg, io.StringIO(text)).read_svs_iter())
    with pytest.raises(ValueError) as got:
        vcf.VCF(cfg, io.StringIO(text)).read_target_table()
    assert str(got.value) == str(want.value) and "Line 4:" in str(want.value)
    assert type(got.value.__cause__) is type(want.value.__cause__)


def test_tra_is_read_as_bnd_and_lines_are_rewritten_from_the_table():
    text = "##fileformat=VCFv4.2\n#CHROM\tPOS\n" + GOOD + "\nchr1\t300\tt\tN\tN]chr9:77]\t.\tPASS\tSVTYPE=TRA\tGT:XX\t0/1:5\textra\n"
    cfg = SnifflesConfig()
    t = vcf.VCF(cfg, io.StringIO(text)).read_target_table()["chr1"]
    assert t["svtype"].tolist() == [sv.TYPES.index("DEL"), sv.TYPES.index("BND")] and t["mate_names"] == ["chr9"]
    assert (int(t["mate_ref_start"][1]), int(t["bnd_is_first"][1]), int(t["bnd_is_reverse"][1])) == (77, 1, 1)
    tuples = [(0, 1, 30, 5, 6, ("1", "7")), cfg.genotype_none]
    for phase in (False, True):
        cfg.phase = phase
        a, b = io.StringIO(), io.StringIO()
        calls = list(vcf.VCF(cfg, io.StringIO(text)).read_svs_iter())
        w = vcf.VCF(cfg, a)
        for c, gt in zip(calls, tuples):
            c.genotype_match_sv, c.genotypes = None, {0: gt}
            w.rewrite_genotype(c)
        assert vcf.VCF(cfg, b).rewrite_genotype_records(t["lines"], tuples) == 2
        assert a.getvalue() == b.getvalue() and a.getvalue().count("\n") == 2 and "extra" not in a.getvalue()
