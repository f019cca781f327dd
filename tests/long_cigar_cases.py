"""Record tables for CIGARs that live in a CG:B,I tag (SAM/BAM spec 4.2.2: more than 65 535 operations do not fit the 16-bit count;
the record then carries `kSmN` inline, k = l_seq, m = the reference span, and the operations in the tag).  Tests: tests/test_long_cigar.py.

A table is a list of `Spec`s.  `real(specs)` writes every record as its spec says (inline or CG form, the tag at a chosen place);
`twin(specs)` writes the same alignments inline and without the tag - that is the table the oracle (oracle/extract_oracle.py, which
reads inline CIGARs only) is asked about.  A CIGAR of more than 65 535 operations has no inline form: its twin has the adjacent
M / = / X operations merged into one M, which leaves a few operations and the same events.  That the merge changes nothing for the
oracle is asserted by `pattern_checked` for every pattern at a size that still fits inline.  Bases come from one seeded generator per
table and a twin draws the same ones, so an inserted sequence read at a wrong offset shows."""
import functools
import struct

import numpy as np

import extract_edges as xe
import size_classes as sc
from extract_edges import D, EQ, H, I, M, N, S, X, el, elements, int_tag, sa_tag, z_tag

U16 = 65535                                  # the largest inline operation count
CONTIGS, CONTIG_LENS = xe.CONTIGS, xe.CONTIG_LENS
WHOLE = (0, 400000)
REF = (M, D, N, EQ, X)
QRY = (M, I, S, EQ, X)


def T():
    return sc.extract_thresholds()


def cg_tag(ops):
    from sniffles_amd import synth_bam
    return synth_bam.cg_tag(ops)


def merged(ops):
    """adjacent M / = / X operations as one M."""
    out = []
    for op, n in ops:
        if op in (M, EQ, X) and out and out[-1][0] == M:
            out[-1] = (M, out[-1][1] + n)
        else:
            out.append((M if op in (M, EQ, X) else op, n))
    return out


class Spec:
    """One alignment.  cg: None = what the writer does by itself (CG form above 65 535 operations), True = forced, False = inline;
    cg_at: the tag's place among `tags` (a list of whole tags; None = last); inline: for records that only look the part - the
    inline operations as they are written (the sequence keeps the length `qlen`), tags as they stand, the same in both tables."""

    def __init__(self, pos, ops, tags=(), cg=None, cg_at=None, flag=0, mapq=60, ref_id=0, name=None, seq=True, inline=None, qlen=None):
        self.pos, self.ops, self.tags, self.cg, self.cg_at = int(pos), [(int(a), int(b)) for a, b in ops], list(tags), cg, cg_at
        self.flag, self.mapq, self.ref_id, self.name, self.seq, self.inline, self.qlen = flag, mapq, ref_id, name, seq, inline, qlen


def _write(specs, seed, as_twin):
    from sniffles_amd import bam, synth_bam
    rng = np.random.default_rng(seed)
    out = []
    for k, s in enumerate(specs):
        qlen = s.qlen if s.qlen is not None else sum(n for op, n in s.ops if op in QRY)
        codes = rng.choice(np.array([1, 2, 4, 8], np.uint8), qlen if s.seq else 0)
        name = s.name or f"r{k:04d}"
        if s.inline is not None:
            rec = synth_bam.make_record(s.ref_id, s.pos, s.mapq, s.flag, name, s.inline, codes, b"".join(s.tags))
        elif as_twin:
            ops = s.ops if len(s.ops) <= U16 else merged(s.ops)
            rec = synth_bam.make_record(s.ref_id, s.pos, s.mapq, s.flag, name, ops, codes, b"".join(s.tags), cg=False)
        else:
            rec = synth_bam.make_record(s.ref_id, s.pos, s.mapq, s.flag, name, s.ops, codes, s.tags, cg=s.cg, cg_at=s.cg_at)
        out.append(rec)
    return bam.records_from_list(CONTIGS, CONTIG_LENS, out)


def real(specs, seed=701):
    return _write(specs, seed, False)


def twin(specs, seed=701):
    return _write(specs, seed, True)


def to_cg(rec: bytes) -> bytes:
    """An inline record rewritten in CG form (what a writer does above 65 535 operations, here at any count): the tag goes last."""
    bs, ref, pos, l_name, mapq, bn, n_cig, flag, l_seq = struct.unpack_from("<iiiBBHHHi", rec, 0)
    a = 36 + l_name
    ops = [(c & 15, c >> 4) for c in struct.unpack_from(f"<{n_cig}I", rec, a)]
    span = sum(n for op, n in ops if op in REF)
    inline = [(l_seq << 4) | S, (span << 4) | N][:max(1, min(2, n_cig))]      # (a tag of one operation takes part under an inline count of one only)
    body = rec[4:16] + struct.pack("<HH", len(inline), flag) + rec[20:a] + struct.pack(f"<{len(inline)}I", *inline) + rec[a + 4 * n_cig:] + cg_tag(ops)
    return struct.pack("<i", len(body)) + body


def table_to_cg(recs):
    from sniffles_amd import bam
    raw = [recs.blob[int(a):int(b)].tobytes() for a, b in zip(recs.rec_off[:-1], recs.rec_off[1:])]
    return bam.records_from_list(recs.ref_names, recs.ref_lens, [to_cg(r) for r in raw])


def inline_counts(recs):
    return [struct.unpack_from("<H", recs.blob, int(o) + 16)[0] for o in recs.rec_off[:-1]]


# ------------------------------------------------------------------------------------------------------------ long CIGARs
def long_ops(n, events=(), lead_clip=0, tail_clip=0):
    """n operations: `=` and X by turns (3 and 1 bases; a twin merges them), the lead-bearing operations of `events` ({index: (op, len)})
    among them, a soft clip as the first / last operation where asked for."""
    ops = [((EQ, 3) if k % 2 == 0 else (X, 1)) for k in range(n)]
    if lead_clip:
        ops[0] = (S, lead_clip)
    if tail_clip:
        ops[n - 1] = (S, tail_clip)
    for k, ev in dict(events).items():
        assert (1 if lead_clip else 0) <= k < n - (1 if tail_clip else 0), (k, n)
        ops[k] = ev
    return ops


def edge_events(n, t):
    """lead-bearing operations on the first operation behind the leading clip, on 65 534 / 65 535 / 65 536, on the last lane's last
    operation of the step that holds 65 536, and (a clip of lead size) on the last operation - as far as n operations reach."""
    step = t["step"]
    at = [1, U16 - 1, U16, U16 + 1, (U16 + 1) // step * step + step - 1]
    ev = {}
    for j, k in enumerate(at):
        if k < n - 1:
            ev[k] = (I, 50 + j) if j % 2 == 0 else (D, 60 + j)
    return ev


@functools.lru_cache(maxsize=None)
def pattern_checked():
    """The twin rule, on the oracle: every pattern the long tables use, at 3 000 operations (events moved to where that size has them),
    gives the same leads, reads and qc_nm_threshold inline as with its matches merged."""
    import extract_oracle as eo
    n = 3000
    specs = [Spec(60000, long_ops(n, {1: (I, 50), n - 3: (D, 61), n - 2: (I, 52)}, lead_clip=50, tail_clip=60), [int_tag("NM", "S", 900)]),
             Spec(70000, long_ops(n, {n - 500: (I, 77)}), [int_tag("NM", "S", 800)]),
             Spec(80000, long_ops(n, {7: (D, 300), 1500: (I, 120)}), [int_tag("NM", "S", 1200), int_tag("HP", "C", 1), int_tag("PS", "i", 5)])]
    a = real(specs)
    b = _write([Spec(s.pos, merged(s.ops), s.tags) for s in specs], 701, False)
    assert max(inline_counts(a)) == n and max(inline_counts(b)) < 12
    outs = [eo.extract_region(r.blob, r.rec_off, r.ref_names, "c1", WHOLE[0], WHOLE[1], eo.Cfg(), 17) for r in (a, b)]
    for key in ("rows", "reads", "qc_nm_threshold", "read_id"):
        assert outs[0][key] == outs[1][key], key
    assert len(outs[0]["rows"]) >= 8
    return True


def edge_specs():
    """The 16-bit edge: 65 534 and 65 535 operations inline and as CG, then the counts that only the tag can hold - one more, two more,
    and one short of / on / one past a whole step more; a record whose only lead-bearing operation lies above 65 536 (the emit pass
    restarts at a step above 16 bits)."""
    t = T()
    assert pattern_checked()
    step = t["step"]
    specs = []
    pos = iter(range(20000, 60000, 1500))
    for n, cg in ((U16 - 1, False), (U16 - 1, True), (U16, False), (U16, True), (U16 + 1, None), (U16 + 2, None),
                  (U16 + step, None), (U16 + 1 + step, None), (U16 + 2 + step, None)):
        specs.append(Spec(next(pos), long_ops(n, edge_events(n, t), lead_clip=50, tail_clip=60), [int_tag("NM", "S", 40000)], cg=cg))
    n = U16 + 1 + 18 * step
    specs.append(Spec(next(pos), long_ops(n, {U16 + 1 + 17 * step + 5: (I, 71)}), [int_tag("NM", "S", 30000), int_tag("HP", "C", 2)]))
    return specs


def among_specs(n_inline=300):
    """one record of more than 65 535 operations in the middle of 300 inline ones."""
    assert pattern_checked()
    specs = [Spec(60000 + 40 * k, [(M, 1000 + k % 7), (I, 50 + k % 60), (M, 30), (D, 45 + k % 9), (M, 10)], [int_tag("NM", "C", k % 200)]) for k in range(n_inline)]
    n = U16 + 300
    specs.insert(n_inline // 2, Spec(60000 + 40 * (n_inline // 2), long_ops(n, {3: (I, 64), n - 2: (D, 90)}, tail_clip=70), [int_tag("NM", "S", 20000)]))
    return specs


# ------------------------------------------------------------------------------------------------------------ where the tag lies
OPS = [(S, 50), (EQ, 700), (X, 1), (EQ, 399), (I, 60), (EQ, 300), (D, 47), (M, 20), (S, 100)]
OPS_QLEN = sum(n for op, n in OPS if op in QRY)
assert OPS_QLEN == 1630
OTHER = [(M, 1000), (I, 99), (M, OPS_QLEN - 1099)]      # what a CG tag that must not be used says


def where_specs():
    t = T()
    cap = t["xauxcap"]
    junk = b"xbBs" + struct.pack("<i9h", 9, *range(9))
    sa = sa_tag(el(pos=90000, strand="-", clip0=10, span=200) + ";")
    five = [int_tag("NM", "C", 9), int_tag("HP", "C", 1), int_tag("PS", "i", 4242), sa, junk]
    specs = []
    pos = iter(range(60000, 240000, 300))
    for at in (0, 1, 2, 3, 4, None):                       # first, between, last
        specs.append(Spec(next(pos), OPS, five, cg=True, cg_at=at))
    for at in (0, None):                                    # read names of four consecutive lengths: the array on every residue modulo 4
        for r in range(4):                                  # (records lie byte by byte in the table: one of the four lengths gives r)
            p = next(pos)
            cands = [Spec(p, OPS, five, cg=True, cg_at=at, name="n" * (5 + k)) for k in range(4)]
            specs.append(next(c for c in cands if cg_offsets(real(specs + [c]))[-1] % 4 == r))
    small = cg_tag(OPS)
    nm = int_tag("NM", "S", 321)
    for total in sc.around(cap):                            # the LDS copy on one side, the blob walk on the other
        room = total - len(small) - len(nm)
        specs.append(Spec(next(pos), OPS, [xe.b_tag("xb", room), nm], cg=True, cg_at=1))
        specs.append(Spec(next(pos), OPS, [z_tag("xz", room - 4), nm], cg=True, cg_at=0))
        specs.append(Spec(next(pos), OPS, [nm, xe.b_tag("xb", room)], cg=True, cg_at=None))
    specs.append(Spec(next(pos), OPS, [nm, cg_tag(OTHER)], cg=True, cg_at=1))      # a second CG behind the first: the first decides
    specs.append(Spec(next(pos), OPS, [cg_tag(OTHER), nm], cg=True, cg_at=0))
    specs.append(Spec(next(pos), [(M, 1200), (S, 20), (M, 300), (I, 50), (M, 9)], [nm], cg=True))      # an S inside the alignment is no clip
    return specs


def aux_lengths(recs):
    out = []
    for o, e in zip(recs.rec_off[:-1], recs.rec_off[1:]):
        o, e = int(o), int(e)
        ln, nc, ls = int(recs.blob[o + 12]), struct.unpack_from("<H", recs.blob, o + 16)[0], struct.unpack_from("<i", recs.blob, o + 20)[0]
        out.append(e - (o + 36 + ln + 4 * nc + (ls + 1) // 2 + ls))
    return out


def cg_offsets(recs):
    """byte offset in the blob of the first value of every record's first CG:B,I array (-1: none)."""
    blob = recs.blob.tobytes()
    out = []
    for o, e in zip(recs.rec_off[:-1], recs.rec_off[1:]):
        k = blob.find(b"CGBI", int(o), int(e))
        out.append(k + 8 if k >= 0 else -1)
    return out


# ------------------------------------------------------------------------------------------------------------ records that only look the part
LOOK_CFG = dict(min_alignment_length=0)      # a record whose inline CIGAR is all clip has no aligned base: let it count as a read


def look_alike_specs():
    """Every record here keeps its inline CIGAR.  The tags say OTHER (an insertion of lead size): a kernel that took one of them
    would emit a lead the oracle, which never looks at CG, does not have."""
    L = OPS_QLEN
    ph = [(S, L), (N, 1500)]
    good = cg_tag(OTHER)
    nm = int_tag("NM", "C", 7)
    specs = []
    pos = iter(range(60000, 240000, 2000))

    def add(inline, tags, **kw):
        specs.append(Spec(next(pos), [], inline=inline, tags=[nm] + tags, qlen=L, **kw))
        specs.append(Spec(next(pos), OPS, [nm]))           # an ordinary record after each
    add(ph, [])                                                                          # S == l_seq, no CG
    add([(S, L - 1), (M, 1), (N, 1500)], [good])                                         # S of l_seq - 1
    add([(M, L), (N, 1500)], [good])                                                     # M first
    add(ph, [b"CGZ" + b"1000M99I481M\0"])                                                # CG:Z
    add(ph, [b"CGBC" + struct.pack("<i", 12) + cg_tag(OTHER)[8:]])                       # CG:B,C
    add(ph, [b"CGBi" + cg_tag(OTHER)[4:]])                                               # CG:B,i
    add(ph, [b"CGBI" + struct.pack("<i", 0)])                                            # count 0
    add(ph, [cg_tag([(M, L)])])                                                          # count 1 under n_cigar_op 2
    add(ph, [b"CGZ" + b"x\0", good])                                                     # the first tag named CG decides: not an array
    add(ph, [good], flag=0x4)                                                            # a placeholder on an unmapped record
    add(ph, [good], ref_id=1)                                                            # ... and on another contig
    return specs


# ------------------------------------------------------------------------------------------------------------ l_seq == 0, split reads
def noseq_specs():
    """no sequence stored: inline `0S mN`, and the query length comes from the operations in the tag."""
    nm = int_tag("NM", "S", 150)
    return [Spec(60000, [(M, 1200), (D, 60), (M, 300)], [nm], cg=True, seq=False),
            Spec(62000, [(S, 30), (EQ, 1500), (D, 50), (X, 100), (S, 45)], [nm], cg=True, seq=False),
            Spec(64000, [(H, 10), (M, 999), (D, 70), (M, 1)], [nm], cg=True, cg_at=0, seq=False),
            Spec(66000, [(EQ, 500), (X, 499)], [nm], cg=True, seq=False),       # one short of min_alignment_length
            Spec(68000, [(EQ, 500), (X, 500)], [nm], cg=True, seq=False)]


SPLIT_CFG = dict(max_splits_base=100)


def split_specs():
    """a primary and a supplementary record in CG form with an SA tag: the break side of Lead.for_bnd and the clip lengths come from
    the first and last operation of the array; and clips of several operations, hard ones outermost."""
    nm = int_tag("NM", "C", 7)
    specs = []
    pos = iter(range(60000, 240000, 3000))
    for ops in (xe.SA_OPS, xe.SA_OPS[::-1]):               # the longer clip on the left / on the right
        for flag, k0 in ((0, 1), (0x10, 2), (0x800, 3), (0x810, 4)):
            for at in (0, None):
                specs.append(Spec(next(pos), ops, [nm, sa_tag(";".join(elements(2, k0)) + ";")], cg=True, cg_at=at, flag=flag))
    specs.append(Spec(next(pos), [(M, 1200), (S, xe.SA_QLEN - 1200)], [nm, sa_tag(elements(1, 1)[0] + ";")], cg=True))
    specs.append(Spec(next(pos), [(H, 7), (S, 30), (S, 35), (M, 1100), (I, 60), (M, 300), (S, 40), (H, 9)], [nm], cg=True))
    specs.append(Spec(next(pos), [(H, 7), (S, 30), (S, 35), (M, 1100), (I, 60), (M, 300), (S, 50), (H, 9)],
                      [sa_tag(el(pos=70000, strand="-") + ";"), nm], cg=True, cg_at=1))
    return specs


# ------------------------------------------------------------------------------------------------------------ errors
ERRORS = dict(cigarop="CIGAR operation > 8", clip="invalid clipping", aux="malformed auxiliary")


def error_specs(kind, cg_first):
    """Twelve records, two of which fail the call: one in CG form (`kind`) and one inline (an HP tag outside 0..2).  cg_first: the CG
    record is the earlier one.  Returns (specs, index of the first failing record).  `aux`: the array's count says more operations than
    the record has bytes left - no inline form of that exists, so no twin either.
    `clip`: the issue asked for "an S in the middle of the array (XE_CLIP)".  That premise was wrong: pysam's clip properties, the
    oracle and the kernels take M S M without complaint (where_specs holds such an array as a record that must pass); what they
    refuse is a hard clip inside a soft one, S H M ..., and that is the shape used here."""
    t = T()
    body = [(M, 3), (I, 1)] * t["step"]
    ops = dict(cigarop=[(M, 1200)] + body + [(9, 5), (I, 60), (M, 100)],
               clip=[(S, 30), (H, 7), (M, 1200)] + body + [(I, 60), (M, 100)],      # a hard clip inside a soft one: pysam refuses the clip properties
               aux=[(M, 1200)] + body + [(I, 60), (M, 100)])[kind]
    early, late = (3, 9) if cg_first else (5, 1)
    specs = []
    for k in range(12):
        if k == early:
            specs.append(Spec(60000 + 500 * k, ops, [int_tag("NM", "C", 1)], cg=True))
        elif k == late:
            specs.append(Spec(60000 + 500 * k, [(M, 1200), (I, 60), (M, 100)], [b"HPC\x09"]))
        else:
            specs.append(Spec(60000 + 500 * k, [(M, 1200), (I, 60), (M, 100)], [int_tag("NM", "C", k)]))
    return specs, min(early, late)


def error_records(kind, cg_first):
    """(the table, its twin or None, index of the first failing record)"""
    from sniffles_amd import bam
    specs, first = error_specs(kind, cg_first)
    recs = real(specs)
    if kind != "aux":
        return recs, twin(specs), first
    raw = [bytearray(recs.blob[int(a):int(b)].tobytes()) for a, b in zip(recs.rec_off[:-1], recs.rec_off[1:])]
    k = 3 if cg_first else 5
    at = bytes(raw[k]).index(b"CGBI") + 4
    n = struct.unpack_from("<i", raw[k], at)[0]
    struct.pack_into("<i", raw[k], at, n + 1)               # one operation more than the record holds
    return bam.records_from_list(CONTIGS, CONTIG_LENS, [bytes(r) for r in raw]), None, first


# ------------------------------------------------------------------------------------------------------------ through the containers
SAMPLE_NAMES, SAMPLE_LENS = ["k1", "k2"], [300000, 200000]
DEL_AT, DEL_LEN, INS_AT, INS_LEN, CARRIERS = 150000, 300, 90000, 120, 12
N_LONG = 3                                      # carriers of each event that are CG records of more than 65 536 operations


def sample_specs():
    """Two contigs; a 300-bp deletion on k1 and a 120-bp insertion on k2, each carried by twelve reads that start at different places.
    Three carriers of each are reads of more than 65 536 operations (`=` 3 / X 1 by turns: about 130 kb of reference).
    Returns [(contig id, spec)] in coordinate order."""
    assert pattern_checked()
    rng = np.random.default_rng(702)
    allele = rng.integers(0, 4, INS_LEN)
    out = []
    for cid, at, ev in ((0, DEL_AT, (D, DEL_LEN)), (1, INS_AT, (I, INS_LEN))):
        for k in range(CARRIERS):
            if k < N_LONG:
                n = U16 + 2 + 97 * k                    # operations; the event after `before` operations of two bases each on average
                before = 30001 + 2 * k
                ops = long_ops(n, {before: ev})
                start = at - sum(ln for op, ln in ops[:before] if op in REF)
            else:
                a, b = 2000 + 137 * k, 2500 + 59 * k
                ops = [(M, a), ev, (M, b)]
                start = at - a
            out.append((cid, start, k, ops))
    out.sort(key=lambda x: (x[0], x[1]))
    specs = [(cid, Spec(start, ops, [int_tag("NM", "S", 400 + k)], ref_id=cid, name=f"q{cid}_{k:02d}")) for cid, start, k, ops in out]
    return specs, allele


def _sample_records(as_twin):
    from sniffles_amd import synth_bam
    specs, allele = sample_specs()
    code = np.array([1, 2, 4, 8], np.uint8)
    rng = np.random.default_rng(703)
    recs = []
    for cid, s in specs:
        parts = []
        for op, n in s.ops:
            if op == I and n == INS_LEN:
                parts.append(allele)
            elif op in QRY:
                parts.append(rng.integers(0, 4, n))
        codes = code[np.concatenate(parts)]
        ops = merged(s.ops) if as_twin and len(s.ops) > U16 else s.ops
        recs.append(synth_bam.make_record(cid, s.pos, 60, 0, s.name, ops, codes, b"".join(s.tags)))
    return recs


@functools.lru_cache(maxsize=None)
def sample_records():
    """(records of the sample, records of its twin)"""
    return _sample_records(False), _sample_records(True)
