"""Record tables that put the extraction kernels (csrc/snf_extract.hip) on the internal edges the seeded fuzz tables reach only by
chance: the 256-operation step of the CIGAR walk and its prefetch, the emit pass that restarts at the first lead-bearing step, the
clip operations lanes 0..7 hold, the LDS copy of the auxiliary region / of the SA string and the size at which it is given up, the
64-byte chunks of the SA cutter and of the NUL search, the 8-byte comma scanner, the segment table, the chunks of the NM sum and
the blocks of the thread form.  Every boundary number comes from size_classes.extract_thresholds(); nothing is random except the read
bases (a seeded generator: a wrong base offset shows as a wrong inserted sequence).

Three tables are registered in cases.EXTRACT (goldens from the unmodified reference); the others are built by tests/test_extract_edges.py
and judged against the oracle there."""
import struct

import numpy as np

import size_classes as sc

M, I, D, N, S, H, P, EQ, X = range(9)
CONTIGS, CONTIG_LENS = ["c1", "c2"], [400000, 50000]
REGION = (50000, 250000)              # of the `cigar` table: records and events are placed on its two ends
# settings of the `cigar` table (cases.EXTRACT carries the same as reference arguments): an odd long_ins_length, so that half of it
# lies between two clip lengths, and a sequence cache small enough for an insertion on either side of it
CIGAR_CFG = dict(long_ins_length=2501, dev_seq_cache_maxlen=400)
MINSVLEN_SCREEN = 45                  # default of the reference (config.py): int(0.9 * 50)


def T():
    return sc.extract_thresholds()


class Table:
    """Records in BAM order; bases from one seeded generator."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.recs = []

    def add(self, pos, ops, tags=b"", flag=0, mapq=60, ref_id=0, name=None, seq=True):
        from sniffles_amd import synth_bam
        ops = [(int(op), int(n)) for op, n in ops]
        qlen = sum(n for op, n in ops if op in (M, I, S, EQ, X)) if seq else 0
        codes = self.rng.choice(np.array([1, 2, 4, 8], np.uint8), qlen)      # A C G T
        self.recs.append(synth_bam.make_record(ref_id, int(pos), mapq, flag, name or f"r{len(self.recs):04d}", ops, codes, tags))
        return len(self.recs) - 1

    def records(self):
        from sniffles_amd import bam
        return bam.records_from_list(CONTIGS, CONTIG_LENS, self.recs)


# ------------------------------------------------------------------------------------------------------------ tags
def int_tag(name, ty, v):
    return name.encode() + ty.encode() + struct.pack("<" + dict(c="b", C="B", s="h", S="H", i="i", I="I")[ty], v)


def z_tag(name, n, fill=b"x"):
    """a Z tag whose string has n bytes (the NUL is byte n)."""
    return name.encode() + b"Z" + fill * n + b"\0"


def b_tag(name, n_bytes):
    """a B:C array of n_bytes bytes in all (name, type, sub-type and count included)."""
    cnt = n_bytes - 8
    assert cnt >= 0
    return name.encode() + b"BC" + struct.pack("<i", cnt) + bytes(k % 251 for k in range(cnt))


def sa_tag(s):
    return b"SAZ" + s.encode() + b"\0"


# ------------------------------------------------------------------------------------------------------------ the `cigar` table
def ladder_ops(n, t):
    """n operations: 1200M, then short matches, with an insertion on the last operation of every step (the last lane's last
    operation) and a deletion on the first of the next; an even n ends on a soft clip of lead size."""
    ops = [(M, 1200)] + [(M, 5 + k % 3) for k in range(1, n)]
    step = t["step"]
    for j, b in enumerate(range(step, n + 1, step)):
        if 1 <= b - 1 < n - 1:
            ops[b - 1] = (I, 50 + j)
        if b < n - 1:
            ops[b] = (D, 60 + j)
    if n % 2 == 0:
        ops[n - 1] = (S, 60)
    return ops[:n]


def steps_ops(n, bearing, t):
    """n short operations; the steps named in `bearing` hold an insertion (lane 2's third operation) and a deletion (lane 25's
    second), the others nothing of lead size."""
    ops = [(M, 1200)] + [(M, 3 + k % 4) for k in range(1, n)]
    opl = t["opl"]
    assert opl >= 3 and sc.WAVE > 25
    for s in bearing:
        ops[s * t["step"] + 2 * opl + 2] = (I, 70 + s)
        ops[s * t["step"] + 25 * opl + 1] = (D, 80 + s)
    return ops


def clip_run(k, hard):
    """k clip operations as they stand on the LEFT end, the hard clip outermost: 30S, 35S, ... (45S and more are of lead size)."""
    if k == 0:
        return []
    run = [(H, 7)] if hard else []
    return run + [(S, 30 + 5 * j) for j in range(k - len(run))]


def cigar_table():
    t = T()
    tb = Table(601)
    step, rs, re_ = t["step"], REGION[0], REGION[1]
    pos = iter(range(60000, 240000, 150))
    # steps of the longest CIGARs: with leads in step 0 alone, walk_hi lies inside the CIGAR and steps are left over that the walk of
    # step 0 has not even requested (it requests X_AHEAD ahead)
    n_steps = 5
    assert n_steps > 1 + t["ahead"]
    # (a) the ladder of operation counts: up to a clip operation more than lanes 0..7 hold, and around every whole number of steps
    for n in sorted({1, 2, 3, 4, 5, t["clip_lanes_end"], t["clip_lanes_end"] + 1} | set(sc.around(*(k * step for k in range(1, n_steps + 1))))):
        tb.add(next(pos), ladder_ops(n, t), int_tag("NM", "C", 9))
    # (b) five steps; which of them bear leads (the emit pass restarts at the first, and stops after the last, that does)
    n_ops = n_steps * step - (t["opl"] - 1)       # the last lane that holds any holds one operation
    for bearing in [(s,) for s in range(n_steps)] + [(0, n_steps - 1), (1, n_steps - 1)]:
        tb.add(next(pos), steps_ops(n_ops, bearing, t), int_tag("NM", "S", 300))
    # (c) clip runs of 0..5 operations on either end (lanes 0..3 and 4..7 hold four each; the fifth is read by the serial loop)
    for l in range(t["clip_lanes"] + 2):
        for r in range(t["clip_lanes_end"] - t["clip_lanes"] + 2):
            hard = (l + r) % 2 == 0
            tb.add(next(pos), clip_run(l, hard) + [(M, 1100), (I, 60), (M, 300)] + clip_run(r, not hard and r > 1)[::-1])
    # (d) a step in which every operation of every lane is an event, and the events that follow in the next
    pairs = 200
    assert step < 2 * pairs < 2 * step
    tb.add(next(pos), [(M, 1200)] + [(M, 2)] * (step - 1) + [(I, 50), (D, 50)] * pairs + [(M, 40)], int_tag("NM", "S", 100 * pairs + 100))
    # (e) two and three insertions among one lane's operations
    tb.add(next(pos), [(M, 1200), (I, 50), (I, 60), (M, 5)] + [(I, 55), (I, 65), (I, 75), (M, 9)] + [(M, 100)])
    tb.add(next(pos), [(M, 1200), (I, 50), (D, 47), (I, 60)] + [(M, 4), (I, 55), (M, 1), (I, 65)] + [(I, 75), (M, 100)])
    # (f) insertions of one wave of bases, one fewer, one more: at even and odd read offsets, and as the last bases of an odd l_seq
    for n in sc.around(sc.WAVE):
        for odd in (0, 1):
            tb.add(next(pos), [(M, 1200 + odd), (I, n), (M, 100)])
        tb.add(next(pos), [(M, 1200 + (n % 2 == 0)), (I, n)])
    # (g) events one base short of the screen, and on it
    for n in (MINSVLEN_SCREEN - 1, MINSVLEN_SCREEN):
        tb.add(next(pos), [(S, n), (M, 1200), (I, n), (M, 20), (D, n), (M, 50), (S, n)])
    # (h) insertions the sequence cache still takes / no longer takes
    for n in (CIGAR_CFG["dev_seq_cache_maxlen"], CIGAR_CFG["dev_seq_cache_maxlen"] + 1):
        tb.add(next(pos), [(M, 1300), (I, n), (M, 77)], int_tag("NM", "S", 500))
    # (i) the "large" rule of NM: indels of more than 10 bases are taken off the tag
    tb.add(next(pos), [(M, 1200), (I, 10), (M, 5), (I, 11), (M, 5), (D, 10), (M, 5), (D, 11), (M, 30), (I, 60), (M, 100)], int_tag("NM", "C", 140))
    # (j) a clip of half the (odd) long_ins_length, rounded down and up, on either end
    half = CIGAR_CFG["long_ins_length"] // 2
    assert CIGAR_CFG["long_ins_length"] % 2 == 1
    for n in (half, half + 1):
        tb.add(next(pos), [(S, n), (M, 1200)])
        tb.add(next(pos), [(M, 1200), (S, n)])
    # (k) the region's ends: the record's position, an event's start, a deletion's end
    for p in (rs - 1, rs, rs + 1, re_ - 1, re_):
        tb.add(p, [(S, 60), (M, 1100), (I, 50), (M, 100)], int_tag("NM", "C", 3))
    for edge in (rs, re_):
        tb.add(edge - 1 - 1100, [(M, 1100), (I, 60), (M, 1), (I, 61), (M, 1), (I, 62), (M, 50)])      # insertions at edge - 1, edge, edge + 1
        tb.add(edge - 1 - 1100, [(M, 1100), (D, 60), (M, 50)])                                        # deletions that start at edge - 1, edge,
        tb.add(edge - 1100, [(M, 1100), (D, 61), (M, 50)])                                            # edge + 1
        tb.add(edge + 1 - 1100, [(M, 1100), (D, 62), (M, 50)])
        for n in (999, 1000, 1001):
            tb.add(edge - 2000, [(M, 1000), (D, n), (M, 500)])                                        # deletions that end at edge - 1, edge, edge + 1
    # (l) read names of 1..16 bytes: whatever follows the name at every alignment modulo 16
    for k in range(1, 17):
        tb.add(next(pos), [(S, 50), (M, 1200), (I, 60 + k), (M, 300)],
               int_tag("NM", "C", k) + int_tag("HP", "C", k % 3) + int_tag("PS", "i", 1000 * k) + sa_tag(el(pos=90000 + k, strand="-") + ";"), name="n" * k)
    return tb.records()


# ------------------------------------------------------------------------------------------------------------ the `sa` table
SA_OPS = [(S, 300), (M, 1200), (I, 80), (M, 400), (S, 100)]
SA_QLEN = 2080


def el(pos=5000, strand="+", clip0=1000, span=500, mapq=60, nm=3, contig="c1"):
    return f"{contig},{pos},{strand},{clip0}S{span}M{SA_QLEN - clip0 - span}S,{mapq},{nm}"


def elements(n, k0=0):
    """n SA elements: strands, contigs, clips and positions mixed (same- and other-strand neighbours, gaps and overlaps in the read)."""
    out = []
    for k in range(k0, k0 + n):
        out.append(el(pos=61000 + 937 * k, strand="-" if k % 3 == 1 else "+", clip0=(211 * k) % 1500, span=300 + 17 * (k % 9),
                      mapq=60 - (k % 5) * 11, nm=k % 13, contig="c2" if k % 7 == 3 else "c1"))
    return out


def sized(element, n):
    """the element, n bytes long: its position written with leading zeros."""
    f = element.split(",")
    assert len(element) <= n
    f[1] = f[1].zfill(len(f[1]) + n - len(element))
    return ",".join(f)


def sa_record(tb, pos, sa, flag=0, tags_before=None, tags_after=b"", mapq=60):
    return tb.add(pos, SA_OPS, (int_tag("NM", "C", 7) if tags_before is None else tags_before) + sa_tag(sa) + tags_after, flag=flag, mapq=mapq)


def sa_table():
    t = T()
    tb = Table(602)
    pos = iter(range(60000, 240000, 400))
    # element counts up to the segment table (the primary alignment takes one entry)
    for n in (1, 2, 3, 30, t["xmaxseg"] - 2, t["xmaxseg"] - 1):
        sa_record(tb, next(pos), ";".join(elements(n, n)) + ";")
    two = elements(2, 5)
    lens = sorted(set(sc.around(t["sa_chunk"], 2 * t["sa_chunk"], t["xauxcap"])) | {t["xauxcap"] - 2})
    for total in lens:      # the string's length, padded with empty elements in front / in the middle (the emit pass keeps total + 1 bytes in LDS)
        body = ";".join(two) + ";"
        assert total >= len(body)
        sa_record(tb, next(pos), ";" * (total - len(body)) + body)
        sa_record(tb, next(pos), two[0] + ";" * (total - len(body) + 1) + two[1] + ";")
    # an element's first byte, then its terminator, on the last byte of a 64-byte chunk and on the first of the next
    a, b = elements(2, 11)
    for chunk in (t["sa_chunk"], 2 * t["sa_chunk"]):
        for at in (chunk - 1, chunk):
            sa_record(tb, next(pos), ";" * at + a + ";" + b + ";")                           # a starts at `at`
            sa_record(tb, next(pos), ";" * (at - len(a)) + a + ";" + b + ";")                # a's terminator at `at`
            sa_record(tb, next(pos), a + ";" * (at - len(a)) + b)                            # b starts at `at`; no trailing ';' (the NUL ends it)
    for off in range(t["comma_word"]):      # an element at every offset modulo 8 of the comma scanner's reads
        sa_record(tb, next(pos), ";" * off + ";".join(elements(3, 20 + off)) + ";")
    for n in range(32, 32 + t["comma_word"]):   # ... and of every length modulo 8 (its last read holds 1..8 bytes of it; the position is padded with zeros)
        sa_record(tb, next(pos), ";".join(sized(e, n) for e in elements(2, n)) + ";")
    # the same elements on a reverse-strand primary and on supplementary records
    for flag in (0x10, 0x800, 0x810):
        for n in (1, 3):
            sa_record(tb, next(pos), ";".join(elements(n, 2)) + ";", flag=flag)
    sa_record(tb, next(pos), ";".join(elements(2, 31)) + ";", tags_before=b"", tags_after=int_tag("NM", "C", 4))      # no NM in front: the string starts the region
    # the longer clip on the right end (the break end's side is read off the LAST operation), in CIGARs of two and of one operation too
    for flag, k0 in ((0, 1), (0x10, 2)):
        tb.add(next(pos), SA_OPS[::-1], int_tag("NM", "C", 7) + sa_tag(";".join(elements(2, k0)) + ";"), flag=flag)
    tb.add(next(pos), [(M, 1200), (S, SA_QLEN - 1200)], int_tag("NM", "C", 7) + sa_tag(elements(1, 1)[0] + ";"))
    tb.add(next(pos), [(M, SA_QLEN)], int_tag("NM", "C", 7) + sa_tag(elements(1, 4)[0] + ";"))
    # a record of the other contig in between, and the SA string as the last bytes of the blob
    tb.add(1000, SA_OPS, int_tag("NM", "C", 7) + sa_tag(";".join(elements(3, 0)) + ";"), ref_id=1)
    sa_record(tb, next(pos), ";".join(elements(3, 40)))
    return tb.records()


# ------------------------------------------------------------------------------------------------------------ the `tags` table
TAG_OPS = [(S, 50), (M, 1100), (I, 60), (M, 300)]


def tags_table():
    t = T()
    tb = Table(603)
    pos = iter(range(60000, 240000, 400))
    cap = t["xauxcap"]
    last = dict(NM=int_tag("NM", "S", 321), HP=int_tag("HP", "C", 2), PS=int_tag("PS", "i", 70707))
    # the region of cap - 1 / cap / cap + 1 bytes, the tag that matters as its last bytes
    for total in sc.around(cap):
        for key in ("NM", "HP", "PS"):
            room = total - len(last[key])
            tb.add(next(pos), TAG_OPS, b_tag("xb", room) + last[key])
            tb.add(next(pos), TAG_OPS, z_tag("xz", room - 4) + last[key])
    # a long array in front of a short SA string: the counting pass parses where the record lies, the emit pass in its LDS copy
    tb.add(next(pos), SA_OPS, int_tag("NM", "C", 5) + b_tag("xb", 2000) + sa_tag(";".join(elements(2, 3)) + ";"))
    # strings whose NUL lies around the ends of the 64-byte steps of the NUL search
    for n in sc.around(t["nul_chunk"], 2 * t["nul_chunk"]):
        tb.add(next(pos), TAG_OPS, z_tag("xz", n - 1) + int_tag("NM", "C", n))
        tb.add(next(pos), TAG_OPS, int_tag("HP", "C", 1) + z_tag("xz", n - 1, b"N") + int_tag("PS", "S", n) + int_tag("NM", "s", -n))
    # second occurrences: the first one counts
    tb.add(next(pos), SA_OPS, int_tag("NM", "C", 11) + int_tag("HP", "C", 1) + int_tag("PS", "I", 5) + sa_tag(el(pos=70000, strand="-") + ";")
           + int_tag("NM", "C", 99) + int_tag("HP", "C", 2) + int_tag("PS", "I", 6) + sa_tag(";".join(elements(3, 1)) + ";"))
    tb.add(next(pos), TAG_OPS, int_tag("NM", "C", 12) + z_tag("NM", 5) + b"HPC\x02" + b"HPC\x07")      # (the second NM / HP would fail the call if it counted)
    # every integer type for NM and PS, negative values among them
    vals = dict(c=-3, C=250, s=-300, S=65000, i=-70000, I=2 ** 31 - 1)
    for ty, v in vals.items():
        tb.add(next(pos), TAG_OPS, int_tag("NM", ty, v) + int_tag("PS", ty, v if ty != "I" else 2 ** 32 - 1) + int_tag("HP", ty, 1))
        tb.add(next(pos), TAG_OPS, int_tag("PS", ty, abs(v) // 2) + int_tag("NM", ty, abs(v) // 2))
    return tb.records()


# ------------------------------------------------------------------------------------------------------------ tables without goldens
def mixed_table():
    """What a wave that takes several records must not carry over: a full segment table and a long SA string are followed by a record
    without the tag; records of the other contig and records the MAPQ filter drops lie in between; CIGAR lengths differ, so the
    dispatch order is not the BAM order."""
    t = T()
    tb = Table(604)
    pos = iter(range(60000, 240000, 400))
    for k in range(6):
        sa_record(tb, next(pos), ";".join(elements(t["xmaxseg"] - 1, k)) + ";", flag=0x10 * (k % 2))
        tb.add(next(pos), [(M, 1100), (I, 60 + k), (M, 300)] + [(M, 2), (D, 1)] * (40 * k) + [(M, 5)], int_tag("NM", "C", 17))      # no SA tag
        if k % 2:
            tb.add(1000 + k, SA_OPS, int_tag("NM", "C", 7) + sa_tag(";".join(elements(5, k)) + ";"), ref_id=1)             # the other contig
        if k % 3 == 0:
            sa_record(tb, next(pos), ";".join(elements(4, k)) + ";", mapq=5)                                                # the MAPQ filter drops it
        sa_record(tb, next(pos), ";".join(elements(2, 9 + k)) + ";")
        tb.add(next(pos), [(S, 1300), (M, 1200)], b_tag("xb", 600) + int_tag("PS", "i", k))                                 # a clip lead only without SA
    return tb.records()


def segment_table_records(n_elements, flag=0):
    tb = Table(605)
    tb.add(60000, TAG_OPS, int_tag("NM", "C", 1))
    sa_record(tb, 70000, ";".join(elements(n_elements, 1)) + ";", flag=flag)
    tb.add(80000, TAG_OPS, int_tag("NM", "C", 2))
    return tb.records()


def _nm_records(n, pattern, seed):
    t = T()
    rng = np.random.default_rng(seed)
    lens = rng.integers(1000, 30001, n)
    nms = rng.integers(1, 2000, n)
    tb = Table(seed)
    ratios = []
    for k in range(n):
        has = dict(all=True, third=k % 3 == 0, gap=not (t["nm_chunk"] <= k < 2 * t["nm_chunk"]), zeros=True)[pattern]
        nm = 0 if pattern == "zeros" and k % 5 == 0 else int(nms[k])
        tb.add(1000 + 7 * k, [(M, int(lens[k]))], int_tag("NM", "S", nm) if has else b"", seq=False)
        if has:
            ratios.append(nm / float(int(lens[k]) + 1))
    return tb, ratios


def ordered_mean(ratios):
    s = 0.0
    for r in ratios:
        s += r
    return s / float(max(1, len(ratios)))


def nm_records(n, pattern):
    """n records of one M operation (1000..30000 bases, no sequence stored) with NM drawn from a seed.  pattern: "all"; "third" (every
    third record has the tag); "gap" (none inside the second chunk of x_nmsum); "zeros" (NM = 0 on every fifth: it counts in the divisor
    and is left out of the sum).  The seed is the first from 606 on whose ratios are sensitive to the order they are added in (the mean
    of the reversed list has other bits), so that a sum in another order cannot pass.  Returns (records, the ratios in BAM order)."""
    for seed in range(606, 670):
        tb, ratios = _nm_records(n, pattern, seed)
        if ordered_mean(ratios) != ordered_mean(ratios[::-1]):
            return tb.records(), ratios
    raise AssertionError(f"no order-sensitive NM table of {n} records found")


def block_records(n):
    """n accepted records of one lead each (the 256-thread blocks of the thread form)."""
    tb = Table(607)
    for k in range(n):
        tb.add(60000 + 11 * k, [(M, 1000 + k % 5), (I, 50 + k % 64), (M, 20)])
    return tb.records()


def error_records(pairing):
    """Two records the call fails on; the later one has the longer CIGAR, so the wave form takes it first."""
    t = T()
    tb = Table(608)
    early, late = dict(hp_then_nmz=(b"HPC\x03", b"NMZabc\0"), sa_then_hp=(sa_tag("c1,5000,+,100M,60;"), b"HPC\x09"),
                       aux_then_sa=(b"XXq\x01", sa_tag(el(pos="1x") + ";")))[pairing]
    for k in range(12):
        tags = early if k == 3 else late if k == 9 else int_tag("NM", "C", k)
        ops = [(M, 1200)] + ([(M, 3), (I, 1)] * t["step"] if k == 9 else []) + [(I, 60), (M, 100)]
        tb.add(60000 + 500 * k, ops, tags)
    return tb.records(), 3


BUILDERS = dict(cigar=cigar_table, sa=sa_table, tags=tags_table)
