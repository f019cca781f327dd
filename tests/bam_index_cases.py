"""Builders for tests/test_bam_index.py: a restatement of the SAM specification's reg2bin and of htslib's bam_endpos, the virtual
offsets of a member table, a naive index over a record table, and the record tables the device passes are judged on."""
import os
import re
import struct

import numpy as np

import bgzf_cases as B
from sniffles_amd import bam, synth_bam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
M, I, D, N, S, H, P, EQ, X = range(9)
REF_CONSUMING = (M, D, N, EQ, X)


def wave_step() -> int:
    """CIGAR operations a wave of bai_span takes per step: the literal of csrc/snf_bamindex.h."""
    with open(os.path.join(ROOT, "sniffles_amd", "csrc", "snf_bamindex.h")) as f:
        m = re.search(r"^#define BAI_STEP (\d+)\b", f.read(), re.M)
    if not m:
        raise RuntimeError("snf_bamindex.h no longer defines BAI_STEP: the cases around the wave step need its value")
    return int(m.group(1))


# ---- the rules, restated (SAM specification 5.3; htslib bam_endpos) ------------------------------------------------
def reg2bin(beg: int, end: int) -> int:
    end -= 1
    if beg >> 14 == end >> 14: return ((1 << 15) - 1) // 7 + (beg >> 14)
    if beg >> 17 == end >> 17: return ((1 << 12) - 1) // 7 + (beg >> 17)
    if beg >> 20 == end >> 20: return ((1 << 9) - 1) // 7 + (beg >> 20)
    if beg >> 23 == end >> 23: return ((1 << 6) - 1) // 7 + (beg >> 23)
    if beg >> 26 == end >> 26: return ((1 << 3) - 1) // 7 + (beg >> 26)
    return 0


def fields(rec: bytes):
    """(ref, pos, flag, [(op, len)], stored bin) of a record that starts with its block_size."""
    ref, pos, l_name, _mapq, bn, n_cig, flag = struct.unpack_from("<iiBBHHH", rec, 4)
    ops = [(c & 15, c >> 4) for c in struct.unpack_from(f"<{n_cig}I", rec, 36 + l_name)]
    return ref, pos, flag, ops, bn


def endpos(rec: bytes) -> int:
    ref, pos, flag, ops, _ = fields(rec)
    rlen = sum(ln for op, ln in ops if op in REF_CONSUMING)
    return pos + 1 if rlen == 0 or flag & 0x4 else pos + rlen


def voffset(members, foff, p: int) -> int:
    """Stream position -> virtual offset: the member that holds the byte (never an empty one); behind the stream: foff[-1] << 16."""
    for m in range(members.shape[0]):
        a = int(members["out_off"][m])
        if a <= p < a + int(members["isize"][m]):
            return int(foff[m]) << 16 | (p - a)
    assert p == int(members["isize"].sum())
    return int(foff[-1]) << 16


def expected_tables(recs, starts, members, foff):
    """Per record (end, bin, vbeg, vend) by the restated rules; `starts`: stream position of every record and the end."""
    out = []
    for r, a, b in zip(recs, starts[:-1], starts[1:]):
        _, pos, _, _, _ = fields(r)
        e = endpos(r)
        out.append((e, reg2bin(pos, e) & 0xffffffff, voffset(members, foff, a), voffset(members, foff, b)))
    return out


def naive_runs(recs, exp):
    """[(ref, bin, beg, end)] - a chunk per change of (ref, bin) in file order, then stably sorted by (ref, bin)."""
    runs, prev = [], None
    for r, (e, bn, vb, ve) in zip(recs, exp):
        ref = fields(r)[0]
        if ref < 0:
            break
        if prev != (ref, bn):
            runs.append([ref, bn, vb, ve])
        else:
            runs[-1][3] = ve
        prev = (ref, bn)
    return sorted(runs, key=lambda x: (x[0], x[1]))


def naive_linear(recs, exp, win_off):
    lin = {}
    for r, (e, bn, vb, ve) in zip(recs, exp):
        ref, pos, flag, _, _ = fields(r)
        if ref < 0 or flag & 0x4:
            continue
        for w in range(pos >> 14, ((e - 1) >> 14) + 1):
            k = int(win_off[ref]) + w
            lin[k] = min(lin.get(k, vb), vb)
    return lin


# ---- records ------------------------------------------------------------------------------------------------------------
NAMES = ["c0", "c1", "c2"]
LENS = [1 << 29, 1 << 29, 3_000_000]


def rec(ref, pos, ops, flag=0, name="r", l_seq=None, tags=b"", stored_bin=None):
    q = sum(ln for op, ln in ops if op in (M, I, S, EQ, X)) if l_seq is None else l_seq
    q = min(q, 40)                     # (the sequence is not read by the index; short records keep the files small)
    r = bytearray(synth_bam.make_record(ref, pos, 60, flag, name, ops, np.ones(q, np.uint8), tags))
    if stored_bin is not None:
        struct.pack_into("<H", r, 14, stored_bin)
    return bytes(r)


def span_table():
    """Records of one file, sorted: every CIGAR / interval case of the span kernel.  [(label, record)]."""
    step = wave_step()
    out, pos = [], 1000
    def add(label, ops, flag=0, at=None, ref=0, **kw):
        nonlocal pos
        p = pos if at is None else at
        out.append((label, rec(ref, p, ops, flag, name=f"q{len(out)}", **kw)))
        if ref == 0:
            pos = max(pos, p) + 3
    for n in sorted({0, 1, 63, 64, 65, 127, 128, 129, step - 1, step, step + 1, 2 * step - 1, 2 * step, 2 * step + 1, 3 * step + 5}):
        add(f"ops_{n}", [((M, I, EQ, D, X, S, N)[k % 7], 1 + k % 5) for k in range(n)])
    for op in range(9):
        add(f"only_{'MIDNSHP=X'[op]}", [(op, 37)])
    add("all_mixed", [(S, 5), (M, 100), (I, 7), (M, 3), (D, 11), (EQ, 9), (X, 2), (N, 500), (P, 1), (M, 40), (H, 6)])
    add("ref_length_zero", [(S, 10), (I, 20)])
    add("flag_unmapped_with_position", [(M, 5000)], flag=0x4)
    add("long_cigar_placeholder", [(S, 70000), (N, 123456)], l_seq=70000,
        tags=b"CGBI" + struct.pack("<i", 3) + struct.pack("<3I", (70000 << 4) | M, (53456 << 4) | D, 0))
    add("stale_bin", [(M, 20000)], stored_bin=1)
    for s in (14, 17, 20, 23, 26):
        k = 3
        add(f"border_{s}_across", [(M, 2)], at=k * (1 << s) - 1)
        add(f"border_{s}_up_to", [(M, 2)], at=(k + 1) * (1 << s) - 2)
    add("just_below_2_29", [(M, 10)], at=(1 << 29) - 10)
    add("second_reference", [(M, 300)], at=5, ref=1)
    add("third_reference_long", [(M, 16384 * 64 + 5)], at=16384 - 2, ref=2)
    for k in range(3):
        out.append((f"unplaced_{k}", rec(-1, -1, [], flag=0x4, name=f"u{k}")))
    labels = [a for a, _ in out]
    assert len(set(labels)) == len(labels)
    return out


def stream_of(recs, names=NAMES, lens=LENS):
    raw = bam.bam_stream(names, lens, recs)
    hlen = len(raw) - sum(len(r) for r in recs)
    starts = np.cumsum([hlen] + [len(r) for r in recs]).tolist()
    return raw, hlen, starts


def windows_table():
    """Reads that cover 1, 2, 63, 64 and 65 windows of 16 kb, several over the same windows (the minima compete)."""
    recs, pos = [], 100
    for k, nwin in enumerate((1, 2, 63, 64, 65, 2, 1, 64, 65, 1)):
        recs.append(rec(0, pos, [(M, (nwin - 1) * 16384 + 10)], name=f"w{k}"))
        assert ((pos + (nwin - 1) * 16384 + 9) >> 14) - (pos >> 14) + 1 == nwin
        pos += 5000
    recs += [rec(1, 16384 * k + 16000, [(M, 500)], name=f"x{k}") for k in range(12)]
    recs.append(rec(-1, -1, [], flag=0x4, name="u"))
    return recs


def sample_file(seed=31, members_of=700):
    """About 300 reads over three contigs, most of them over several 16-kb windows, a few flagged unmapped at their mate's place, an
    unplaced tail; short sequences keep the file small, small members make the records cross their borders (at least 20 members per
    contig): (file bytes, names, lens, records)."""
    rng = np.random.default_rng(seed)
    names, lens = ["chr20", "chr21", "chr22"], [900_000, 800_000, 700_000]
    recs = []
    for ref, ln in enumerate(lens):
        lo, hi = 60_000 + 20_000 * ref, ln - 150_000
        pos = np.sort(rng.integers(lo, hi, 100))
        pos[40:60] = pos[40] + 200_000 + np.sort(rng.integers(0, 3000, 20))      # (an empty stretch of windows before them)
        pos = np.sort(pos)
        for k, p0 in enumerate(pos.tolist()):
            span = int(rng.choice([300, 5000, 16384, 40000, 100000]))
            ops, left = [(S, int(rng.integers(1, 30)))], span
            while left > 0:
                run = int(min(left, rng.integers(50, 9000)))
                ops.append((int(rng.choice([M, EQ, X])), run))
                left -= run
                if left > 0:
                    ops.append((I, int(rng.integers(1, 60))) if rng.random() < 0.5 else (int(rng.choice([D, N])), int(min(left, rng.integers(1, 700)))))
                    left -= ops[-1][1] if ops[-1][0] != I else 0
            flag = 0x4 if k % 37 == 5 else (0x10 if k % 2 else 0)
            recs.append(rec(ref, p0, ops if not flag & 0x4 else [], flag, name=f"read_{ref}_{k:03d}_" + "x" * int(rng.integers(0, 40))))
    recs += [rec(-1, -1, [], 0x4, name=f"unplaced_{k}") for k in range(7)]
    raw, hlen, starts = stream_of(recs, names, lens)
    # a member border where the contig changes: the member that holds the end of one contig is then not read for the next one too,
    # and the bytes the contigs read add up to less than the file
    first = [starts[k] for k in range(1, len(recs)) if fields(recs[k])[0] != fields(recs[k - 1])[0]]
    return B.reblock(raw, sorted(first + list(range(members_of, len(raw), members_of)))), names, lens, recs
