"""Builders of the BGZF / record-chain cases (tests/test_bgzf.py): BGZF framing, a bit writer for the deflate streams zlib does
not emit on demand, the re-blocking of a BAM stream at chosen member sizes.  Every well-formed payload is checked against
`zlib.decompress(payload, -15)` here, every malformed one is checked to be rejected by it: a case cannot pass by being skipped."""
import struct
import zlib

import numpy as np

from sniffles_amd import bam, synth_bam


# ------------------------------------------------------------------------------------------------------- framing
def member(payload: bytes, isize: int, crc: int = 0) -> bytes:
    """One BGZF member around a raw deflate payload (CRC-32 is not checked by either path)."""
    bsize = len(payload) + 25
    assert bsize <= 65536, bsize
    return b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", bsize) + payload + struct.pack("<II", crc, isize)


def good(payload: bytes) -> tuple:
    """(member bytes, expected output) of a payload zlib accepts."""
    raw = zlib.decompress(payload, -15)
    assert len(raw) <= 65536
    return member(payload, len(raw), zlib.crc32(raw)), raw


def bad(payload: bytes, isize=None) -> bytes:
    """A member the host path refuses: zlib rejects the payload, or its output is not ISIZE bytes long."""
    try:
        raw = zlib.decompress(payload, -15)
    except zlib.error:
        return member(payload, 100 if isize is None else isize)
    assert isize is not None and isize != len(raw) and isize > 0, "zlib accepts this payload"
    return member(payload, isize)


def deflate(data: bytes, level=6, strategy=zlib.Z_DEFAULT_STRATEGY) -> bytes:
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return co.compress(data) + co.flush()


# ---------------------------------------------------------------------------------------------------- bit writer
class Bits:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    @property
    def bitpos(self):
        return 8 * len(self.out) + self.n

    def bits(self, v, n):      # a field, least significant bit first
        assert 0 <= v < (1 << n) or n == 0
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 0xff)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, n):      # a Huffman code, most significant bit first
        for b in range(n - 1, -1, -1):
            self.bits((c >> b) & 1, 1)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def bytes_(self, b):
        assert self.n == 0
        self.out += b

    def done(self) -> bytes:
        self.align()
        return bytes(self.out)


def canon(lens) -> dict:
    """Canonical codes of a list of code lengths: symbol -> (code, length)."""
    codes, code = {}, 0
    for ln in range(1, 16):
        for s, l in enumerate(lens):
            if l == ln:
                codes[s] = (code, ln)
                code += 1
        code <<= 1
    return codes


LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 30
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
CL_LENS = [4] * 13 + [5] * 6      # a complete code over all 19 code-length symbols


def len_sym(n):
    if n == 258:
        return 28
    s = max(k for k in range(28) if LBASE[k] <= n)
    return s


def dist_sym(d):
    return max(k for k in range(30) if DBASE[k] <= d)


def put_tokens(w: Bits, tokens, ll, dd):
    """tokens: ints (literals) and (length, distance) pairs; then the end-of-block code."""
    for t in tokens:
        if isinstance(t, tuple):
            n, d = t
            s = len_sym(n)
            w.code(*ll[257 + s]); w.bits(n - LBASE[s], LEXT[s])
            s = dist_sym(d)
            w.code(*dd[s]); w.bits(d - DBASE[s], DEXT[s])
        else:
            w.code(*ll[t])
    w.code(*ll[256])


def fixed_block(w: Bits, tokens, final=True):
    w.bits(1 if final else 0, 1); w.bits(1, 2)
    put_tokens(w, tokens, canon(FIXED_LL), canon(FIXED_D))


def stored_block(w: Bits, data: bytes, final=True, nlen=None):
    w.bits(1 if final else 0, 1); w.bits(0, 2)
    w.align()
    w.bytes_(struct.pack("<HH", len(data), (len(data) ^ 0xffff) if nlen is None else nlen) + data)


def plain_clseq(lens):
    return [(l, 0) for l in lens]


def dynamic_block(w: Bits, tokens, ll_lens, d_lens, final=True, clseq=None, cl_lens=None):
    """A dynamic block with the given code lengths.  clseq: the code-length symbols [(symbol, value of its extra bits)], default one
    literal symbol per length; it must expand to ll_lens + d_lens (a repeat may run across the border)."""
    cl_lens = CL_LENS if cl_lens is None else cl_lens
    clseq = plain_clseq(list(ll_lens) + list(d_lens)) if clseq is None else clseq
    exp = []
    for s, x in clseq:
        if s < 16: exp.append(s)
        elif s == 16: exp += [exp[-1]] * (3 + x)
        elif s == 17: exp += [0] * (3 + x)
        else: exp += [0] * (11 + x)
    assert exp == list(ll_lens) + list(d_lens), "the code-length sequence does not expand to the lengths"
    w.bits(1 if final else 0, 1); w.bits(2, 2)
    w.bits(len(ll_lens) - 257, 5); w.bits(len(d_lens) - 1, 5); w.bits(19 - 4, 4)
    for o in CL_ORDER:
        w.bits(cl_lens[o], 3)
    cl = canon(cl_lens)
    for s, x in clseq:
        w.code(*cl[s])
        if s >= 16:
            w.bits(x, {16: 2, 17: 3, 18: 7}[s])
    put_tokens(w, tokens, canon(ll_lens), canon(d_lens))


def expand(tokens) -> bytes:
    out = bytearray()
    for t in tokens:
        if isinstance(t, tuple):
            n, d = t
            for _ in range(n):
                out.append(out[-d])
        else:
            out.append(t)
    return bytes(out)


# ------------------------------------------------------------------------------------------------------ the data
def data_kinds(n=0xff00):
    rng = np.random.default_rng(77)
    _, _, recs = synth_bam.gen_records(5, 40, read_len_mean=1500)
    out = {"acgt": np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes(),
           "bam": (b"".join(recs) * 2)[:n],
           "equal": b"\x41" * n,
           "random": rng.integers(0, 256, n, dtype=np.uint8).tobytes()}
    for p in (2, 3, 63, 64, 65):
        out[f"period{p}"] = (rng.integers(0, 256, p, dtype=np.uint8).tobytes() * (n // p + 1))[:n]
    assert len(out["bam"]) == n
    return out


def zlib_edges():
    """[(name, member, expected)]: levels 0 / 1 / 6 / 9 and the four strategies over the data kinds, then the member sizes."""
    cases = []
    kinds = data_kinds()
    for kind, data in kinds.items():
        for lvl in (0, 1, 6, 9):
            cases.append((f"{kind}_l{lvl}",) + good(deflate(data, lvl)))
        for nm, st in (("fixed", zlib.Z_FIXED), ("rle", zlib.Z_RLE), ("huff", zlib.Z_HUFFMAN_ONLY), ("filtered", zlib.Z_FILTERED)):
            if kind == "random" and nm in ("fixed", "huff"):      # (more than 64 KB of payload: no BGZF member holds it)
                data_s = data[:0xe000]
            else:
                data_s = data
            cases.append((f"{kind}_{nm}",) + good(deflate(data_s, 6, st)))
    rng = np.random.default_rng(3)
    text = np.frombuffer(b"ACGTN", np.uint8)[rng.integers(0, 5, 65536)].tobytes()
    for n in (0, 1, 2, 63, 64, 65, 0xff00, 65536):
        cases.append((f"size{n}",) + good(deflate(text[:n], 6)))
    return cases


def several_blocks():
    """One member: a fixed block, a stored block that starts at a bit position that is not byte-aligned, a dynamic block that
    reaches back into both, an empty stored block, a fixed block.  Asserted from the writer's bit position."""
    w = Bits()
    t1 = list(b"GATTACA") + [(40, 7), 0x41, (3, 1)]
    fixed_block(w, t1, final=False)
    assert (w.bitpos + 3) % 8 != 0, "the stored block's header must not end on a byte border by itself"
    stored = bytes(range(200, 256)) * 3
    stored_block(w, stored, final=False)
    ll = [0] * 286
    for s, l in ((65, 2), (67, 2), (71, 3), (84, 3), (256, 3), (285, 4), (257, 5), (260, 5)):
        ll[s] = l
    assert sum(2.0 ** -l for l in ll if l) == 1.0
    dl = [2, 2, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2]      # distances 1, 2, 3 and 129..192
    t3 = [65, 67, 71, 84, (258, 3), (6, 2), (3, 170), 84, (258, 1)]
    dynamic_block(w, t3, ll, dl, final=False)
    stored_block(w, b"", final=False)
    fixed_block(w, [(100, 500), 0, 255], final=True)
    m, raw = good(w.done())
    out = expand(t1) + stored
    assert raw[:len(out)] == out and len(raw) > len(out) + 500
    return [("several_blocks", m, raw)]


def _ladder(first_syms):
    """Code lengths 1, 2, ..., 14, 15, 15 (complete, the maximum of 15 bits) over the given symbols in that order."""
    return dict(zip(first_syms, list(range(1, 16)) + [15]))


def handwritten():
    cases = []
    # literal/length and distance codes of 15 bits
    lsyms = [65, 67, 256, 257, 285, 71, 84, 78, 97, 99, 103, 116, 110, 10, 0, 255]
    ll = [0] * 286
    for s, l in _ladder(lsyms).items():
        ll[s] = l
    dl = [0] * 30
    for s, l in _ladder([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 29]).items():
        dl[s] = l
    toks = [65, 67, 0, 255, 10, 110, (3, 1), (258, 2), 71, 84, 78, 97, 99, 103, 116] + [0, 255] * 200 + [(3, 150), (258, 192), (3, 129)]
    toks += [65] * 33000 + [255, (258, 24577), (3, 32768), (258, 30000)]
    assert ll[0] == ll[255] == 15 and dist_sym(150) == 14 and dl[14] == 15 and dist_sym(24577) == 29 and dl[29] == 15
    w = Bits(); dynamic_block(w, toks, ll, dl)
    cases.append(("max_bits",) + good(w.done()))
    # a distance alphabet with exactly one code (distance 1), and one with none (HDIST = 1, that length zero)
    ll2 = [0] * 286
    for s, l in ((65, 1), (256, 2), (257, 3), (285, 3)):
        ll2[s] = l
    w = Bits(); dynamic_block(w, [65, (3, 1), 65, (258, 1), (258, 1)], ll2, [1])
    cases.append(("one_distance_code",) + good(w.done()))
    ll3 = [0] * 257
    ll3[65] = 1; ll3[66] = 2; ll3[256] = 2
    w = Bits(); dynamic_block(w, [65, 66] * 50, ll3, [0])
    cases.append(("no_distance_code",) + good(w.done()))
    # code-length repeats (16, 17, 18) that run across the literal/length - distance border
    ll4 = [0] * 65 + [2, 2] + [0] * (256 - 67) + [2] + [4] * 4       # 65, 66, 256: 2 bits; 257..260: 4 bits (3/4 + 4/16 = 1)
    dl4 = [4, 4, 3, 2] + [0] * 21 + [1]                              # 2/16 + 1/8 + 1/4 + 1/2 = 1
    seq = [(18, 65 - 11), (2, 0), (2, 0), (18, 138 - 11), (18, 256 - 67 - 138 - 11), (2, 0), (4, 0), (16, 5 - 3), (3, 0), (2, 0),
           (18, 21 - 11), (1, 0)]      # 16 copies the 4 three times inside the literal/length lengths and twice beyond the border
    w = Bits(); dynamic_block(w, [65, 66, 65, (3, 1), (4, 2), (5, 3), (6, 4)], ll4, dl4, clseq=seq)
    cases.append(("repeat16_across_border",) + good(w.done()))
    ll5 = [0] * 65 + [1] + [0] * (256 - 66) + [2, 3, 3] + [0] * 8    # HLIT = 267: eight zero lengths at its end
    dl5 = [0] * 5 + [1]                                              # ... and five at the start of the distance lengths (distance 7..8)
    seq = [(18, 65 - 11), (1, 0), (18, 138 - 11), (18, 256 - 66 - 138 - 11), (2, 0), (3, 0), (3, 0), (18, 13 - 11), (1, 0)]
    w = Bits(); dynamic_block(w, [65] * 9 + [(4, 7), (3, 8)], ll5, dl5, clseq=seq)
    cases.append(("repeat18_across_border",) + good(w.done()))
    ll6 = ll5[:259] + [0] * 3
    dl6 = [0] * 3 + [1]
    seq = [(18, 65 - 11), (1, 0), (18, 138 - 11), (18, 256 - 66 - 138 - 11), (2, 0), (3, 0), (3, 0), (17, 6 - 3), (1, 0)]
    w = Bits(); dynamic_block(w, [65] * 9 + [(4, 4)], ll6, dl6, clseq=seq)
    cases.append(("repeat17_across_border",) + good(w.done()))
    # repeat code 16 as the first distance length: it copies the last literal/length length
    ll7 = [0] * 65 + [2, 2] + [0] * (256 - 67) + [2] + [3, 3]         # 3/4 + 2/8 = 1; the last length is 3
    dl7 = [3, 3, 3, 3, 1]                                            # 4/8 + 1/2 = 1
    seq = [(18, 65 - 11), (2, 0), (2, 0), (18, 138 - 11), (18, 256 - 67 - 138 - 11), (2, 0), (3, 0), (3, 0), (16, 4 - 3), (1, 0)]
    w = Bits(); dynamic_block(w, [65, 66, 65, 66, (3, 1), (3, 2), (4, 3), (4, 4), (3, 5)], ll7, dl7, clseq=seq)
    cases.append(("repeat16_first_distance",) + good(w.done()))
    # distance 32 768 with length 258, ending on the last byte of a 65 536-byte member
    rng = np.random.default_rng(9)
    lits = rng.integers(0, 144, 32770).tolist()      # (8-bit fixed codes: the payload stays below 64 KB)
    toks = lits + [(258, 32768)] * 127
    w = Bits(); fixed_block(w, toks)
    m, raw = good(w.done())
    assert len(raw) == 65536
    cases.append(("distance_32768_to_the_end", m, raw))
    # a match whose source is the byte the token directly before it wrote, around the end of a token batch
    for k in (61, 62, 63, 64, 65, 127, 128):
        toks = [(i * 7 + 3) & 0xff for i in range(k)] + [(5, 1), 0x55, (4, 1), (3, 2)] + list(range(70))
        w = Bits(); fixed_block(w, toks)
        cases.append((f"match_after_token_{k}",) + good(w.done()))
    # members whose token count is exactly 63, 64, 65, 128
    for n in (63, 64, 65, 128):
        toks = [((i * 11) & 0xff) if i % 3 else (3 + i % 20, 1 + i % 5) for i in range(n)]
        toks[0] = 7; toks[1] = 9; toks[2] = 1; toks[3] = 4; toks[4] = 200; toks[5] = 33
        assert len(toks) == n
        w = Bits(); fixed_block(w, toks)
        cases.append((f"tokens_{n}",) + good(w.done()))
    return cases


def all_good():
    return zlib_edges() + several_blocks() + handwritten()


def malformed():
    """[(name, member)]: each refused by the host path."""
    out = []
    w = Bits(); w.bits(1, 1); w.bits(3, 2); w.bits(0, 13)
    out.append(("block_type_3", bad(w.done())))
    w = Bits(); stored_block(w, b"hello", nlen=0x1234)
    out.append(("stored_nlen", bad(w.done())))
    w = Bits(); w.bits(1, 1); w.bits(2, 2); w.bits(0, 5); w.bits(0, 5); w.bits(15, 4)
    for _ in range(19):
        w.bits(1, 3)      # nineteen code-length codes of one bit
    w.bits(0, 32)
    out.append(("oversubscribed_code_lengths", bad(w.done())))
    w = Bits(); fixed_block(w, [65, (3, 2), 66])
    out.append(("distance_before_start", bad(w.done())))
    ok = deflate(b"0123456789" * 10, 6)
    out.append(("longer_than_isize", bad(ok, isize=99)))
    out.append(("shorter_than_isize", bad(ok, isize=101)))
    full = deflate(data_kinds(3000)["acgt"], 6)
    out.append(("ends_inside_a_symbol", bad(full[:len(full) // 2], isize=3000)))
    return out


def file_of(members) -> bytes:
    return b"".join(members)


# ------------------------------------------------------------------------------------------------ record chain
REFS = (["chrA", "chr10", "chr2", "chrB_alt"], [400000, 300000, 300000, 100000])


def short_record(i, contig=0):
    return synth_bam.make_record(contig, 100 + i, 60, 0, f"s{i}", [(0, 1)], np.array([1], np.uint8), b"")


def reblock(raw: bytes, borders, level=1) -> bytes:
    """`raw` cut at the given stream positions (repeats give empty members), each piece a BGZF member, plus the EOF member."""
    cuts = [0] + [min(max(0, int(b)), len(raw)) for b in borders] + [len(raw)]
    assert cuts == sorted(cuts)
    cuts = sorted(cuts + [p for a, b in zip(cuts[:-1], cuts[1:]) for p in range(a + 0xff00, b, 0xff00)])      # (no piece above 64 KB)
    ms = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        assert b - a <= 65536
        ms.append(good(deflate(raw[a:b], level))[0] if b > a else member(b"\x03\0", 0))
    ms.append(member(b"\x03\0", 0))
    return b"".join(ms)


def chain_stream(n_reads=30, seed=11, extra=()):
    names, lens, recs = synth_bam.gen_records(seed, n_reads, read_len_mean=600)
    recs = list(recs) + list(extra)
    raw = bam.bam_stream(names, lens, recs)
    hlen = len(raw) - sum(len(r) for r in recs)
    starts = np.cumsum([hlen] + [len(r) for r in recs]).tolist()      # stream position of every record, and the end
    return raw, hlen, starts
