"""Inputs for tests/test_deflate.py: the smallest shapes at which each part of deflate_member (sniffles_amd/csrc/snf_deflate.h)
can go wrong.  The kernel's widths are read from the header, as tests/size_classes.py does for the other kernels."""
import os
import random
import re
import struct
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FF00 = 0xff00
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def widths():
    with open(os.path.join(ROOT, "sniffles_amd", "csrc", "snf_deflate.h")) as f:
        src = f.read()
    val = lambda name: int(re.search(rf"#define {name} (\w+)", src).group(1), 0)
    w = dict(wg=val("DZ_WG"), tok=val("DZ_TOK"), max=val("DZ_MAX"), minlen=val("DZ_MINLEN"))
    assert w["max"] == FF00 and w["wg"] % 64 == 0
    return w


def rnd(seed, n, alphabet=None):
    r = random.Random(seed)
    return bytes(r.choice(alphabet) for _ in range(n)) if alphabet else bytes(r.getrandbits(8) for _ in range(n))


def de_bruijn(k, n):
    """Every n-gram over k symbols exactly once (Lyndon words): no substring of n symbols repeats."""
    a, seq = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    return bytes(seq)


def fibonacci_counts():
    """Bytes with Fibonacci counts over 22 symbols, 46 367 of them, shuffled: an unlimited Huffman code is 21 bits deep."""
    fib = [1, 1]
    while len(fib) < 22:
        fib.append(fib[-1] + fib[-2])
    data = bytearray()
    for s, c in enumerate(fib):
        data += bytes([65 + s]) * c
    assert len(data) == 46367
    random.Random(22).shuffle(data)
    return bytes(data)


def distance_case(at):
    """1000 random bytes at offset 0, filler that shares no four bytes with them, the same 1000 bytes again at offset `at`."""
    head = rnd(3, 1000, bytes(range(128, 256)))
    filler = rnd(4, at - 1000, bytes(range(0, 128)))
    return head + filler + head + rnd(5, 300, bytes(range(0, 128)))


def skewed_no_repeats(m, seed):
    """Even bytes: a sequence in which no pair repeats; odd bytes: m symbols with Fibonacci counts, shuffled.  No four bytes repeat, so the
    member is literals alone, and their code lengths spread from 2 bits to 13 and more."""
    fib = [1, 1]
    while len(fib) < m:
        fib.append(fib[-1] + fib[-2])
    odd = [200 + s for s, c in enumerate(fib) for _ in range(c)]
    random.Random(seed).shuffle(odd)
    k = 2
    while k * k < len(odd) + 1:
        k += 1
    assert k < 200
    out = bytearray()
    for c, s in zip(de_bruijn(k, 2), odd):
        out += bytes([c, s])
    return bytes(out)


def long_tokens():
    """Tokens of more than 32 bits, which reach into a third dword at the higher bit offsets: a few long matches far back (length
    symbols 281 .. 284 with 5 extra bits and distance symbol 28 with 13, all rare, so their codes are long) among many near ones and
    literals with a skewed histogram."""
    r = random.Random(2)
    out = bytearray(skewed_no_repeats(19, 3))      # 21 890 bytes
    for k in range(1500):                          # near matches: the distance symbols of the far ones become rare
        p = 40 + 14 * k
        d = 5 + (k % 4)
        out[p:p + 6] = out[p - d:p - d + 6]
    filler = skewed_no_repeats(18, 4)
    out += filler[:12000]
    for j in range(14):
        n, d = 131 + r.randrange(127), 16385 + r.randrange(3000)
        a = len(out) - d
        out += out[a:a + n] + filler[12000 + 40 * j:12040 + 40 * j]
    return bytes(out[:FF00])


def period(p, n, seed=9):
    unit = rnd(seed + p, p)
    return (unit * (n // p + 1))[:n]


def all_cases():
    """[(name, input bytes)], each at most 0xff00 bytes."""
    w = widths()
    wg, tile = w["wg"], w["wg"] * w["tok"]
    out = []
    lengths = {0, 1, 2, 3, 4, 5, 63, 64, 65, FF00 - 1, FF00}
    for edge in (wg, 2 * wg, tile):      # a match round, two of them, an emission round of literals
        lengths |= {edge - 1, edge, edge + 1}
    for n in sorted(lengths):
        out.append((f"len{n}", rnd(100 + n, n, b"ACGTN\n\t0123456789") if n < FF00 - 1 else rnd(100 + n, n, b"ACGT")))
    for n in sorted({258, 259, 260, 261, 262, wg - 1, wg, wg + 1, wg + 258, wg + 259, FF00}):
        out.append((f"equal{n}", b"\x55" * n))
    for p in sorted({2, 3, 4, 5, 63, 64, 65, 257, 258, 259, 300, wg - 1, wg, wg + 1}):
        out.append((f"period{p}", period(p, 3 * wg + 7 if p < 300 else 5 * p + 3)))
    out.append(("period300_full", period(300, FF00)))
    # a match that ends exactly on the member's last byte; one whose continuation would run past it (the bytes behind the member
    # in a strided workgroup's LDS are those of the member before: tests put the same period there)
    out.append(("period_ends_on_last_byte", period(300, 300 + 258)))      # 300 literals, one match of 258 up to the last byte
    out.append(("period_cut_by_the_end", period(300, 300 + 258 + 142)))      # ... and one of 142 whose source goes on matching
    out.append(("distance32768", distance_case(32768)))
    out.append(("distance32769", distance_case(32769)))
    out.append(("fibonacci", fibonacci_counts()))
    out.append(("literals_200_distinct", bytes(range(200))))
    out.append(("literals_de_bruijn", de_bruijn(16, 3)))      # 4096 bytes over 16 symbols, no three bytes repeat: a dynamic block of literals alone
    out.append(("single_byte", b"x"))
    out.append(("random_full", rnd(7, FF00)))
    out.append(("random_full_minus_1", rnd(8, FF00 - 1)))
    out.append(("acgt_full", rnd(11, FF00, b"ACGT")))
    out.append(("long_tokens", long_tokens()))
    out.append(("skewed_literals", skewed_no_repeats(20, 5)))
    names = [n for n, _ in out]
    assert len(names) == len(set(names)) and all(len(d) <= FF00 for _, d in out)
    return out


def members_of(image: bytes):
    """[(offset, size, payload, crc, isize)] of a run of BGZF members: the 18-byte header checked field by field."""
    out, p = [], 0
    while p < len(image):
        assert image[p:p + 12] == bytes.fromhex("1f8b08040000000000ff0600"), (p, image[p:p + 12].hex())
        assert image[p + 12:p + 16] == b"BC\x02\x00"
        size = struct.unpack_from("<H", image, p + 16)[0] + 1
        crc, isize = struct.unpack_from("<II", image, p + size - 8)
        out.append((p, size, image[p + 18:p + size - 8], crc, isize))
        p += size
    assert p == len(image)
    return out


def zlib_sizes(data: bytes, member_len, level):
    total, p = 0, 0
    for n in member_len:
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        total += len(c.compress(data[p:p + n]) + c.flush()) + 26
        p += n
    return total


def header_code_lengths(payload: bytes):
    """(literal/length code lengths, distance code lengths) of the dynamic block a payload begins with, decoded as RFC 1951 3.2.7 says."""
    bits, pos = int.from_bytes(payload[:1024], "little"), 0

    def take(n):
        nonlocal pos
        v = (bits >> pos) & ((1 << n) - 1)
        pos += n
        return v
    assert take(1) == 1 and take(2) == 2
    hlit, hdist, hclen = take(5) + 257, take(5) + 1, take(4) + 4
    cl = [0] * 19
    for i in range(hclen):
        cl[(16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)[i]] = take(3)
    codes, code = {}, 0
    for n in range(1, 8):
        for sym in range(19):
            if cl[sym] == n:
                codes[(n, code)] = sym
                code += 1
        code <<= 1
    lens = []
    while len(lens) < hlit + hdist:
        c, n = 0, 0
        while (n, c) not in codes:
            c, n = (c << 1) | take(1), n + 1
            assert n <= 7
        sym = codes[(n, c)]
        if sym < 16:
            lens.append(sym)
        elif sym == 16:
            lens += [lens[-1]] * (3 + take(2))
        elif sym == 17:
            lens += [0] * (3 + take(3))
        else:
            lens += [0] * (11 + take(7))
    assert len(lens) == hlit + hdist
    return lens[:hlit], lens[hlit:]
