"""Builders for tests/test_fasta_device.py: FASTA texts whose headers, line ends and runs of 'N' sit on the borders of the device
kernels' work units (sniffles_amd/csrc/snf_fasta.h), and BGZF files with chosen member cuts.  The unit sizes are read from the
source, as tests/size_classes.py does for the other kernels: a literal that is no longer found is an error, not a default."""
import os
import re
import struct
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def chunk_sizes():
    """Bytes a thread, a wave and a workgroup of fa_index / fa_nruns take per step, and bases a wave of fa_gather takes."""
    with open(os.path.join(ROOT, "sniffles_amd", "csrc", "snf_fasta.h")) as f:
        src = f.read()
    out = {}
    for name in ("FA_VEC", "FA_WG", "FA_WAVE_BYTES", "FA_CHUNK", "FA_GATHER_STEP"):
        m = re.findall(rf"^#define {name} (\d+)\b", src, re.M)
        if len(m) != 1:
            raise AssertionError(f"fasta_cases: expected exactly one #define {name} in snf_fasta.h, found {len(m)}")
        out[name] = int(m[0])
    assert out["FA_WAVE_BYTES"] == 64 * out["FA_VEC"] and out["FA_CHUNK"] == out["FA_WG"] * out["FA_VEC"]
    return out


def borders():
    """Every text offset at which the work changes hands: thread, wave and workgroup, up to three workgroup steps."""
    s = chunk_sizes()
    return dict(thread=s["FA_VEC"], wave=s["FA_WAVE_BYTES"], workgroup=s["FA_CHUNK"])


def record(name: bytes, seq: bytes, width: int, nl: bytes = b"\n") -> bytes:
    return b">" + name + nl + b"".join(seq[i:i + width] + nl for i in range(0, len(seq), width))


def bases(rng, n: int, alphabet: bytes = b"ACGT") -> bytes:
    return rng.choice(np.frombuffer(alphabet, np.uint8), n).tobytes() if n else b""


def text_with_header_at(offset: int, rng, nl: bytes = b"\n", width: int = 60, head: bytes = b"second extra words") -> bytes:
    """Two records; the '>' of the second one is byte `offset` of the text."""
    per = width + len(nl)
    for pad in range(per):           # (a longer first name until the last line holds at least one base)
        first = b">a" + b"x" * pad + nl
        full, rest = divmod(offset - len(first), per)
        if offset > len(first) and (rest == 0 or rest > len(nl)):
            break
    else:
        raise AssertionError(offset)
    seq_len = full * width + (rest - len(nl) if rest else 0)
    seq = bases(rng, seq_len)
    body = b"".join(seq[i:i + width] + nl for i in range(0, full * width, width))
    if rest:
        body += seq[full * width:] + nl
    out = first + body
    assert len(out) == offset, (len(out), offset)
    return out + record(head, bases(rng, 130), width, nl)


def text_of_length(total: int, rng, width: int = 60) -> bytes:
    """Three records, `total` bytes in all, the last line without a newline when that is what fits."""
    out = record(b"x1", bases(rng, 500), width) + record(b"x2 y", bases(rng, 77), width) + b">x3\n"
    left = total - len(out)
    assert left > 2 * width
    full, rest = divmod(left, width + 1)
    seq = bases(rng, full * width + rest)
    out += b"".join(seq[i:i + width] + b"\n" for i in range(0, full * width, width)) + seq[full * width:]
    assert len(out) == total
    return out


def sequence_with_runs(length: int, runs, fill: bytes = b"ACGT") -> bytes:
    """`fill` repeated, with 'N' over every [start, end) of `runs` (clipped to the sequence)."""
    a = np.resize(np.frombuffer(fill, np.uint8), length).copy()
    for s, e in runs:
        a[max(0, s):max(0, min(e, length))] = 78
    return a.tobytes()


def base_of_text_offset(offset: int, first_base_offset: int, width: int, nl_len: int):
    """The base coordinate of a text offset inside a contig's lines, or None where a line end stands."""
    rel = offset - first_base_offset
    if rel < 0:
        return None
    line, col = divmod(rel, width + nl_len)
    return None if col >= width else line * width + col


def bgzf_member(chunk: bytes, level: int = 6) -> bytes:
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    cdata = co.compress(chunk) + co.flush()
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(cdata) + 25) + cdata +
            struct.pack("<II", zlib.crc32(chunk) & 0xffffffff, len(chunk)))


EOF = bgzf_member(b"")


def bgzf_cut(raw: bytes, cuts) -> bytes:
    """`raw` as BGZF members of the lengths `cuts` (cycled; 0: an empty member), closed by the EOF member."""
    out, p, k = [], 0, 0
    while p < len(raw):
        n = cuts[k % len(cuts)]
        k += 1
        out.append(bgzf_member(raw[p:p + n]))
        p += n
    return b"".join(out) + EOF


def bgzf_truncated(raw: bytes) -> bytes:
    """A BGZF file whose second member lost the last 6 bytes of its deflate payload (BSIZE says so too: the container is whole,
    the deflate stream is not)."""
    a, b = bgzf_member(raw[:3000]), bgzf_member(raw[3000:])
    payload = b[18:-8][:-6]
    b = b[:16] + struct.pack("<H", len(payload) + 25) + payload + b[-8:]
    return a + b + EOF
