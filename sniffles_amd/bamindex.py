"""BAM indexes on the host: BAI and CSI read, queried and written - SAM specification sections 5.2 and 5.3, CSIv1.

The reference requires an index (`sniffles:172`, `check_index`), takes `bam.mapped` and the per-contig counts from it
(`sniffles:298`, `317`) and reads every task's records with `bam.fetch(contig, start, end)` (`leadprov.py:488`) - all of it
pysam / htslib.  This module is that bookkeeping: numpy and struct only.  The index of a file that has none is built on the
GPU (`bam.index_bam`, csrc/snf_bamindex.h); `bam.open_indexed` fetches through either kind.

A virtual offset is `file offset of a BGZF member << 16 | offset inside its inflated bytes`; a chunk is a pair of them,
[beg, end): the records that START in it.
"""
from __future__ import annotations

import os
import struct
from dataclasses import dataclass, field

import numpy as np

U64_MAX = 0xFFFFFFFFFFFFFFFF


def meta_bin(depth: int) -> int:
    """The pseudo-bin that holds a reference's metadata: one past the last real bin (37450 at depth 5)."""
    return ((1 << (3 * (depth + 1))) - 1) // 7 + 1


def reg2bin(beg: int, end: int, min_shift: int = 14, depth: int = 5) -> int:
    end -= 1
    s, t = min_shift, ((1 << (3 * depth)) - 1) // 7
    for l in range(depth, 0, -1):
        if beg >> s == end >> s:
            return t + (beg >> s)
        s += 3
        t -= 1 << (3 * (l - 1))
    return 0


def reg2bins(beg: int, end: int, min_shift: int = 14, depth: int = 5) -> list:
    """Every bin that may hold a record overlapping [beg, end)."""
    end -= 1
    s, t, out = min_shift + 3 * depth, 0, []
    for l in range(depth + 1):
        out.extend(range(t + (beg >> s), t + (end >> s) + 1))
        s -= 3
        t += 1 << (3 * l)
    return out


@dataclass
class RefIndex:
    bins: dict = field(default_factory=dict)      # bin -> uint64[k, 2] chunks in file order
    linear: np.ndarray = None                     # BAI: uint64[n_intv], the smallest start offset per 16-kb window (0: unknown)
    loffset: dict = None                          # CSI: bin -> the smallest start offset of a record overlapping the bin
    meta: tuple = None                            # (off_beg, off_end, n_mapped, n_unmapped) or None


@dataclass
class BamIndex:
    refs: list
    n_no_coor: int = 0
    fmt: str = "bai"
    min_shift: int = 14
    depth: int = 5
    aux: bytes = b""
    ref_lens: list = None                         # known for an index built from a BAM (write_bai checks them)

    @property
    def n_ref(self) -> int:
        return len(self.refs)

    @property
    def mapped(self) -> int:
        """pysam's `AlignmentFile.mapped`: the mapped counts of the metadata bins, summed."""
        return sum(int(r.meta[2]) for r in self.refs if r.meta is not None)

    def contig_mapped(self, ref_id: int) -> int:
        """`get_index_statistics()[ref_id].mapped`."""
        m = self.refs[ref_id].meta
        return int(m[2]) if m is not None else 0

    def _min_off(self, r: RefIndex, beg: int) -> int:
        if r.loffset is None:
            lin = r.linear
            if lin is None or lin.shape[0] == 0:
                return 0
            w = beg >> 14
            return int(lin[w]) if w < lin.shape[0] else int(lin[-1])
        # CSI: the loffset of the first bin present at or before the window, level by level upwards (htslib hts_itr_query)
        b = ((1 << (3 * self.depth)) - 1) // 7 + (beg >> self.min_shift)
        while b:
            if b in r.loffset:
                return int(r.loffset[b])
            first = (((b - 1) >> 3) << 3) + 1
            b = b - 1 if b > first else (b - 1) >> 3
        return int(r.loffset.get(0, 0))

    def query(self, ref_id: int, beg: int = 0, end: int = None) -> np.ndarray:
        """uint64[k, 2]: disjoint ascending chunks; every record of `ref_id` with pos < end and endpos > beg starts inside one."""
        top = 1 << (self.min_shift + 3 * self.depth)
        beg = max(0, int(beg))
        end = top if end is None else min(int(end), top)
        if ref_id < 0 or ref_id >= len(self.refs) or beg >= end:
            return np.zeros((0, 2), np.uint64)
        r = self.refs[ref_id]
        lo = self._min_off(r, beg)
        parts = [r.bins[b] for b in reg2bins(beg, end, self.min_shift, self.depth) if b in r.bins]
        if not parts:
            return np.zeros((0, 2), np.uint64)
        c = np.concatenate(parts)
        c = c[c[:, 1] > np.uint64(lo)]
        if c.shape[0] == 0:
            return np.zeros((0, 2), np.uint64)
        c = c[np.argsort(c[:, 0], kind="stable")]
        out = [[int(c[0, 0]), int(c[0, 1])]]
        for a, b in c[1:].tolist():
            if a <= out[-1][1]:
                out[-1][1] = max(out[-1][1], b)
            else:
                out.append([a, b])
        return np.array(out, np.uint64)

    def _norm(self):
        def ref(r):
            lin = () if r.linear is None else tuple(r.linear.tolist())
            return (sorted((b, c.tolist()) for b, c in r.bins.items()), lin, None if r.loffset is None else sorted(r.loffset.items()),
                    None if r.meta is None else tuple(int(x) for x in r.meta))
        return [ref(r) for r in self.refs], int(self.n_no_coor), self.min_shift, self.depth

    def __eq__(self, other):
        return isinstance(other, BamIndex) and self._norm() == other._norm()


class _Reader:
    def __init__(self, data: bytes, what: str):
        self.d, self.p, self.what = data, 0, what

    def take(self, fmt: str, name: str):
        n = struct.calcsize(fmt)
        if self.p + n > len(self.d):
            raise ValueError(f"{self.what}: truncated in {name} (byte {self.p} of {len(self.d)})")
        v = struct.unpack_from(fmt, self.d, self.p)
        self.p += n
        return v[0] if len(v) == 1 else v

    def array(self, dtype, count: int, name: str):
        n = np.dtype(dtype).itemsize * count
        if count < 0 or self.p + n > len(self.d):
            raise ValueError(f"{self.what}: truncated in {name} ({count} entries at byte {self.p} of {len(self.d)})")
        a = np.frombuffer(self.d, dtype, count, self.p).copy()
        self.p += n
        return a


def _read_refs(rd: _Reader, n_ref: int, csi: bool, depth: int):
    mb = meta_bin(depth)
    refs = []
    for i in range(n_ref):
        r = RefIndex(loffset={} if csi else None)
        n_bin = rd.take("<i", f"n_bin of reference {i}")
        if n_bin < 0:
            raise ValueError(f"{rd.what}: n_bin of reference {i} is negative")
        for _ in range(n_bin):
            b = rd.take("<I", f"bin of reference {i}")
            loff = rd.take("<Q", f"loffset of bin {b}, reference {i}") if csi else None
            n_chunk = rd.take("<i", f"n_chunk of bin {b}, reference {i}")
            ch = rd.array("<u8", 2 * n_chunk, f"chunks of bin {b}, reference {i}").reshape(-1, 2)
            if b == mb:
                if n_chunk != 2:
                    raise ValueError(f"{rd.what}: n_chunk of the metadata bin of reference {i} is {n_chunk}, not 2")
                r.meta = (int(ch[0, 0]), int(ch[0, 1]), int(ch[1, 0]), int(ch[1, 1]))
                continue
            if b > mb:
                raise ValueError(f"{rd.what}: bin {b} of reference {i} is beyond the last bin of depth {depth}")
            if np.any(ch[:, 1] < ch[:, 0]):
                raise ValueError(f"{rd.what}: chunks of bin {b}, reference {i}: an end before its beginning")
            r.bins[b] = ch
            if csi:
                r.loffset[b] = loff
        if not csi:
            n_intv = rd.take("<i", f"n_intv of reference {i}")
            r.linear = rd.array("<u8", n_intv, f"ioffset of reference {i}")
        refs.append(r)
    return refs


def parse_index(data: bytes, what: str = "index") -> BamIndex:
    if data[:4] == b"BAI\x01":
        rd = _Reader(data, what)
        rd.p = 4
        n_ref = rd.take("<i", "n_ref")
        if n_ref < 0:
            raise ValueError(f"{what}: n_ref is negative")
        refs = _read_refs(rd, n_ref, False, 5)
        n_no_coor = rd.take("<Q", "n_no_coor") if rd.p < len(data) else 0      # (optional in the specification)
        return BamIndex(refs, int(n_no_coor), "bai")
    if data[:4] == b"\x1f\x8b\x08\x04":
        from . import bam
        raw = bam.bgzf_inflate(data)
        if raw[:4] != b"CSI\x01":
            raise ValueError(f"{what}: magic is neither BAI\\1 nor CSI\\1")
        rd = _Reader(raw, what)
        rd.p = 4
        min_shift, depth, l_aux = rd.take("<iii", "min_shift / depth / l_aux")
        if min_shift < 0 or depth < 0 or depth > 10 or l_aux < 0:
            raise ValueError(f"{what}: min_shift {min_shift} / depth {depth} / l_aux {l_aux} out of range")
        aux = rd.array("u1", l_aux, "aux").tobytes()
        n_ref = rd.take("<i", "n_ref")
        if n_ref < 0:
            raise ValueError(f"{what}: n_ref is negative")
        refs = _read_refs(rd, n_ref, True, depth)
        n_no_coor = rd.take("<Q", "n_no_coor") if rd.p < len(raw) else 0
        return BamIndex(refs, int(n_no_coor), "csi", min_shift, depth, aux)
    raise ValueError(f"{what}: magic is neither BAI\\1 nor CSI\\1")


def read_index(path: str) -> BamIndex:
    with open(path, "rb") as f:
        return parse_index(f.read(), path)


def find_index(bam_path: str):
    """`path.bai`, then `path` with `.bam` replaced by `.bai`, then `path.csi`; None if there is none."""
    cands = [bam_path + ".bai"]
    if bam_path.endswith(".bam"):
        cands.append(bam_path[:-4] + ".bai")
    cands.append(bam_path + ".csi")
    for c in cands:
        if os.path.exists(c):
            return c
    return None


def fill_linear(lin: np.ndarray) -> np.ndarray:
    """A window no record overlaps (U64_MAX) takes the offset of the next window that one does (htslib hts_idx_finish); the last
    window must be known.  Windows that hold 0 (older writers: unknown) stay as they are."""
    lin = np.array(lin, np.uint64)
    hole = lin == np.uint64(U64_MAX)
    if not hole.any():
        return lin
    if hole[-1]:
        raise ValueError("linear index ends in a window no record overlaps")
    nxt = np.where(hole, lin.shape[0], np.arange(lin.shape[0]))
    return lin[np.minimum.accumulate(nxt[::-1])[::-1]]


def bai_bytes(index: BamIndex) -> bytes:
    if index.min_shift != 14 or index.depth != 5:
        raise ValueError(f"BAI is min_shift 14 / depth 5; this index is {index.min_shift} / {index.depth}")
    for i, ln in enumerate(index.ref_lens or []):
        if int(ln) > 1 << 29:
            raise ValueError(f"BAI cannot hold reference {i} of {int(ln)} bases: its bins end at 2^29 (a CSI index can)")
    out = [b"BAI\x01", struct.pack("<i", index.n_ref)]
    for r in index.refs:
        out.append(struct.pack("<i", len(r.bins) + (1 if r.meta is not None else 0)))
        for b in sorted(r.bins):
            ch = np.ascontiguousarray(r.bins[b], "<u8")
            out += [struct.pack("<Ii", b, ch.shape[0]), ch.tobytes()]
        if r.meta is not None:
            out.append(struct.pack("<Ii4Q", meta_bin(5), 2, *[int(x) for x in r.meta]))
        if r.linear is not None:
            lin = np.array(r.linear, np.uint64)
        else:      # from a CSI: no windows are known, every query keeps all chunks of its bins
            lin = np.zeros(0, np.uint64)
        lin = fill_linear(lin)
        out += [struct.pack("<i", lin.shape[0]), lin.astype("<u8").tobytes()]
    out.append(struct.pack("<Q", int(index.n_no_coor)))
    return b"".join(out)


def write_bai(index: BamIndex, path: str) -> None:
    data = bai_bytes(index)
    with open(path, "wb") as f:
        f.write(data)


# ------------------------------------------------------------------------------------------------------------- CSI, written
CSI_META_LOFFSET = 0      # the loffset htslib stores with the metadata pseudo-bin (hts_idx_finish / update_loff: a bin beyond the real ones)


def csi_depth(max_ref_len: int, min_shift: int = 14) -> int:
    """The smallest depth with 2^(min_shift + 3 depth) >= max_ref_len + 256: htslib's rule (sam_index_build, tbx_index_build),
    5 for the human genome at min_shift 14.  A reference of a few bases gives 0; the device entry point takes 1 .. 10."""
    need, depth = int(max_ref_len) + 256, 0
    while need > 1 << (min_shift + 3 * depth):
        depth += 1
    return depth


def bin_first_window(bins, depth: int) -> np.ndarray:
    """int64[k]: the first min_shift window of every bin (htslib hts_bin_bot); `bins` are real bins of `depth` levels."""
    b = np.asarray(bins, np.int64)
    first = np.array([((1 << (3 * l)) - 1) // 7 for l in range(depth + 2)], np.int64)      # first bin of every level, and one past the last
    level = np.searchsorted(first, b, side="right") - 1
    return (b - first[level]) << (3 * (depth - level))


def csi_loffsets(bins, filled: np.ndarray, depth: int) -> dict:
    """bin -> loffset by htslib's update_loff.  `filled`: the window minima of the reference at min_shift granularity, cut behind
    the last known window, holes filled with the following window's value (`fill_linear`).  A bin takes the value at its first
    window, 0 if that window lies behind the array."""
    b = sorted(int(x) for x in bins)
    if not b:
        return {}
    w = bin_first_window(b, depth)
    inside = w < filled.shape[0]
    val = np.zeros(len(b), np.uint64)
    val[inside] = filled[w[inside]]
    return dict(zip(b, val.tolist()))


def csi_raw(index: BamIndex) -> bytes:
    """The inflated bytes of a CSIv1 file: magic, min_shift, depth, l_aux + aux, n_ref; per reference the bins in ascending order
    with loffset and chunks, the metadata pseudo-bin last; n_no_coor."""
    ms, depth = int(index.min_shift), int(index.depth)
    if ms < 0 or depth < 0 or depth > 10:
        raise ValueError(f"CSI: min_shift {ms} / depth {depth} out of range")
    mb = meta_bin(depth)
    aux = bytes(index.aux or b"")
    out = [b"CSI\x01", struct.pack("<iii", ms, depth, len(aux)), aux, struct.pack("<i", index.n_ref)]
    for i, r in enumerate(index.refs):
        if r.bins and r.loffset is None:
            raise ValueError(f"CSI: reference {i} has no loffset table (an index read from a BAI does not carry one)")
        out.append(struct.pack("<i", len(r.bins) + (1 if r.meta is not None else 0)))
        for b in sorted(r.bins):
            if b >= mb:
                raise ValueError(f"CSI: bin {b} of reference {i} is beyond the last bin of depth {depth}")
            ch = np.ascontiguousarray(r.bins[b], "<u8")
            out += [struct.pack("<IQi", b, int(r.loffset[b]), ch.shape[0]), ch.tobytes()]
        if r.meta is not None:
            out.append(struct.pack("<IQi4Q", mb, CSI_META_LOFFSET, 2, *[int(x) for x in r.meta]))
    out.append(struct.pack("<Q", int(index.n_no_coor)))
    return b"".join(out)


def csi_bytes(index: BamIndex, deflater=None) -> bytes:
    """A CSIv1 file: `csi_raw` as BGZF members of at most 0xff00 bytes and the EOF member, as htslib writes it.  The members come
    from the host's zlib; `deflater`: a `bgzfout.DeflateDevice` that compresses them on the GPU instead."""
    raw = csi_raw(index)
    if deflater is None:
        from . import bam
        return bam.bgzf_deflate(raw, 6)
    from . import bgzfout
    image, _ = deflater.compress(raw)
    return image + bgzfout.EOF_MEMBER


def write_csi(index: BamIndex, path: str, deflater=None) -> None:
    data = csi_bytes(index, deflater)
    with open(path, "wb") as f:
        f.write(data)
