"""Host side of signature extraction: BGZF/BAM container -> inflated alignment records for the GPU.

The reference reads alignments through pysam (`bam.fetch(contig, start, end)`, `leadprov.py:487`); the extraction
kernels (`csrc/snf_extract.hip`) instead take the INFLATED BAM alignment records of one contig as one byte blob plus
record offsets and parse CIGAR / tags / sequence on the GPU.  This module is the container layer in front of that:
BGZF block inflate (zlib), header parse, the record chain (each record starts with its `block_size`), the
overlap filter `fetch` applies, and the interning of read names / contig names to order-preserving ranks
(SoA convention, `sniffles_amd/soa.py`).  Pure I/O and bookkeeping; no signature logic lives here.
"""
from __future__ import annotations

import struct
import zlib
from dataclasses import dataclass

import numpy as np


def bgzf_inflate(data: bytes) -> bytes:
    """Concatenated BGZF blocks (gzip members with a BC extra field) -> raw BAM stream."""
    out = []
    p = 0
    n = len(data)
    while p < n:
        if data[p:p + 4] != b"\x1f\x8b\x08\x04":
            raise ValueError(f"not a BGZF block at byte {p}")
        xlen = struct.unpack_from("<H", data, p + 10)[0]
        q = p + 12
        bsize = None
        while q < p + 12 + xlen:
            si1, si2, slen = data[q], data[q + 1], struct.unpack_from("<H", data, q + 2)[0]
            if si1 == 66 and si2 == 67 and slen == 2:
                bsize = struct.unpack_from("<H", data, q + 4)[0] + 1
            q += 4 + slen
        if bsize is None:
            raise ValueError("BGZF block without BC field")
        cdata = data[p + 12 + xlen:p + bsize - 8]
        isize = struct.unpack_from("<I", data, p + bsize - 4)[0]
        raw = zlib.decompress(cdata, -15) if isize else b""
        if len(raw) != isize:
            raise ValueError("BGZF block size mismatch")
        out.append(raw)
        p += bsize
    return b"".join(out)


def bgzf_deflate(raw: bytes, level: int = 1) -> bytes:
    """Raw BAM stream -> BGZF blocks (+ the empty EOF block); the inverse of `bgzf_inflate` (tests, synthetic inputs)."""
    out = []
    for p in list(range(0, len(raw), 0xff00)) + [None]:
        chunk = b"" if p is None else raw[p:p + 0xff00]
        co = zlib.compressobj(level, zlib.DEFLATED, -15)
        cdata = co.compress(chunk) + co.flush()
        bsize = len(cdata) + 25
        out.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", bsize) + cdata +
                   struct.pack("<II", zlib.crc32(chunk) & 0xffffffff, len(chunk)))
    return b"".join(out)


def bam_stream(ref_names, ref_lens, records, header_text: str = "@HD\tVN:1.6\tSO:coordinate\n") -> bytes:
    """Header + records as an inflated BAM stream (SAM/BAM spec 4.2)."""
    text = header_text.encode("ascii")
    parts = [b"BAM\x01", struct.pack("<i", len(text)), text, struct.pack("<i", len(ref_names))]
    for name, ln in zip(ref_names, ref_lens):
        nm = name.encode("ascii") + b"\0"
        parts += [struct.pack("<i", len(nm)), nm, struct.pack("<i", int(ln))]
    return b"".join(parts) + b"".join(records)


@dataclass
class BamRecords:
    """Inflated alignment records of a BAM stream (all contigs, file order)."""
    ref_names: list          # header reference names, index = BAM refID
    ref_lens: list
    blob: np.ndarray         # uint8, the concatenated records, each starting with its block_size field
    rec_off: np.ndarray      # int64[n+1] byte offset of every record in blob
    ref_id: np.ndarray       # int32[n]
    pos: np.ndarray          # int32[n]

    @property
    def n(self) -> int:
        return int(self.rec_off.shape[0] - 1)

    def qname(self, i: int) -> str:
        o = int(self.rec_off[i])
        l_read_name = int(self.blob[o + 12])
        return bytes(self.blob[o + 36:o + 36 + l_read_name - 1]).decode("ascii")

    def select(self, idx) -> "BamRecords":
        idx = np.asarray(idx, np.int64)
        lens = (self.rec_off[idx + 1] - self.rec_off[idx]).astype(np.int64)
        off = np.zeros(idx.shape[0] + 1, np.int64)
        np.cumsum(lens, out=off[1:])
        # consecutive records are one slice (a contig of a coordinate-sorted BAM is a single run)
        if idx.shape[0]:
            brk = np.nonzero(np.diff(idx) != 1)[0] + 1
            starts = np.r_[0, brk]
            ends = np.r_[brk, idx.shape[0]]
            parts = [self.blob[int(self.rec_off[idx[a]]):int(self.rec_off[idx[b - 1] + 1])] for a, b in zip(starts.tolist(), ends.tolist())]
            blob = np.concatenate(parts) if len(parts) > 1 else parts[0].copy()
        else:
            blob = np.zeros(0, np.uint8)
        return BamRecords(self.ref_names, self.ref_lens, blob, off, self.ref_id[idx].copy(), self.pos[idx].copy())


def parse_bam(raw: bytes) -> BamRecords:
    """Raw (inflated) BAM stream -> header + record table."""
    if raw[:4] != b"BAM\x01":
        raise ValueError("not a BAM stream")
    l_text = struct.unpack_from("<i", raw, 4)[0]
    p = 8 + l_text
    n_ref = struct.unpack_from("<i", raw, p)[0]
    p += 4
    names, lens = [], []
    for _ in range(n_ref):
        l_name = struct.unpack_from("<i", raw, p)[0]
        names.append(raw[p + 4:p + 4 + l_name - 1].decode("ascii"))
        lens.append(struct.unpack_from("<i", raw, p + 4 + l_name)[0])
        p += 8 + l_name
    start = p
    offs, rid, pos = [0], [], []
    n = len(raw)
    while p < n:
        bs = struct.unpack_from("<i", raw, p)[0]
        if bs < 32 or p + 4 + bs > n:
            raise ValueError(f"truncated BAM record at byte {p}")
        r, ps = struct.unpack_from("<ii", raw, p + 4)
        rid.append(r)
        pos.append(ps)
        p += 4 + bs
        offs.append(p - start)
    blob = np.frombuffer(raw, np.uint8, count=n - start, offset=start).copy()
    return BamRecords(names, lens, blob, np.array(offs, np.int64), np.array(rid, np.int32), np.array(pos, np.int32))


def read_bam(path: str) -> BamRecords:
    with open(path, "rb") as f:
        return parse_bam(bgzf_inflate(f.read()))


def records_from_list(ref_names, ref_lens, records) -> BamRecords:
    """Build the record table from a list of raw record byte strings (each including block_size)."""
    offs = np.zeros(len(records) + 1, np.int64)
    np.cumsum([len(r) for r in records], out=offs[1:])
    blob = np.frombuffer(b"".join(records), np.uint8).copy() if records else np.zeros(0, np.uint8)
    rid = np.array([struct.unpack_from("<i", r, 4)[0] for r in records], np.int32)
    pos = np.array([struct.unpack_from("<i", r, 8)[0] for r in records], np.int32)
    return BamRecords(list(ref_names), list(ref_lens), blob, offs, rid, pos)


def record_flags(recs) -> np.ndarray:
    """FLAG of every record (uint16 at byte 18 of the record, block_size included)."""
    if isinstance(recs, DeviceBamRecords):
        return recs.flags
    o = recs.rec_off[:-1]
    return recs.blob[o + 18].astype(np.uint16) | (recs.blob[o + 19].astype(np.uint16) << 8)


def contig_records(recs: BamRecords, contig: str) -> BamRecords:
    """The mapped records of one contig in file order (what `bam.fetch(contig)` iterates).  A region fetch
    additionally drops records that do not overlap the region; the kernel applies the reference's own
    `reference_start` window (leadprov.py:500), which is the stricter test, so contig granularity is enough."""
    if isinstance(recs, DeviceBamRecords):
        return recs.contig_view(contig)
    rid = recs.ref_names.index(contig)
    keep = np.nonzero((recs.ref_id == rid) & ((record_flags(recs) & 0x4) == 0))[0] if recs.n else np.zeros(0, np.int64)
    return recs.select(keep)


def fnv1a64(b: bytes) -> int:
    h = 0xcbf29ce484222325
    for c in b:
        h = ((h ^ c) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def contig_tables(ref_names):
    """Contig names -> (sorted hash table, rank of the hashed name, rank per BAM refID, names in rank order).
    Rank = position in Python str order (SoA convention for mate contigs)."""
    order = sorted(range(len(ref_names)), key=lambda i: ref_names[i])
    rank_of_refid = np.zeros(len(ref_names), np.int32)
    for r, i in enumerate(order):
        rank_of_refid[i] = r
    hashes = np.array([fnv1a64(nm.encode("ascii")) for nm in ref_names], np.uint64)
    if len(set(hashes.tolist())) != len(ref_names):
        raise ValueError("contig name hash collision (or duplicate names) in the BAM header")
    ho = np.argsort(hashes, kind="stable")
    return hashes[ho].copy(), rank_of_refid[ho].copy(), rank_of_refid, [ref_names[i] for i in order]


def qname_ranks(recs: BamRecords):
    """Read names of the records -> (rank per record in Python str order, sorted distinct names).  Names are ASCII
    (SAM spec), so byte order of the NUL-padded names is Python's str order; one `np.unique` over a fixed-width view
    replaces a Python loop over millions of records."""
    if isinstance(recs, DeviceBamRecords):
        return recs.qname_ranks()
    n = recs.n
    if n == 0:
        return np.zeros(0, np.uint32), []
    o = recs.rec_off[:-1]
    ln = recs.blob[o + 12].astype(np.int64) - 1                    # l_read_name counts the terminating NUL
    width = int(ln.max()) if n else 0
    if width <= 0:
        return np.zeros(n, np.uint32), [""]
    col = np.arange(width, dtype=np.int64)
    idx = (o + 36)[:, None] + col[None, :]
    mat = np.where(col[None, :] < ln[:, None], recs.blob[np.minimum(idx, recs.blob.shape[0] - 1)], 0).astype(np.uint8)
    keys = np.ascontiguousarray(mat).view(f"S{width}").reshape(n)
    uniq, inv = np.unique(keys, return_inverse=True)
    return inv.astype(np.uint32), [u.decode("ascii") for u in uniq.tolist()]


# ---------------------------------------------------------------------------------- the same container layer on the device
def bgzf_members(data: bytes) -> np.ndarray:
    """The host-side hop over the member headers (BSIZE): one row per BGZF member - offset and length of its deflate payload,
    ISIZE and the offset of its output (the exclusive sum of ISIZE) - `abi.BGZF_MEMBER_DTYPE`, what `snf_bgzf_inflate` takes.
    Raises what `bgzf_inflate` raises for a bad magic or a missing BC field."""
    from .abi import BGZF_MEMBER_DTYPE
    rows = []
    p, n, out = 0, len(data), 0
    while p < n:
        if data[p:p + 4] != b"\x1f\x8b\x08\x04":
            raise ValueError(f"not a BGZF block at byte {p}")
        xlen = struct.unpack_from("<H", data, p + 10)[0]
        q = p + 12
        bsize = None
        while q < p + 12 + xlen:
            si1, si2, slen = data[q], data[q + 1], struct.unpack_from("<H", data, q + 2)[0]
            if si1 == 66 and si2 == 67 and slen == 2:
                bsize = struct.unpack_from("<H", data, q + 4)[0] + 1
            q += 4 + slen
        if bsize is None:
            raise ValueError("BGZF block without BC field")
        if p + bsize > n or bsize < 12 + xlen + 8:
            raise ValueError(f"truncated BGZF block at byte {p}")
        isize = struct.unpack_from("<I", data, p + bsize - 4)[0]
        rows.append((p + 12 + xlen, out, bsize - 8 - 12 - xlen, isize))
        out += isize
        p += bsize
    return np.array(rows, BGZF_MEMBER_DTYPE) if rows else np.zeros(0, BGZF_MEMBER_DTYPE)


def _bam_header(raw: bytes):
    """(ref_names, ref_lens, header length) of an inflated BAM stream, or None while `raw` does not hold the whole header."""
    if len(raw) >= 4 and raw[:4] != b"BAM\x01":
        raise ValueError("not a BAM stream")
    if len(raw) < 8:
        return None
    p = 8 + struct.unpack_from("<i", raw, 4)[0]
    if len(raw) < p + 4:
        return None
    n_ref = struct.unpack_from("<i", raw, p)[0]
    p += 4
    names, lens = [], []
    for _ in range(n_ref):
        if len(raw) < p + 4:
            return None
        l_name = struct.unpack_from("<i", raw, p)[0]
        if len(raw) < p + 8 + l_name:
            return None
        names.append(raw[p + 4:p + 4 + l_name - 1].decode("ascii"))
        lens.append(struct.unpack_from("<i", raw, p + 4 + l_name)[0])
        p += 8 + l_name
    return names, lens, p


class BgzfDevice:
    """One `snf_bgzf_t`: inflates runs of BGZF members on the GPU and chains the BAM records (csrc/snf_bgzf.h).  The inflated
    stream and the record offsets stay in HBM until the next `inflate` / `close`."""

    def __init__(self, device: int = 0):
        import ctypes as C
        from . import lib as L
        self.lib = L.load()
        self._err = L.SnifflesAmdError
        self.device = device
        self._h = C.c_void_p()
        self._check(self.lib.snf_bgzf_create(device, C.byref(self._h)))

    def _check(self, rc):
        if rc != 0:
            raise self._err(self.lib.snf_bgzf_last_error().decode("utf-8", "replace"))

    def inflate(self, data, members: np.ndarray, carry=None, header_len: int = 0) -> dict:
        """`data`: the compressed bytes `members` (bgzf_members) points into; `carry`: the carry a previous run returned, or
        None for the first run of a stream whose BAM header is `header_len` bytes long.  Returns the host tables, the final
        carry, the device pointers and the kernel times."""
        import ctypes as C
        from . import abi
        buf = np.frombuffer(data, np.uint8)
        mem = np.ascontiguousarray(members, abi.BGZF_MEMBER_DTYPE)
        if carry is None:
            carry = abi.snf_bam_carry_t(skip=int(header_len), count=0, stream_pos=0, origin=int(header_len), n_part=0)
        self._check(self.lib.snf_bgzf_inflate(self._h, buf.ctypes.data if buf.shape[0] else None, int(buf.shape[0]),
                                              mem.ctypes.data if mem.shape[0] else None, int(mem.shape[0]), C.byref(carry)))
        r = abi.snf_bgzf_result_t()
        self._check(self.lib.snf_bgzf_result(self._h, C.byref(r)))
        n, w = int(r.n_records), int(r.name_width)
        out_carry = abi.snf_bam_carry_t.from_buffer_copy(r.carry)
        return dict(stream_len=int(r.stream_len), n=n, name_width=w,
                    rec_off=np.ctypeslib.as_array(r.rec_off, shape=(n + 1,)).copy(),
                    heads=(np.ctypeslib.as_array(r.heads, shape=(n * 6,)).copy() if n else np.zeros(0, np.uint32)).reshape(n, 6),
                    names=(np.ctypeslib.as_array(r.names, shape=(n * w,)).copy() if n * w else np.zeros(0, np.uint8)).reshape(n, w),
                    carry=out_carry, d_stream=int(r.d_stream or 0), d_rec_off=int(r.d_rec_off or 0), device=int(r.device),
                    ms_inflate=float(r.ms_inflate), ms_chain=float(r.ms_chain))

    def read_stream(self, off: int, length: int) -> bytes:
        """Inflated bytes of the last run, copied back to the host (tests)."""
        out = np.zeros(max(1, int(length)), np.uint8)
        self._check(self.lib.snf_bgzf_read_stream(self._h, int(off), int(length), out.ctypes.data))
        return out[:int(length)].tobytes()

    def close(self):
        if self._h:
            self.lib.snf_bgzf_destroy(self._h)
            self._h.value = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@dataclass
class DeviceBamRecords:
    """`BamRecords` whose blob stays in HBM: the host columns come from the two small tables the device hands back (the first
    six dwords and the read name of every record).  `handle` owns the device memory and must outlive every extraction."""
    ref_names: list
    ref_lens: list
    rec_off: np.ndarray      # int64[n+1], relative to the first record of the FILE (also for a contig view)
    ref_id: np.ndarray       # int32[n]
    pos: np.ndarray          # int32[n]
    flags: np.ndarray        # uint16[n]
    heads: np.ndarray        # uint32[n, 6]
    names: np.ndarray        # uint8[n, width], NUL-padded
    handle: BgzfDevice
    d_blob: int              # device address of the file's first record
    blob_len: int
    d_rec_off: int           # device address of rec_off[0] of this view
    device: int
    keep: np.ndarray = None  # contig view: the records `contig_records` keeps on the host (mapped, of the contig)
    info: dict = None        # read_bam_device: kernel times and byte counts

    @property
    def n(self) -> int:
        return int(self.rec_off.shape[0] - 1)

    def qname(self, i: int) -> str:
        return self.names[i].tobytes().split(b"\0", 1)[0].decode("ascii")

    def qname_ranks(self):
        """`qname_ranks` over the name table (records a contig view does not keep get rank 0: the extraction skips them)."""
        n = self.n
        sel = np.arange(n) if self.keep is None else np.nonzero(self.keep)[0]
        if sel.shape[0] == 0:
            return np.zeros(n, np.uint32), []
        ln = (self.heads[sel, 3] & 0xff).astype(np.int64) - 1
        width = int(ln.max())
        rank = np.zeros(n, np.uint32)
        if width <= 0:
            return rank, [""]
        mat = np.ascontiguousarray(self.names[sel, :width])
        keys = mat.view(f"S{width}").reshape(sel.shape[0])
        uniq, inv = np.unique(keys, return_inverse=True)
        rank[sel] = inv.astype(np.uint32)
        return rank, [u.decode("ascii") for u in uniq.tolist()]

    def contig_view(self, contig: str) -> "DeviceBamRecords":
        """The contiguous record range of `contig` (coordinate-sorted file), no copy: the extraction skips the unmapped records."""
        rid = self.ref_names.index(contig)
        idx = np.nonzero(self.ref_id == rid)[0]
        if idx.shape[0] and int(idx[-1]) - int(idx[0]) + 1 != idx.shape[0]:
            raise ValueError(f"the records of contig {contig} are not one run: the file is not coordinate-sorted "
                             "(read_bam serves such a file)")
        lo, hi = (int(idx[0]), int(idx[-1]) + 1) if idx.shape[0] else (0, 0)
        sl = slice(lo, hi)
        keep = (self.ref_id[sl] == rid) & ((self.flags[sl] & 0x4) == 0)
        return DeviceBamRecords(self.ref_names, self.ref_lens, self.rec_off[lo:hi + 1], self.ref_id[sl], self.pos[sl], self.flags[sl],
                                np.ascontiguousarray(self.heads[sl]), self.names[sl], self.handle, self.d_blob, self.blob_len,
                                self.d_rec_off + 8 * lo, self.device, keep=keep, info=self.info)


def read_bam_device(path: str, device: int = 0) -> DeviceBamRecords:
    """`read_bam` with the inflate and the record chain on the GPU: the compressed file bytes go over PCIe, the inflated
    records stay in HBM.  The host only hops through the member headers and parses the BAM header (zlib over the leading
    members).  Refuses a file whose inflated size does not fit the device."""
    with open(path, "rb") as f:
        data = f.read()
    return bam_device(data, device)


def bam_device(data: bytes, device: int = 0) -> DeviceBamRecords:
    members = bgzf_members(data)
    raw, hdr = b"", None
    for m in members:
        a, ln = int(m["payload_off"]), int(m["payload_len"])
        part = zlib.decompress(data[a:a + ln], -15) if m["isize"] else b""
        if len(part) != int(m["isize"]):
            raise ValueError("BGZF block size mismatch")
        raw += part
        hdr = _bam_header(raw)
        if hdr is not None:
            break
    if hdr is None:
        raise ValueError("not a BAM stream")
    names, lens, hlen = hdr
    z = BgzfDevice(device)
    try:
        try:
            r = z.inflate(data, members, header_len=hlen)
        except z._err as e:
            if str(e).startswith("truncated BAM record"):
                raise ValueError(str(e)) from None
            raise
        c = r["carry"]
        if c.skip or c.n_part:      # the chain does not end at the end of the stream
            at = hlen + int(r["rec_off"][r["n"] - 1]) if c.skip else r["stream_len"] - int(c.n_part)
            raise ValueError(f"truncated BAM record at byte {at}")
    except Exception:
        z.close()
        raise
    heads = r["heads"]
    info = dict(ms_inflate=r["ms_inflate"], ms_chain=r["ms_chain"], compressed_bytes=len(data), stream_len=r["stream_len"],
                bytes_h2d=len(data) + members.nbytes, bytes_d2h=r["rec_off"].nbytes + heads.nbytes + r["names"].nbytes)
    return DeviceBamRecords(names, lens, r["rec_off"], heads[:, 1].astype(np.uint32).view(np.int32).copy(),
                            heads[:, 2].astype(np.uint32).view(np.int32).copy(), (heads[:, 4] >> 16).astype(np.uint16), heads, r["names"], z,
                            r["d_stream"] + hlen, r["stream_len"] - hlen, r["d_rec_off"], r["device"], info=info)
