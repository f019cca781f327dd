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
    if isinstance(recs, IndexedBam):
        return recs.fetch_device(contig)
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
def bgzf_members(data: bytes, start: int = 0, stop: int = None, max_bytes: int = None) -> np.ndarray:
    """The host-side hop over the member headers (BSIZE): one row per BGZF member - offset and length of its deflate payload,
    ISIZE and the offset of its output (the exclusive sum of ISIZE) - `abi.BGZF_MEMBER_DTYPE`, what `snf_bgzf_inflate` takes.
    Raises what `bgzf_inflate` raises for a bad magic or a missing BC field.
    `start` / `stop`: only the members that begin in [start, stop) of `data` (a memory-mapped file is touched there only);
    `max_bytes`: at least one member, then as many as stay within that many compressed bytes - and the empty members that follow
    them (the virtual offset of a record that ends at a member border names the next member that holds a byte)."""
    from .abi import BGZF_MEMBER_DTYPE
    rows = []
    p, n, out = int(start), len(data) if stop is None else min(int(stop), len(data)), 0
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
        if p + bsize > len(data) or bsize < 12 + xlen + 8:
            raise ValueError(f"truncated BGZF block at byte {p}")
        isize = struct.unpack_from("<I", data, p + bsize - 4)[0]
        if max_bytes is not None and rows and isize and p + bsize - int(start) > max_bytes:
            break
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

    def bai_run(self, member_file_off: np.ndarray, win_off: np.ndarray, carry=None) -> dict:
        """The index tables of the run the last `inflate` left in HBM (csrc/snf_bamindex.h).  `member_file_off`: n_members + 1
        (`member_file_offsets`); `win_off`: the first 16-kb window of every reference in one table, n_ref + 1; `carry`: the
        `snf_bai_carry_t` the run before returned, or None at the start of the file."""
        return self._index_run(member_file_off, win_off, carry, None)

    def csi_run(self, member_file_off: np.ndarray, win_off: np.ndarray, carry=None, min_shift: int = 14, depth: int = 5) -> dict:
        """`bai_run` for a CSI of `depth` levels over windows of 2^min_shift bases (snf_csi_run): the bins follow
        `bamindex.reg2bin(pos, end, min_shift, depth)`, `win_off` (`window_offsets(lens, min_shift)`), `win_index` and `win_min`
        count windows of that size.  Parameters the entry point does not take are a ValueError; the handle stays usable."""
        return self._index_run(member_file_off, win_off, carry, (int(min_shift), int(depth)))

    def _index_run(self, member_file_off, win_off, carry, scheme) -> dict:
        import ctypes as C
        from . import abi
        foff = np.ascontiguousarray(member_file_off, np.int64)
        wo = np.ascontiguousarray(win_off, np.int64)
        cin = abi.snf_bai_carry_t() if carry is None else abi.snf_bai_carry_t.from_buffer_copy(carry)
        cin.n_ref = int(wo.shape[0] - 1)
        cin.win_off = wo.ctypes.data_as(C.POINTER(C.c_int64))
        r = abi.snf_bai_run_result_t()
        if scheme is None:
            rc = self.lib.snf_bai_run(self._h, foff.ctypes.data, C.byref(cin), C.byref(r))
        else:
            rc = self.lib.snf_csi_run(self._h, foff.ctypes.data, C.byref(cin), scheme[0], scheme[1], C.byref(r))
        if rc != 0:
            msg = self.lib.snf_bai_last_error().decode("utf-8", "replace")
            if msg.startswith(("truncated BAM record", "BAM not coordinate-sorted", "snf_csi_run: min_shift")):
                raise ValueError(msg)
            raise self._err(msg)
        n, k, w = int(r.n_records), int(r.n_runs), int(r.n_windows)
        col = lambda ptr, cnt, dt: np.ctypeslib.as_array(ptr, shape=(cnt,)).copy() if cnt else np.zeros(0, dt)
        out_carry = abi.snf_bai_carry_t.from_buffer_copy(r.carry)
        out_carry.win_off = None
        return dict(n=n, end=col(r.end, n, np.int64), bin=col(r.bin, n, np.uint32), vbeg=col(r.vbeg, n, np.uint64), vend=col(r.vend, n, np.uint64),
                    runs=col(r.runs, 3 * k, np.uint64).reshape(k, 3), head_n=int(r.head_n), head_end=int(r.head_end),
                    win_index=col(r.win_index, w, np.int64), win_min=col(r.win_min, w, np.uint64), carry=out_carry,
                    ms_span=float(r.ms_span), ms_linear=float(r.ms_linear), ms_runs=float(r.ms_runs))

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
    owns_handle: bool = False  # `IndexedBam.fetch_device`: these records are all their handle holds, `close` frees it

    @property
    def n(self) -> int:
        return int(self.rec_off.shape[0] - 1)

    def qname(self, i: int) -> str:
        return self.names[i].tobytes().split(b"\0", 1)[0].decode("ascii")

    def close(self):
        """Free the device memory behind the records, if they own it (`IndexedBam.fetch_device`).  A table of `read_bam_device`
        and its contig views share one handle, which stays with whoever loaded the file (`recs.handle.close()`): nothing happens."""
        if self.owns_handle:
            self.handle.close()

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


def member_file_offsets(members: np.ndarray, start: int = 0) -> np.ndarray:
    """int64[n + 1]: the file offset of every member of a `bgzf_members` table that begins at `start`, and of the byte behind the last."""
    off = np.empty(members.shape[0] + 1, np.int64)
    off[0] = int(start)
    off[1:] = members["payload_off"] + members["payload_len"].astype(np.int64) + 8
    return off


def leading_header(data):
    """(ref_names, ref_lens, header length) of a BGZF-compressed BAM: zlib over the leading members only (`data` may be a memory map)."""
    raw, hdr, p = b"", None, 0
    while hdr is None and p < len(data):
        m = bgzf_members(data, p, p + 1)[0]
        a, ln = int(m["payload_off"]), int(m["payload_len"])
        part = zlib.decompress(data[a:a + ln], -15) if m["isize"] else b""
        if len(part) != int(m["isize"]):
            raise ValueError("BGZF block size mismatch")
        raw += part
        hdr = _bam_header(raw)
        p = a + ln + 8
    if hdr is None:
        raise ValueError("not a BAM stream")
    return hdr


def bam_device(data: bytes, device: int = 0) -> DeviceBamRecords:
    members = bgzf_members(data)
    hdr = leading_header(data)
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


# ------------------------------------------------------------------------------------------------- indexed access
def window_offsets(ref_lens, min_shift: int = 14) -> np.ndarray:
    """int64[n_ref + 1]: the first window of 2^min_shift bases (16 kb) of every reference in one table (a reference of no bases
    has one window)."""
    off = np.zeros(len(ref_lens) + 1, np.int64)
    np.cumsum([((max(int(n), 1) - 1) >> min_shift) + 1 for n in ref_lens], out=off[1:])
    return off


def _map_file(path: str):
    import mmap
    import os
    if os.path.getsize(path) == 0:
        raise ValueError("not a BAM stream")
    with open(path, "rb") as f:
        return mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)


class _IndexTables:
    """What the runs of `index_bam` add up to: chunks per (reference, bin) in file order, the window minima, the counts.
    `scheme`: None for a BAI, (min_shift, depth) for a CSI - the windows are then 2^min_shift bases and `finish` turns the
    minima into the bins' loffset values."""

    def __init__(self, ref_lens, scheme=None):
        from . import bamindex
        self.ref_lens = [int(x) for x in ref_lens]
        self.scheme = scheme
        n_ref = len(self.ref_lens)
        self.win_off = window_offsets(self.ref_lens, 14 if scheme is None else scheme[0])
        self.lin = np.full(int(self.win_off[-1]), bamindex.U64_MAX, np.uint64)
        self.chunks = {}
        self.mapped, self.unmapped = np.zeros(n_ref, np.int64), np.zeros(n_ref, np.int64)
        self.off_beg, self.off_end = [None] * n_ref, [None] * n_ref
        self.n_no_coor = 0
        self.last_key = None      # (reference, bin) of the last placed record so far: the chunk a run's leading records may continue

    def add_run(self, b: dict, heads: np.ndarray):
        """`b`: what `BgzfDevice.bai_run` returned; `heads`: the heads of the records it indexed."""
        n_ref = len(self.ref_lens)
        if b["head_n"] and self.last_key is not None:
            self.chunks[self.last_key][-1][1] = b["head_end"]
        for key, beg, end in b["runs"].tolist():
            self.chunks.setdefault((key >> 32, key & 0xffffffff), []).append([beg, end])
        if b["win_index"].shape[0]:
            self.lin[b["win_index"]] = np.minimum(self.lin[b["win_index"]], b["win_min"])
        ref = heads[:, 1].astype(np.uint32).view(np.int32)
        placed = ref >= 0
        is_un = ((heads[:, 4] >> 16) & 0x4) != 0
        self.n_no_coor += int((~placed).sum())
        if placed.any():
            self.mapped += np.bincount(ref[placed & ~is_un], minlength=n_ref)[:n_ref]
            self.unmapped += np.bincount(ref[placed & is_un], minlength=n_ref)[:n_ref]
            pi = np.nonzero(placed)[0]
            change = ref[pi][1:] != ref[pi][:-1]
            for i in pi[np.r_[True, change]].tolist():      # the first record of every reference in this run
                if self.off_beg[int(ref[i])] is None:
                    self.off_beg[int(ref[i])] = int(b["vbeg"][i])
            for i in pi[np.r_[change, True]].tolist():      # ... and the last
                self.off_end[int(ref[i])] = int(b["vend"][i])
        c = b["carry"]
        self.last_key = (int(c.prev_ref), int(c.prev_bin)) if c.have_prev and c.prev_ref >= 0 else None

    def finish(self):
        from . import bamindex
        refs = []
        for i in range(len(self.ref_lens)):
            seg = self.lin[int(self.win_off[i]):int(self.win_off[i + 1])]
            known = np.nonzero(seg != np.uint64(bamindex.U64_MAX))[0]
            seg = bamindex.fill_linear(seg[:int(known[-1]) + 1]) if known.shape[0] else np.zeros(0, np.uint64)
            bins = {bn: np.array(ch, np.uint64).reshape(-1, 2) for (rf, bn), ch in self.chunks.items() if rf == i}
            meta = (self.off_beg[i], self.off_end[i], int(self.mapped[i]), int(self.unmapped[i])) if self.off_beg[i] is not None else None
            if self.scheme is None:
                refs.append(bamindex.RefIndex(bins=bins, linear=seg, meta=meta))
            else:
                refs.append(bamindex.RefIndex(bins=bins, loffset=bamindex.csi_loffsets(bins, seg, self.scheme[1]), meta=meta))
        if self.scheme is None:
            return bamindex.BamIndex(refs, self.n_no_coor, "bai", ref_lens=self.ref_lens)
        return bamindex.BamIndex(refs, self.n_no_coor, "csi", self.scheme[0], self.scheme[1], ref_lens=self.ref_lens)


def _next_run(r: dict, n_use: int, members: np.ndarray, foff: np.ndarray, carry, count: int):
    """Where the run behind this one starts: (file offset, chain carry, inflated bytes this run is done with).  `r`: the inflate's
    result for `members` (file offsets `foff`), of whose records the first `n_use` are whole; `carry`: what the run started from.
    A run that ends on a record border is followed by the next member; one that cuts a record - inside its data (carry.skip) or
    inside its block_size field (carry.n_part) - by the member that holds the record's first byte, `skip` = its offset in there."""
    from . import abi
    c, origin = r["carry"], int(carry.origin)
    if not (c.skip or c.n_part):
        return int(foff[-1]), abi.snf_bam_carry_t(skip=0, count=count, stream_pos=int(c.stream_pos), origin=origin, n_part=0), r["stream_len"]
    p = (int(r["rec_off"][n_use]) + origin - int(carry.stream_pos)) if c.skip else r["stream_len"] - int(c.n_part)      # in this run's stream
    m = int(np.searchsorted(members["out_off"], p, side="right")) - 1                                               # (never an empty member)
    at = int(members["out_off"][m])
    return int(foff[m]), abi.snf_bam_carry_t(skip=p - at, count=count, stream_pos=int(carry.stream_pos) + at, origin=origin, n_part=0), at


def index_bam(path: str, out: str = None, device: int = 0, run_bytes: int = 256 << 20, stats: dict = None, fmt: str = "bai", min_shift: int = 14):
    """The BAI (`fmt="bai"`) or CSI (`fmt="csi"`) of a coordinate-sorted BAM, built on the GPU (csrc/snf_bamindex.h); written to
    `out` if given.  A CSI has windows of 2^min_shift bases and as many levels as the longest reference of the header needs
    (`bamindex.csi_depth`, at least 1): it holds references beyond 2^29 bases, which a BAI cannot.  The file is
    memory-mapped and goes through in runs of members of at most `run_bytes` compressed bytes: `BgzfDevice.inflate`, then
    `BgzfDevice.bai_run`; the host merges the tables of the runs (`_IndexTables`).  A run usually ends inside a record: that record
    is left out of the run and the next run starts at the member that holds its first byte (`_next_run`); a record larger than a
    run grows the run.  Refuses what htslib refuses: a file that is not coordinate-sorted (ValueError, naming the first offending
    record).  `stats`: filled with the number of runs, the kernel times and the byte counts."""
    from . import abi, bamindex
    if fmt not in ("bai", "csi"):
        raise ValueError(f"index_bam: fmt {fmt!r} is neither 'bai' nor 'csi'")
    if fmt == "csi" and not abi.CSI_MIN_SHIFT[0] <= int(min_shift) <= abi.CSI_MIN_SHIFT[1]:
        raise ValueError(f"index_bam: min_shift {min_shift} outside {abi.CSI_MIN_SHIFT[0]} .. {abi.CSI_MIN_SHIFT[1]}")
    data = _map_file(path)
    z = None
    try:
        names, lens, hlen = leading_header(data)
        size = len(data)
        scheme = None if fmt == "bai" else (int(min_shift), max(1, bamindex.csi_depth(max([int(x) for x in lens] + [0]), int(min_shift))))
        tables = _IndexTables(lens, scheme)
        z = BgzfDevice(device)
        fo, budget = 0, max(1, int(run_bytes))
        carry = abi.snf_bam_carry_t(skip=hlen, count=0, stream_pos=0, origin=hlen, n_part=0)
        bcarry = None
        info = dict(runs=0, ms_inflate=0.0, ms_chain=0.0, ms_span=0.0, ms_linear=0.0, ms_runs=0.0, stream_bytes=0, peak_stream_len=0,
                    bytes_h2d=0)
        while fo < size:
            members = bgzf_members(data, fo, max_bytes=budget)
            foff = member_file_offsets(members, fo)
            stop = int(foff[-1])
            rel = members.copy()
            rel["payload_off"] -= fo
            try:
                r = z.inflate(memoryview(data)[fo:stop], rel, carry=carry)
            except z._err as e:
                if str(e).startswith("truncated BAM record"):
                    raise ValueError(str(e)) from None
                raise
            c = r["carry"]
            cut = bool(c.skip or c.n_part)
            if cut and stop >= size:                  # the chain does not end at the end of the stream
                at = hlen + int(r["rec_off"][r["n"] - 1]) if c.skip else int(carry.stream_pos) + r["stream_len"] - int(c.n_part)
                raise ValueError(f"truncated BAM record at byte {at}")
            n_use = r["n"] - (1 if c.skip and r["n"] else 0)
            if cut and n_use == 0:                    # not one whole record (or the header) in this run: a longer one from the same place
                budget *= 2
                continue
            b = z.bai_run(foff, tables.win_off, bcarry) if scheme is None else z.csi_run(foff, tables.win_off, bcarry, *scheme)
            assert b["n"] == n_use
            tables.add_run(b, r["heads"][:n_use])
            bcarry = b["carry"]
            info["runs"] += 1
            for k in ("ms_inflate", "ms_chain"):
                info[k] += r[k]
            for k in ("ms_span", "ms_linear", "ms_runs"):
                info[k] += b[k]
            info["peak_stream_len"] = max(info["peak_stream_len"], r["stream_len"])
            info["bytes_h2d"] += stop - fo + members.nbytes + foff.nbytes
            fo, carry, done = _next_run(r, n_use, members, foff, carry, int(bcarry.count))
            info["stream_bytes"] += done
            budget = max(1, int(run_bytes))
        index = tables.finish()
        if stats is not None:
            stats.update(info)
        if out is not None:
            (bamindex.write_bai if scheme is None else bamindex.write_csi)(index, out)
        return index
    finally:
        if z is not None:
            z.close()
        data.close()


class IndexedBam:
    """A BAM file with its index (`open_indexed`): the header, the counts of the index, and `fetch_device` - only the compressed
    bytes a contig or a region needs are read and uploaded, the records a fetch returns own their device memory."""

    def __init__(self, path, data, ref_names, ref_lens, hlen, index, device):
        self.path, self._data, self.ref_names, self.ref_lens, self.hlen, self.index, self.device = path, data, ref_names, ref_lens, hlen, index, device
        self.fetches = []        # the `info` of every fetch so far (bytes_read, stream_len, ...)

    def close(self):
        if self._data is not None:
            self._data.close()
            self._data = None

    def fetch_device(self, contig: str, start: int = None, end: int = None) -> DeviceBamRecords:
        """A superset of the records `bam.fetch(contig, start, end)` iterates, in file order, in HBM: everything that starts
        between the first and the last chunk the index gives for the interval; `keep` marks the mapped ones of the contig (the
        extraction applies the interval itself).  Close the returned records to free the contig."""
        from . import abi
        rid = self.ref_names.index(contig)
        data = self._data
        ch = self.index.query(rid, 0 if start is None else start, end)
        z = BgzfDevice(self.device)
        try:
            if ch.shape[0] == 0:
                fo = stop = skip = 0
                members = bgzf_members(b"")
                end_pos = 0
            else:
                vb, ve = int(ch[0, 0]), int(ch[-1, 1])
                fo, skip = vb >> 16, vb & 0xffff
                last = ve >> 16
                members = bgzf_members(data, fo, min(len(data), last + (1 if ve & 0xffff else 0)))
                foff = member_file_offsets(members, fo)
                stop = int(foff[-1])
                k = int(np.searchsorted(foff[:-1], last, side="left"))
                end_pos = int(members["out_off"][k]) + (ve & 0xffff) if k < members.shape[0] else int(members["isize"].sum())
            rel = members.copy()
            rel["payload_off"] -= fo
            carry = abi.snf_bam_carry_t(skip=skip, count=0, stream_pos=0, origin=skip, n_part=0)
            try:
                r = z.inflate(memoryview(data)[fo:stop] if stop > fo else b"", rel, carry=carry)
            except z._err as e:
                if str(e).startswith("truncated BAM record"):
                    raise ValueError(str(e)) from None
                if "do not fit the free device memory" in str(e):
                    raise z._err(f"contig {contig}: {e}") from None
                raise
            n = int(np.searchsorted(r["rec_off"][:r["n"]] + skip, end_pos, side="left"))      # records that start at or behind the end: not ours
            heads = np.ascontiguousarray(r["heads"][:n])
            ref_id = heads[:, 1].astype(np.uint32).view(np.int32).copy()
            flags = (heads[:, 4] >> 16).astype(np.uint16)
            info = dict(ms_inflate=r["ms_inflate"], ms_chain=r["ms_chain"], compressed_bytes=stop - fo, bytes_read=stop - fo, stream_len=r["stream_len"],
                        bytes_h2d=stop - fo + members.nbytes, bytes_d2h=r["rec_off"].nbytes + r["heads"].nbytes + r["names"].nbytes,
                        contig=contig, start=start, end=end)
            self.fetches.append(info)
            return DeviceBamRecords(self.ref_names, self.ref_lens, r["rec_off"][:n + 1], ref_id, heads[:, 2].astype(np.uint32).view(np.int32).copy(),
                                    flags, heads, r["names"][:n], z, r["d_stream"] + skip, r["stream_len"] - skip, r["d_rec_off"], r["device"],
                                    keep=(ref_id == rid) & ((flags & 0x4) == 0), info=info, owns_handle=True)
        except Exception:
            z.close()
            raise


def open_indexed(path: str, index=None, device: int = 0) -> IndexedBam:
    """`path` memory-mapped, its header parsed from the leading members, its index loaded: `index` is a `bamindex.BamIndex`, the
    path of a BAI / CSI file, or None for `bamindex.find_index(path)`.  A file without an index is refused as the reference's
    `check_index` refuses it (`bam.index_bam` builds one)."""
    from . import bamindex
    if index is None:
        index = bamindex.find_index(path)
        if index is None:
            raise ValueError(f"Unable to load index for input file '{path}'. Please verify that your input file is sorted + indexed "
                             f"and that the index .bai file is valid and in the right location.")
    if not isinstance(index, bamindex.BamIndex):
        index = bamindex.read_index(index)
    data = _map_file(path)
    try:
        names, lens, hlen = leading_header(data)
        if index.n_ref != len(names):
            raise ValueError(f"the index holds {index.n_ref} references, the header of {path} {len(names)}")
    except Exception:
        data.close()
        raise
    return IndexedBam(path, data, names, lens, hlen, index, device)
