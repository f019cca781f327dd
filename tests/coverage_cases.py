"""The task builders of tests/test_coverage_edges.py (the reference they are compared with: tests/coverage_ref.py).

The library keeps no coverage vector: the reference's `np.uint16` array of `contig_len` (leadprov.py:451, `coverage[s:e] += 1` per read,
leadprov.py:510; runs of 'N' zeroed afterwards, leadprov.py:420-443) is answered by rank queries over the sorted read starts and the sorted
read ends of ALL tasks of a batch, with sampled levels at every 16th, 256th and 4096th GLOBAL position (snf_exact.h), and coverage.mean()
is summed over chunks of 4096 GLOBAL reads (d5w_covsum).  The builders place the task segments
and the values inside them on the borders of those levels; every input is legal (reads inside [0, L], masks sorted, disjoint, non-empty and
inside the contig - the upload refuses anything else)."""
import functools

import numpy as np

import cases
import size_classes as sc
from coverage_ref import BINSIZE, UPDOWN, dense, dense_block_coverage, ref_coverage, sample_indices      # noqa: F401 - one name space for the tests
from sniffles_amd.soa import SVT

CT = sc.coverage_thresholds()
NODE, MID, TOP = 16, 1 << CT["top_shift"], 4096      # rank_upper_16ary: 16 entries a node, three levels (the 16 and the 4096 are literals there)
COVSUM_CHUNK = CT["covsum_chunk"]                    # d5w_covsum: reads per workgroup round
SENTINEL = -7                                        # initial value of a coverage field that has to "keep its value"
BLOCK_BINSIZES = (500, 7, 2, 1, 4096)


# ---------------------------------------------------------------------------------------------- through the library
def code(svtype):
    """The type code `postprocessing.coverage` of this package hands to the library: every type but INS / BND samples like a DEL."""
    return SVT[svtype] if svtype in ("INS", "BND") else SVT["DEL"]


def run_calls(batch, t, calls):
    """`calls` as for ref_coverage through Batch.coverage_calls: (rows, status, mean)."""
    out, status, mean = batch.coverage_calls(t, [code(c[0]) for c in calls], [c[1] for c in calls], [c[2] for c in calls],
                                             [1 if c[3] else 0 for c in calls], [c[4] for c in calls])
    return out.tolist(), status, mean


# ---------------------------------------------------------------------------------------------- builders
def read_task(starts, ends, L, task_id, leads=(), mask=None):
    """A task over the given reads (sorted by start here, stably - the order the library keeps)."""
    ti = cases.mk_task(list(leads), [], int(L), task_id=task_id, contig=f"chrV{task_id}")
    s, e = np.asarray(starts, np.int32), np.asarray(ends, np.int32)
    assert len(s) == len(e) and (len(s) == 0 or (s.min() >= 0 and s.max() < L and e.max() <= L and (e >= s).all()))
    o = np.argsort(s, kind="stable")
    ti.read_start, ti.read_end, ti.read_hp = s[o], e[o], (np.arange(len(s)) % 3).astype(np.uint8)
    if mask:
        prev = 0
        for a, b in mask:
            assert prev <= a < b <= L
            prev = b
        ti.nmask_start, ti.nmask_end = np.array([m[0] for m in mask], np.int32), np.array([m[1] for m in mask], np.int32)
    ti.validate()
    return ti


# (a) read counts of the index batch.  With the running sum as the global offset `lo` of a task's segment [lo, hi) of the read arrays:
#   t0 4095 [0, 4095)  t1 1 [4095, 4096)  t2 1 [4096, 4097)  t3 4096 [4097, 8193)  t4 0 (empty)  t5 4097 [8193, 12290)
#   t6 13 [12290, 12303): wholly inside the node [12288, 12304), no sampled position of any level in it
#   t7 15 [12303, 12318)  t8 225 [12318, 12543)  t9 1 [12543, 12544): ends on a border of all three lower levels
#   t10 257 [12544, 12801)  t11 256 [12801, 13057)  t12 255 [13057, 13312)  t13 16 [13312, 13328)  t14 17 [13328, 13345)
#   t15 300 [13345, 13645): R = 13645 ends in a partial node.
# coverage.mean() is summed by d5w_covsum over chunks of COVSUM_CHUNK = 4096 GLOBAL reads, a pass per task present in a chunk: the task
# borders 4095 / 4096 / 4097 are positions 4095 / 0 / 1 of their chunks; the chunk [8192, 12288) holds the last read of t3, the empty t4
# and the head of t5; the last chunk [12288, 13645) holds the tail of t5 and ten whole tasks.
INDEX_COUNTS = (4095, 1, 1, 4096, 0, 4097, 13, 15, 225, 1, 257, 256, 255, 16, 17, 300)
CLUSTER_TYPES = ("DEL", "INS", "DUP", "INV")
DEL_LEN = 300


def index_offsets():
    return np.concatenate(([0], np.cumsum(INDEX_COUNTS))).tolist()


def _borders(lo, hi):
    """Global positions in (lo + 2, hi - 2) that are multiples of 4096, of 256 and of 16: the first of each and the last multiple of 16."""
    out = []
    for w in (TOP, MID, NODE):
        g = (lo + 3 + w - 1) // w * w
        if g < hi - 2 and g not in out:
            out.append(g)
    g = (hi - 3) // NODE * NODE
    if g > lo + 2 and g not in out:
        out.append(g)
    return out


def _cluster_borders(lo, hi):
    """Global positions in [lo, hi) that are multiples of 16, the higher levels first (needs hi - lo >= 16)."""
    out = []
    for w in (TOP, MID, NODE):
        g = (lo + w - 1) // w * w
        if g < hi and g not in out:
            out.append(g)
    g = (hi - 1) // NODE * NODE
    if g >= lo and g not in out:
        out.append(g)
    return out


def _reads_with_runs(rng, n, L, lo):
    """n reads of a contig of L bases whose sorted starts and whose sorted ends each carry a run of four equal values across every border
    of _borders(lo, lo + n) - two entries on either side of the global position - besides the many ties a short contig gives anyway.
    Returns (starts ascending, ends: ends[i] belongs to starts[i], ends sorted ascending)."""
    s = np.sort(rng.integers(0, L - 1, n))
    ln = rng.integers(0, max(2, L // 2), n)
    ln[rng.random(n) < 0.05] = 0                               # zero-length reads: a start and an end at once
    e = np.sort(np.minimum(s + ln, L))                         # the k-th smallest end is >= the k-th smallest start
    for g in _borders(lo, lo + n):
        k = g - lo
        s[k - 2:k + 2] = s[k - 2]
        e[k - 2:k + 2] = e[k + 1]
    assert (e >= s).all() and (np.diff(s) >= 0).all() and (np.diff(e) >= 0).all()
    return s, e


@functools.lru_cache(maxsize=None)
def index_tasks():
    """The batch of (a), (b) and (f): (tasks, plan) - plan[t] = [(svtype, position, on_border)] of the clusters of task t, whose positions are
    read starts (DEL, DUP) and read ends (INS, INV) stored AT a border of a level of the global arrays (on_border: the value itself, not
    clipped into the contig)."""
    off = index_offsets()
    tis, plan = [], []
    for t, n in enumerate(INDEX_COUNTS):
        rng = np.random.default_rng([t, 6101])
        L = 3001 + 211 * t
        lo = off[t]
        if n == 0:
            tis.append(read_task([], [], L, t)); plan.append([]); continue
        s, e = _reads_with_runs(rng, n, L, lo) if n >= 8 else (np.sort(rng.integers(0, L - 1, n)), None)
        if e is None:
            e = np.minimum(s + rng.integers(1, L, n), L)
        leads, clusters = [], []
        if n >= NODE:
            allele = cases._rng_seq(rng, 90)
            B = _cluster_borders(lo, lo + n)
            for c, svtype in enumerate(CLUSTER_TYPES):
                g = B[c % len(B)]
                v = int((s if svtype in ("DEL", "DUP") else e)[g - lo])
                # (a lead lies inside the contig, a read may end AT L; a DEL lead lies behind the deleted bases: the call begins at
                # ref_start + svlen)
                shift = DEL_LEN if svtype == "DEL" else 0
                p = min(max(v, 1), L - 2 - shift)
                for i in range(6 + c % 3):
                    d = cases._ladder_lead(svtype, rng, p, f"t{t}c{c}_{i}", i, allele, c)
                    d["ref_start"] = p + shift                  # every lead AT the border value: the call's position is that value
                    if svtype == "DEL":
                        d["svlen"] = -DEL_LEN
                    leads.append(d)
                clusters.append((svtype, p, p == v))
            if t in (3, 10):                                    # a BND cluster behind the others (a task of BNDs alone is the reference's error)
                p = int(s[n // 2]) + 1
                for i in range(6):
                    d = cases._ladder_lead("BND", rng, p, f"t{t}b_{i}", i, None, 0)
                    d["ref_start"] = p
                    leads.append(d)
                clusters.append(("BND", p, False))
        o = rng.permutation(n)                                  # ends[i] >= starts[i] holds for the sorted pairing; the reads come unsorted
        tis.append(read_task(s[o], e[o], L, t, leads))
        plan.append(clusters)
    return tis, plan


def global_arrays(tis):
    """The two arrays the index samples: every task's read starts ascending, and its read ends ascending, task after task."""
    return (np.concatenate([np.sort(ti.read_start) for ti in tis]), np.concatenate([np.sort(ti.read_end) for ti in tis]))


def point_queries(ti, extra=()):
    """INS calls whose centre sample lands on v - 1, v, v + 1 for every distinct read start and read end v of the task, on the edges of
    the index range (0, 1, L - 2, L - 1, L, L + 5, -1, -L, -L - 1) and on `extra`; every field starts as SENTINEL.  Returns
    (calls, number of distinct values)."""
    L = int(ti.contig_len)
    vals = sorted(set(ti.read_start.tolist()) | set(ti.read_end.tolist()))
    xs = [v + d for v in vals for d in (-1, 0, 1)] + [0, 1, L - 2, L - 1, L, L + 5, -1, -L, -L - 1] + list(extra)
    return [("INS", int(x), 1, False, [SENTINEL] * 5) for x in xs], len(vals)


# (d) the uint16 wrap decision
WRAP_DEPTHS = tuple(sc.around(CT["wrap_depth"]))             # 65 535, 65 536, 65 537
WRAP_LENGTHS = (2 * CT["covx_chunk"], 2 * CT["covx_chunk"] + 1)


@functools.lru_cache(maxsize=None)
def wrap_tasks():
    """Six tasks whose largest depth is 65 535 / 65 536 / 65 537 (the decision `>= 65536` of the upload, r3_maxdepth) at L = 8192 / 8193:
    D - 2 identical reads over [1000, 3000), one read [500, 2000) and one [1500, 4000) - the depth is D over [1500, 2000) only - three
    zero-length reads at 1500 (a start and an end at the deepest start: they change no depth), and an ordinary stretch that ends at L."""
    tis = []
    for L in WRAP_LENGTHS:
        for D in WRAP_DEPTHS:
            s = [1000] * (D - 2) + [500, 1500] + [1500] * 3 + [4000 + 37 * i for i in range(30)] + [L - 1, 4095, 4096, 4097]
            e = [3000] * (D - 2) + [2000, 4000] + [1500] * 3 + [L - 41 * i for i in range(30)] + [L, 4096, 4097, L]
            tis.append(read_task(s, e, L, len(tis)))
    return tis


# (e) the exact walk and the mask borders
MASKED = {
    CT["covx_chunk"] - 1: [(100, 101), (2000, 2300), (4090, 4095)],
    CT["covx_chunk"]: [(100, 101), (4000, 4095), (4095, 4096)],
    CT["covx_chunk"] + 1: [(100, 101), (4095, 4096), (4096, 4097)],
    2 * CT["covx_chunk"] + 1: [(100, 101), (4095, 4097), (5000, 5001), (8191, 8192), (8192, 8193)],
}


@functools.lru_cache(maxsize=None)
def masked_tasks():
    """Masked tasks of L = SNF_COVX_CHUNK - 1 / + 0 / + 1 and 2 * SNF_COVX_CHUNK + 1: read starts, read ends and mask borders at
    4096 k - 1 / + 0 / + 1 (clipped to what is legal), a single-base mask and a mask that touches L in each."""
    tis = []
    for L, mask in MASKED.items():
        P = sorted({p for k in (1, 2) for p in (CT["covx_chunk"] * k - 1, CT["covx_chunk"] * k, CT["covx_chunk"] * k + 1) if p <= L} | {99, 101, 2150})
        s, e = [0] * 20, [L] * 20
        for p in P:
            if p < L:
                s += [p, p]; e += [min(L, p + 700), p]          # a read that starts at p, and a zero-length one
            s += [max(0, p - 900)]; e += [p]                     # a read that ends at p
        tis.append(read_task(s, e, L, len(tis), mask=mask))
    return tis


def mask_points(ti):
    return [x for a, b in zip(ti.nmask_start.tolist(), ti.nmask_end.tolist()) for x in (a - 1, a, b - 1, b)]
