"""The reference's dense coverage vector and what it computes on it, restated plainly (no threshold of the library enters here;
tests/coverage_cases.py builds the tasks, tests/test_coverage_edges.py and tests/test_snf.py compare).

The library keeps no coverage vector: the reference's `np.uint16` array of `contig_len` (leadprov.py:451, `coverage[s:e] += 1` per read,
leadprov.py:510; runs of 'N' zeroed afterwards, leadprov.py:420-443) is answered by rank queries over sorted read starts and ends.  Here
the vector is built as the reference builds it (vectorised: difference array, cumsum, mod 2^16), and `postprocessing.coverage`
(postprocessing.py:69-130), `coverage.mean()` (the vector's own `.mean()`) and `SNFile.annotate_block_coverages` (snf.py:249-267) are
restated on top of it."""
import numpy as np

BINSIZE, UPDOWN = 100, 5                             # coverage_binsize (= cluster_binsize), coverage_updown_bins: the defaults


# ---------------------------------------------------------------------------------------------- the reference, restated
def dense(ti):
    """The reference's coverage vector of a task: uint16, one increment per read over [start, end), mask intervals zeroed."""
    L = int(ti.contig_len)
    d = np.zeros(L + 1, np.int64)
    s = np.minimum(ti.read_start.astype(np.int64), L)
    e = np.minimum(ti.read_end.astype(np.int64), L)
    np.add.at(d, s, 1)
    np.add.at(d, e, -1)
    cov = (np.cumsum(d[:L]) % 65536).astype(np.uint16)
    if getattr(ti, "nmask_start", None) is not None:
        for a, b in zip(ti.nmask_start.tolist(), ti.nmask_end.tolist()):
            cov[a:b] = 0
    return cov


def dense_block_coverage(ti, binsize):
    """SNFile.annotate_block_coverages (snf.py:249-267): the vector zero-padded to a multiple of `binsize`, float64 mean per bin, round()."""
    cov = dense(ti)
    pad = -len(cov) % binsize
    return [round(x) for x in np.pad(cov, (0, pad), mode="constant").reshape(-1, binsize).mean(axis=1)]


def ref_coverage(cv, calls, binsize=BINSIZE, updown=UPDOWN):
    """postprocessing.coverage (postprocessing.py:69-130) over `calls` = [(svtype name, pos, svlen, bnd_is_first, [5 fields])]: returns
    (the five fields of every call, status).  `end` lives on from call to call as the loop variable of the reference does: a BND takes
    the one of the call before it, and a BND with nothing before it is the reference's UnboundLocalError - status 1, that call and every
    later one untouched.  An IndexError leaves the field as it was; a negative index counts from the end (numpy)."""
    out = [list(c[4]) for c in calls]
    have_end, end = False, None

    def sample(row, k, idx):
        try:
            row[k] = int(cv[idx])
        except IndexError:
            pass
    for i, (svtype, pos, svlen, first, _) in enumerate(calls):
        start = pos
        if svtype == "INS":
            end, have_end = start + 1, True
        elif svtype == "BND":
            if first:
                start -= 1
            if not have_end:
                return out, 1
        else:
            end, have_end = pos + abs(svlen), True
        row = out[i]
        if svtype in ("INS", "BND"):
            sample(row, 1, start - binsize)
            sample(row, 2, start)
            sample(row, 3, end + binsize)
        else:
            sample(row, 1, start)
            sample(row, 2, int((start + end) / 2))
            sample(row, 3, end - binsize)
        sample(row, 0, start - binsize * updown)
        sample(row, 4, end + binsize * updown)
    return out, 0


def sample_indices(svtype, pos, svlen, first, end_before=None, binsize=BINSIZE, updown=UPDOWN):
    """The five indices (upstream, start, center, end, downstream) of one call, as postprocessing.coverage forms them."""
    start = pos
    if svtype == "INS":
        end = start + 1
    elif svtype == "BND":
        start -= 1 if first else 0
        end = end_before
    else:
        end = pos + abs(svlen)
    if svtype in ("INS", "BND"):
        mid = [start - binsize, start, None if end is None else end + binsize]
    else:
        mid = [start, int((start + end) / 2), end - binsize]
    return [start - binsize * updown] + mid + [None if end is None else end + binsize * updown]
