"""The read-table rank index and the coverage kernels on it, at the borders of the index (tests/size_classes.py::coverage_thresholds
reads the sizes from the sources; tests/coverage_cases.py restates the reference and builds the tasks).

The reference keeps a dense uint16 coverage vector per contig; the library answers the same questions - the five samples of a call
(d4s_coverage / d4_coverage for the batch's own candidates, s2_covends / s2_covcalls for the calls of a force-calling run), coverage.mean()
(d5w_covsum, d5x_covexact), the per-bin means of the SNF writer (s1_blockcov), the largest depth (r3_maxdepth) - by rank queries over the
sorted read starts and ends of all tasks, through sampled levels at every 16th, 256th and 4096th GLOBAL position (r1_endkeys / r2_unpack
build them; bound_top_i32, rank_upper_16ary, rank_level16, upper_bound_hint_i32 of snf_exact.h descend them).  A task's segment begins
anywhere, so the cases put segment borders, runs of equal values and the queried values themselves on the borders of every level; the
uint16 wrap decision at depth 65 536 and the 4096-position chunks of the exact walk get their - 1 / 0 / + 1 too.  Every comparison is
exact: integers, and == on float64.  Every case has a host-tier form (tests/emu) and a `-m gpu` form."""
import collections

import numpy as np
import pytest

import coverage_cases as cc
import size_classes as sc
from sniffles_amd import lib
from sniffles_amd.config import SnifflesConfig

CT = cc.CT
TIERS = ["host", pytest.param("gpu", marks=pytest.mark.gpu)]


def use_tier(tier, monkeypatch):
    if tier == "host":
        import emu.emu as E
        E.lib()
    else:
        assert lib.device_count() >= 1


def forms_lines(capfd):
    return [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("[SNF_PROF] forms:")]


# ---------------------------------------------------------------------------------------------- the borders themselves
def test_thresholds_are_found_and_the_index_batch_sits_on_them():
    assert (cc.NODE, cc.MID, cc.TOP) == (16, 256, 4096) and 1 << CT["top_shift"] == 256     # the level layout the cases are placed on
    assert CT["cov_chunk"] == 256 and CT["covx_chunk"] == 4096 and CT["gt_n"] == 251 and CT["wrap_depth"] == 65536
    off = cc.index_offsets()
    los, counts = off[:-1], list(cc.INDEX_COUNTS)
    assert {0, 1, 15} <= {lo % 16 for lo in los}
    assert {255, 0, 1} <= {lo % 256 for lo in los} and {4095, 4096, 4097} <= set(los)
    assert {0, 1, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097} <= set(counts)
    inside = [(lo, lo + n) for lo, n in zip(los, counts) if n and lo % 16 and (lo + n - 1) // 16 == lo // 16]
    assert inside                                                    # a segment inside one node, no sampled position in it
    assert any(n and (lo + n) % 256 == 0 for lo, n in zip(los, counts))                      # ... one that ends on a border
    assert off[-1] % 16 and counts[-1] > 16                          # the last one ends in a partial node at R
    # (f) d5w_covsum (the kernel every pass launches; d5_covsum / SNF_COV_CHUNK is a thread form nothing launches): task borders at
    # positions 4095 / 0 / 1 of a chunk of 4096 GLOBAL reads, a chunk that holds several whole tasks, an empty task between two others
    # inside one chunk, chunks of two tasks, and a last chunk that is cut short by R
    ch = CT["covsum_chunk"]
    assert ch == cc.COVSUM_CHUNK == 4096
    assert {ch - 1, 0, 1} <= {lo % ch for lo, n in zip(los, counts) if n and lo}
    whole = collections.Counter(lo // ch for lo, n in zip(los, counts) if n and lo // ch == (lo + n - 1) // ch)
    assert max(whole.values()) >= 3
    empties = [t for t in range(1, len(counts) - 1) if counts[t] == 0 and counts[t - 1] and counts[t + 1]]
    assert empties and all((los[t] - 1) // ch == los[t] // ch for t in empties)      # the reads on either side lie in ONE chunk
    per_chunk = collections.Counter(c for lo, n in zip(los, counts) if n for c in range(lo // ch, (lo + n - 1) // ch + 1))
    assert 2 in per_chunk.values() and max(per_chunk.values()) > 3 and off[-1] % ch
    # runs of equal starts and of equal ends across a border of every level
    tis, _ = cc.index_tasks()
    gs, ge = cc.global_arrays(tis)
    task_of = np.repeat(np.arange(len(tis)), counts)
    for a in (gs, ge):
        for w in (cc.NODE, cc.MID, cc.TOP):
            g = np.arange(w, len(a), w)
            assert np.any((a[g - 1] == a[g]) & (task_of[g - 1] == task_of[g])), w


def test_a_missing_coverage_threshold_is_an_error(monkeypatch):
    monkeypatch.setattr(sc, "_src", lambda name: "// nothing here\n")
    with pytest.raises(AssertionError):
        sc.coverage_thresholds()


# ---------------------------------------------------------------------------------------------- (a) + (f) index levels, d5w_covsum
def check_point_queries(b, tis, extra=lambda ti: ()):
    """Every task: the INS calls of cc.point_queries against postprocessing.coverage on the dense vector, all five fields, and the mean."""
    total = 0
    for t, ti in enumerate(tis):
        cv = cc.dense(ti)
        calls, n_vals = cc.point_queries(ti, extra(ti))
        assert len(calls) >= 3 * n_vals + 9 and (n_vals > 0) == (len(ti.read_start) > 0)
        got, status, mean = cc.run_calls(b, t, calls)
        want, wstatus = cc.ref_coverage(cv, calls)
        assert status == wstatus == 0
        bad = [(c[1], g, w) for c, g, w in zip(calls, got, want) if g != w]
        assert bad == [], (t, bad[:5])
        assert mean == float(cv.mean()), t
        total += len(calls)
    return total


@pytest.mark.parametrize("sort64", [False, True], ids=["keys32", "SNF_SORT64"])
@pytest.mark.parametrize("tier", TIERS)
def test_samples_and_means_at_every_index_level(tier, sort64, monkeypatch):
    """(a) and (f): Batch.coverage_calls (s2_covends / s2_covcalls: bound_top_i32) with the centre sample on v - 1, v, v + 1 of every read
    start and end of sixteen tasks whose segments begin and end on, before and behind the borders of the 16- / 256- / 4096-levels, and
    coverage.mean() of every task (d5w_covsum: the task borders fall at reads 4095 / 4096 / 4097 of its 4096-read chunks, one chunk holds
    ten whole tasks, an empty task lies between two others inside a chunk - the layout is asserted above).  SNF_SORT64: 64-bit end keys
    in r1_endkeys - that the handle took the key width it is tested for is read from the bytes its sort of the read ends reports
    (R pairs in and out, key + 4-byte value), on a second handle that rebuilds the index inside the pass, where it is bracketed."""
    use_tier(tier, monkeypatch)
    if sort64:
        monkeypatch.setenv("SNF_SORT64", "1")
    tis, _ = cc.index_tasks()
    with lib.Batch(SnifflesConfig(), list(tis)) as b:
        b.call_candidates()
        n = check_point_queries(b, tis)
        res = b.fetch(0)
    assert n > 30_000
    means = [float(cc.dense(ti).mean()) for ti in tis]
    assert [float(x) for x in res.coverage_average_total] == means
    monkeypatch.setenv("SNF_READPREP_EACH_PASS", "1")
    with lib.Batch(SnifflesConfig(), list(tis)) as b:
        b.timing_every(1)
        b.call_candidates()
        res = b.fetch(0)
        sorts = [nbytes for name, _, nbytes in b.timings() if name == "sort_read_ends"]
    R = sum(cc.INDEX_COUNTS)
    assert sorts == [R * 2 * ((8 if sort64 else 4) + 4)], sorts
    assert [float(x) for x in res.coverage_average_total] == means


# ---------------------------------------------------------------------------------------------- (b) the candidates' own samples
@pytest.mark.parametrize("form", ["d4s_coverage", "d4_coverage"])
@pytest.mark.parametrize("tier", TIERS)
def test_the_candidates_own_samples_on_node_borders(tier, form, monkeypatch, capfd):
    """(b) d4s_coverage (a thread per sample, rank_upper_16ary through all three levels) and, under SNF_D4=thread, d4_coverage (a thread per
    call, upper_bound_hint_i32 galloping from the sample before): small clusters of every type whose positions are read starts / ends
    stored AT node borders.  The five indices are formed again from the call's own pos / svlen / svtype; a BND's `end` is the one of
    another call, so only its three start-based samples are compared."""
    use_tier(tier, monkeypatch)
    monkeypatch.setenv("SNF_PROF", "1")
    if form == "d4_coverage":
        monkeypatch.setenv("SNF_D4", "thread")
    tis, plan = cc.index_tasks()
    capfd.readouterr()
    with lib.Batch(SnifflesConfig(), list(tis)) as b:
        lines = forms_lines(capfd)
        b.call_candidates(); b.finalize()
        res = b.fetch(1)
    assert len(lines) == 1 and f"coverage by {form}," in lines[0], lines
    assert [int(s) for s in res.task_status] == [0] * len(tis)
    names = {v: k for k, v in cc.SVT.items()}
    seen, on_border = collections.Counter(), 0
    for t, ti in enumerate(tis):
        cv, L = cc.dense(ti), int(ti.contig_len)
        calls = res.calls[int(res.task_call_off[t]):int(res.task_call_off[t + 1])]
        assert sorted((names[int(c["svtype"])], int(c["pos"])) for c in calls) == sorted((p[0], p[1]) for p in plan[t]), t
        border_values = {p[1] for p in plan[t] if p[2]}
        for c in calls:
            svtype = names[int(c["svtype"])]
            idx = cc.sample_indices(svtype, int(c["pos"]), int(c["svlen"]), bool(c["bnd_is_first"]))
            want = [0 if (i is None or not -L <= i < L) else int(cv[i]) for i in idx]       # (a candidate's fields start as 0, sv.py:117-121)
            got = [int(x) for x in c["cov"]]
            ks = (0, 1, 2) if svtype == "BND" else range(5)
            assert [got[k] for k in ks] == [want[k] for k in ks], (t, svtype, int(c["pos"]), idx, got, want)
            seen[svtype] += 1
            on_border += int(c["pos"]) in border_values
    n_big = sum(1 for n in cc.INDEX_COUNTS if n >= cc.NODE)
    assert all(seen[s] == n_big for s in cc.CLUSTER_TYPES) and seen["BND"] == 2, seen
    assert on_border >= 2 * n_big


# ---------------------------------------------------------------------------------------------- (c) list semantics
def list_task():
    s = [0, 10, 10, 250, 400, 400, 999, 1500]
    e = [700, 10, 900, 260, 2000, 1999, 2000, 1501]
    return cc.read_task(s, e, 2000, 0)


S = cc.SENTINEL
CALL_LISTS = {
    "bnd_first": [("BND", 500, 0, True, [S] * 5), ("INS", 500, 60, False, [S] * 5), ("DEL", 300, -100, False, [S] * 5)],
    "bnd_after_ins": [("INS", 400, 60, False, [S] * 5), ("BND", 900, 0, True, [S] * 5), ("BND", 900, 0, False, [S] * 5)],
    "bnd_after_del": [("DEL", 250, -150, False, [S] * 5), ("BND", 10, 0, False, [S] * 5), ("BND", 10, 0, True, [S] * 5),
                      ("INS", 1500, 5, False, [S] * 5), ("BND", 0, 0, True, [S] * 5)],
    "preset_fields": [("DEL", 250, -150, False, [1, 2, 3, 4, 5])],
    "negative_svlen_and_odd_centre": [("DEL", 251, -150, False, [S] * 5), ("DEL", 250, 151, False, [S] * 5), ("DUP", 9, -2, False, [S] * 5),
                                      ("INV", 0, 1, False, [S] * 5), ("DEL", 1999, -1, False, [S] * 5)],
    "at_minus_L_and_L": [("INS", -2000, 1, False, [S] * 5), ("INS", 2000, 1, False, [S] * 5), ("INS", -2001, 1, False, [S] * 5),
                         ("INS", -1500, 1, False, [S] * 5), ("INS", 1500, 1, False, [S] * 5), ("INS", 1899, 1, False, [S] * 5),
                         ("DEL", 1000, -1100, False, [S] * 5), ("DEL", 1000, -1000, False, [S] * 5), ("DEL", -2000, -4000, False, [S] * 5),
                         ("BND", -1999, 0, True, [S] * 5), ("BND", 2000, 0, True, [S] * 5)],
    "empty": [],
}


@pytest.mark.parametrize("tier", TIERS)
def test_coverage_calls_list_semantics(tier, monkeypatch):
    """(c) what the loop of postprocessing.coverage does to a LIST: `end` carried into a BND from the call before it (INS: pos + 1; any
    other type: pos + |svlen|), bnd_is_first moving the start, a BND with nothing before it (status 1, that call and the rest untouched),
    negative svlen, a centre whose start + end is odd, samples exactly at -L (the first position) and at L (outside), and no call at all."""
    use_tier(tier, monkeypatch)
    ti = list_task()
    cv = cc.dense(ti)
    with lib.Batch(SnifflesConfig(), [ti]) as b:
        b.call_candidates()
        for name, calls in CALL_LISTS.items():
            got, status, mean = cc.run_calls(b, 0, calls)
            want, wstatus = cc.ref_coverage(cv, calls)
            assert (got, status) == (want, wstatus), name
            assert mean == float(cv.mean())
        got, status, _ = cc.run_calls(b, 0, CALL_LISTS["bnd_first"])
        assert status == 1 and got == [[S] * 5] * 3
        got, status, _ = cc.run_calls(b, 0, CALL_LISTS["empty"])
        assert status == 0 and got == []
    # the lists do what they are named after on the dense vector itself
    want, _ = cc.ref_coverage(cv, CALL_LISTS["bnd_after_del"])
    assert want[1][3] == int(cv[400 + 100]) and want[2][2] == int(cv[9]) and want[4][2] == int(cv[-1]) and want[4][3] == int(cv[1501 + 100])
    want, _ = cc.ref_coverage(cv, CALL_LISTS["at_minus_L_and_L"])
    assert want[0][2] == int(cv[0]) and want[1][2] == S and want[2][2] == S and want[1][1] == int(cv[1900])
    want, _ = cc.ref_coverage(cv, CALL_LISTS["negative_svlen_and_odd_centre"])
    assert want[0][2] == int(cv[326]) and want[1][2] == int(cv[325])


# ---------------------------------------------------------------------------------------------- (d) + (e) wrap decision, exact walk
def check_means_and_blocks(b, tis):
    for t, ti in enumerate(tis):
        for bs in cc.BLOCK_BINSIZES:
            want = cc.dense_block_coverage(ti, bs)
            got = b.block_coverage(t, bs, 0, len(want) + 1)
            assert got[:len(want)].tolist() == want, (t, bs)
            assert int(got[len(want)]) == -1, (t, bs)            # a bin beyond the padded vector


@pytest.mark.parametrize("exact", [False, True], ids=["decided", "SNF_COV_EXACT"])
@pytest.mark.parametrize("tier", TIERS)
def test_the_uint16_wrap_decision(tier, exact, monkeypatch):
    """(d) largest depth 65 535 / 65 536 / 65 537 (r3_maxdepth and the decision `>= 65536` of the upload) at L = 8192 / 8193: at 65 536 the
    dense vector reads 0 over the deepest stretch, and a task that wrongly kept the closed forms would report a mean larger by orders of
    magnitude.  Point samples around every depth change, coverage.mean(), block coverage (s1_blockcov; d5x_covexact / cov_range_sum for
    the tasks that wrap).  Then the same with the exact walk forced on every task."""
    use_tier(tier, monkeypatch)
    if exact:
        monkeypatch.setenv("SNF_COV_EXACT", "1")
    tis = cc.wrap_tasks()
    assert [int(cc.dense(ti).max()) for ti in tis] == [65535, 65535, 31] * 2       # the deepest stretch reads 65 535, 0 and 1
    assert [int(cc.dense(ti)[1700]) for ti in tis] == [65535, 0, 1] * 2
    with lib.Batch(SnifflesConfig(), list(tis)) as b:
        b.call_candidates()
        assert check_point_queries(b, tis) > 6 * 3 * 40
        check_means_and_blocks(b, tis)


@pytest.mark.parametrize("tier", TIERS)
def test_the_exact_walk_at_chunk_and_mask_borders(tier, monkeypatch):
    """(e) masked tasks (always the exact walk) of L = SNF_COVX_CHUNK - 1 / + 0 / + 1 and 2 * SNF_COVX_CHUNK + 1 with read starts, read ends
    and mask borders at 4096 k - 1 / + 0 / + 1, a single-base mask and a mask that touches L: point samples at nm_start - 1, nm_start,
    nm_end - 1, nm_end and around every read start and end, coverage.mean(), block coverage."""
    use_tier(tier, monkeypatch)
    tis = cc.masked_tasks()
    assert [int(ti.contig_len) for ti in tis] == [CT["covx_chunk"] - 1, CT["covx_chunk"], CT["covx_chunk"] + 1, 2 * CT["covx_chunk"] + 1]
    for ti in tis:
        assert int(ti.nmask_end[-1]) == ti.contig_len and any(b - a == 1 for a, b in zip(ti.nmask_start.tolist(), ti.nmask_end.tolist()))
    with lib.Batch(SnifflesConfig(), list(tis)) as b:
        b.call_candidates()
        check_point_queries(b, tis, cc.mask_points)
        check_means_and_blocks(b, tis)


# ---------------------------------------------------------------------------------------------- legal input
@pytest.mark.parametrize("tier", TIERS)
def test_illegal_reads_and_masks_are_refused(tier, monkeypatch):
    """What keeps the builders honest: a read that starts at L (or ends before it starts) and a mask that leaves the contig, overlaps the
    one before it or is empty are refused by the upload."""
    use_tier(tier, monkeypatch)

    def task(s, e, mask=None):
        ti = cc.read_task([5], [50], 1000, 0)
        ti.read_start, ti.read_end, ti.read_hp = np.array(s, np.int32), np.array(e, np.int32), np.zeros(len(s), np.uint8)
        if mask:
            ti.nmask_start, ti.nmask_end = np.array([m[0] for m in mask], np.int32), np.array([m[1] for m in mask], np.int32)
        return ti
    with lib.Batch(SnifflesConfig(), [task([999], [1000], [(0, 1), (1, 1000)])]) as b:       # the legal extremes pass
        b.call_candidates()
    for bad in (task([1000], [1000]), task([10], [9]), task([-1], [5]), task([5], [50], [(900, 1001)]), task([5], [50], [(10, 20), (19, 30)]),
                task([5], [50], [(10, 10)])):
        with pytest.raises(lib.SnifflesAmdError):
            with lib.Batch(SnifflesConfig(), [bad]):
                pass
