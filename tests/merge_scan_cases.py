"""Builders for the directed cases of the adaptive merge scan (snf_stage_cluster.h, stages B and C; tests/test_merge_scan_edges.py runs
them, the unmodified reference's clusters for every table are tests/golden/merge_scan_edges.json.gz).

A case is a batch of tasks made from SEEDS - S(bin, offsets, svlen): the leads of one bin of `cluster_binsize` bp at bin * binsize +
offset, in arrival order - grouped by (task, svtype), plus the tasks' tandem repeats, the options and what the case is ABOUT: trace
tuples of the restatement (tests/merge_scan_ref.py) that must occur, asserted when the table is built, so that a case that has left its
edge fails as such.  Two facts carry most builders: three leads at a, a + k, a + 2k have statistics.stdev exactly k (the variance k^2 is
an exact rational and its root is exact), and seed starts are multiples of the bin size, so `inner` and `outer` are too.  At the
defaults (cluster_r 2.5) inner = 100 merges iff both neighbours have k >= 40.

`plan` maps a value of SNF_RUN_GAP (None: unset) to the number of (task, svtype) groups the library must redo serially; the number of
runs follows from the seeds alone (runs_planned)."""
import numpy as np

import cases
import merge_scan_ref as ref
import size_classes as sc
from sniffles_amd.config import SnifflesConfig
from sniffles_amd.soa import SVTYPES

T = sc.merge_thresholds()
CAP, ADDED, MCH = T["sample_cap"], T["added_below"], T["mch"]
GAPS = (None, "0", "100", "-1")
FAR = 50                      # bins between the pieces of a table that must not see each other (inner 4 900 bp and more)
_SVLEN = dict(DEL=300, INS=90, DUP=700, INV=900, BND=0)
_ALLELES = {}


def S(b, offs, svlen=None, long_every=0):
    """One bin: leads at offsets `offs` (arrival order); svlen: one magnitude or one per lead (DEL leads carry it negated);
    long_every = m: INS leads 0, m, 2m ... carry no length (`leads_long`)."""
    return dict(bin=b, offs=list(offs), svlen=svlen, long_every=long_every)


def three(b, k, svlen=None, at=0):
    return S(b, [at, at + k, at + 2 * k], svlen)


def same(b, n, off=0, svlen=None):
    return S(b, [off] * n, svlen)


def _allele(n):
    if n not in _ALLELES:
        _ALLELES[n] = cases._rng_seq(np.random.default_rng([n, 811]), n)
    return _ALLELES[n]


def _lead(svtype, pos, svlen, name, i, c, is_long):
    d = dict(svtype=svtype, ref_start=pos, read=name, strand="+-"[i % 2])
    s = _SVLEN[svtype] if svlen is None else svlen
    if svtype == "DEL":
        d["svlen"] = -s
    elif svtype == "INS":
        d.update(svlen=None, seq=None) if is_long else d.update(svlen=s, seq=_allele(s))
    elif svtype == "BND":
        d["mate"] = ("chr2", 700_000 + 5000 * (c % 100) + i % 7, True, False)
    else:
        d.update(svlen=s, source="SPLIT_SUP")
    return d


def case(groups, cfg=None, trs=None, bs=100, contig_len=None, n_tasks=None, expect=(), plan=None, env=None, forms=None):
    """groups: [(task, svtype, [S ...])]; trs: {task: [(start, end) ...]} (a task not named: None); expect: [(task, svtype, kind,
    {field: value or predicate}, count or None)] - so many tuples of that kind (None: at least one) in the group's trace."""
    cfg = dict(cfg or {})
    if bs != 100:
        cfg["cluster_binsize"] = bs
    last = max(s["bin"] for _, _, ss in groups for s in ss)
    return dict(groups=groups, cfg=cfg, trs=dict(trs or {}), bs=bs, contig_len=contig_len or (last + FAR) * bs, n_tasks=n_tasks,
                expect=list(expect), plan=dict(plan or {}), env=dict(env or {}), forms=forms)


def build(c):
    """The tasks of a case: the leads of a task arrive one per bin in turn (the stable sort by bin then has work to do and the order
    inside a bin stays the planned one)."""
    Tn = c["n_tasks"] if c["n_tasks"] is not None else 1 + max(g[0] for g in c["groups"])
    per = [[] for _ in range(Tn)]
    for gi, (t, svtype, seeds) in enumerate(c["groups"]):
        for si, s in enumerate(seeds):
            for i, off in enumerate(s["offs"]):
                assert 0 <= off < c["bs"], (s, c["bs"])
                sv = s["svlen"][i] if isinstance(s["svlen"], (list, tuple)) else s["svlen"]
                is_long = bool(s["long_every"]) and i % s["long_every"] == 0
                per[t].append((i, gi, si, _lead(svtype, s["bin"] * c["bs"] + off, sv, f"g{gi}s{si}_{i}", i, si, is_long)))
    tis = []
    for t in range(Tn):
        L = c["contig_len"]
        leads = [x[3] for x in sorted(per[t], key=lambda x: x[:3])]
        if leads and all(d["svtype"] == "BND" for d in leads):
            raise AssertionError("a task of BND leads only is the reference's UnboundLocalError (cases.case_bnd_first_error): add another type")
        R = min(L, 200_000)          # (reads over the front of a very long contig only: the reference counts coverage base by base)
        tis.append(cases.mk_task(leads, cases._reads(24, 0, R) + cases._reads(6, 0, max(1, R // 2), 1), L, trs=c["trs"].get(t), task_id=t, contig=f"chrM{t}"))
    return tis


def config(c):
    return SnifflesConfig(**c["cfg"])


def reference_args(c):
    """The options of a case as the reference's command line takes them."""
    out = []
    for k, v in sorted(c["cfg"].items()):
        out += ["--" + k.replace("_", "-")] + ([] if v is True else [str(v)])
    return out


def lead_order_sha(rows, tis):
    """One hash over (ref_start, svlen) of every cluster's leads in list order (the fixture holds it instead of the lists)."""
    import hashlib
    return hashlib.sha256(repr([[(int(tis[r[0]].leads["ref_start"][k]), sv) for k, sv in zip(r[6], r[7])] for r in rows]).encode()).hexdigest()


def planned(c, tis=None):
    """(rows, traces) of the restatement for the case, its `expect` asserted."""
    tis = tis or build(c)
    rows, traces = ref.batch_clusters(tis, config(c))
    for t, svtype, kind, want, count in c["expect"]:
        found = ref.has(traces[(t, svtype)], kind, **want)
        assert (len(found) >= 1 if count is None else len(found) == count), (t, svtype, kind, want, count, [x for x in traces[(t, svtype)] if x[0] == kind])
    return rows, traces


def default_run_gap(cfg):
    """The rule of do_upload: max(1000, cluster_merge_bnd, cluster_repeat_h_max as an int, clamped)."""
    h = cfg.cluster_repeat_h_max
    h = 0 if not h > 0 else T["run_gap_max"] if h >= T["run_gap_max"] else int(h)
    return max(T["run_gap_floor"], cfg.cluster_merge_bnd, h)


def runs_planned(tis, cfg, gap):
    """(run_gap, runs, groups) the library must report: a run begins at the first seed of a group and wherever a seed lies more than
    run_gap behind the end of the seed in front of it (never, for a negative run_gap)."""
    run_gap = default_run_gap(cfg) if gap is None else int(gap)
    runs = groups = 0
    for ti in tis:
        bins = ref.task_bins(ti, cfg)
        for name in SVTYPES:
            seeds = [s for s, leads in bins.get(name, []) if sum(ld[1] is not None for ld in leads) >= cfg.dev_min_leads_cluster]      # (cluster.py:262)
            if not seeds:
                continue
            groups += 1
            runs += 1 + (sum(b - (a + cfg.cluster_binsize) > run_gap for a, b in zip(seeds, seeds[1:])) if run_gap >= 0 else 0)
    return run_gap, runs, groups


CASES = {}
TYPES4 = ("DEL", "INS", "DUP", "INV")


# ---------------------------------------------------------------------------------------------- (a) criterion 1
def _pairs(ks, gap_bins=2, base=10):
    """Pairs of three-lead seeds `gap_bins` apart (inner = (gap_bins - 1) bins), FAR bins between the pairs."""
    out = []
    for j, (ka, kb) in enumerate(ks):
        out += [three(base + FAR * j, ka), three(base + FAR * j + gap_bins, kb)]
    return out


def _crit1():
    c = {}
    ks = [(39, 41), (41, 39), (39, 39), (40, 41), (41, 40), (40, 40), (41, 41)]
    for svtype in TYPES4:
        exp = [(0, svtype, "cmp", dict(inner=100, sd_a=float(a), sd_b=float(b), rule=(1 if min(a, b) >= 40 else None)), 1) for a, b in ks]
        c[f"crit1_inner100_{svtype}"] = case([(0, svtype, _pairs(ks)), (0, "BND" if svtype == "DEL" else "DEL", _pairs([(40, 40), (39, 40)]))], expect=exp)
    # inner = 0 always merges, two seeds of identical positions (sd = 0) and two of one lead each included
    c["crit1_inner0_sd0"] = case([(0, "DEL", [same(10, 3), same(11, 3), same(10 + FAR, 1), same(11 + FAR, 1), same(10 + 2 * FAR, 2), same(12 + 2 * FAR, 2)])],
                                 cfg=dict(dev_min_leads_cluster=1),
                                 expect=[(0, "DEL", "cmp", dict(inner=0, sd_a=0, sd_b=0, rule=1), 2), (0, "DEL", "cmp", dict(inner=100, sd_a=0.0, sd_b=0.0, rule=None), 1)])
    # cluster_r: 5.0 moves the threshold of inner = 100 to k = 20; 0.2 leaves inner = 0 only
    ks = [(19, 21), (20, 21), (21, 20), (20, 20)]
    c["crit1_r5"] = case([(0, "DEL", _pairs(ks))], cfg=dict(cluster_r=5.0),
                         expect=[(0, "DEL", "cmp", dict(inner=100, sd_a=float(a), sd_b=float(b), rule=(1 if min(a, b) >= 20 else None)), 1) for a, b in ks])
    c["crit1_r0_2"] = case([(0, "DEL", _pairs([(49, 49)]) + _pairs([(1, 49)], gap_bins=1, base=10 + FAR))], cfg=dict(cluster_r=0.2),
                           expect=[(0, "DEL", "cmp", dict(inner=100, rule=None), 1), (0, "DEL", "cmp", dict(inner=0, rule=1), 1)])
    c["crit1_r2_5_written_out"] = case([(0, "DUP", _pairs([(39, 40), (40, 40)]))], cfg=dict(cluster_r=2.5),
                                       expect=[(0, "DUP", "cmp", dict(inner=100, rule=1), 1), (0, "DUP", "cmp", dict(inner=100, rule=None), 1)])
    # cluster_binsize 50 (inner = 50: k = 20) and 1000 (inner = 1000: k = 400)
    for bs, k in ((50, 20), (1000, 400)):
        ks = [(k - 1, k + 1), (k, k + 1), (k + 1, k), (k, k), (k + 1, k - 1)]
        c[f"crit1_binsize_{bs}"] = case([(0, "DEL", _pairs(ks)), (1, "INV", _pairs(ks))], bs=bs,
                                        expect=[(t, sv, "cmp", dict(inner=bs, sd_a=float(a), sd_b=float(b), rule=(1 if min(a, b) >= k else None)), 1)
                                                for t, sv in ((0, "DEL"), (1, "INV")) for a, b in ks])
    # inner = 200 needs sd >= 80, more than a bin of 100 bp can have: met by two merged clusters only.  D | a0 a1 | b0 b1: a0 + a1 merge
    # at list index 1 (stay), a | b0 fails, b0 + b1 merge at index 2 (step back), a | b merges
    for d, rule in ((0, 1), (40, None)):      # (the second table: b1's leads closer to b0's - sd of b below 80)
        seeds = [three(2, 1), same(10, 3, 0), same(11, 3, 99), same(14, 3, 0 + d), same(15, 3, 99 - d)]
        c[f"crit1_inner200_by_merged_only_{'merges' if rule else 'fails'}"] = case(
            [(0, "DEL", seeds)], expect=[(0, "DEL", "cmp", dict(inner=200, i=1, sd_a=lambda x: x >= 80, sd_b=(lambda x: x >= 80) if rule else (lambda x: 1 < x < 80), rule=rule), 1),
                                         (0, "DEL", "cmp", dict(inner=200, i=1, sd_b=0.0, rule=None), 1)])
    return c


# ---------------------------------------------------------------------------------------------- (b) criterion 2
def _rep_pair(b, bins_apart, sv_a, sv_b, n_a=3, n_b=3):
    """Two seeds of identical positions (sd = 0: criterion 1 fails for every inner > 0), outer = (bins_apart + 1) bins."""
    return [same(b, n_a, 0, sv_a), same(b + bins_apart, n_b, 0, sv_b)]


def _crit2():
    c = {}
    # outer 900 against 899.5 / 900, outer 1000 against 999 / 1000.5 (h_max itself decides), outer 1100 against h_max
    table = [(8, [300, 300, 299], 300, None), (8, 300, 300, 2), (9, 333, 333, None), (9, 333, 334, 2), (10, 500, 500, None)]
    for svtype in ("DEL", "INS", "DUP"):
        seeds, exp = [], []
        for j, (apart, a, b, rule) in enumerate(table):
            seeds += _rep_pair(10 + FAR * j, apart, a, b)
            exp.append((0, svtype, "cmp", dict(outer=(apart + 1) * 100, inner=(apart - 1) * 100, rep=True, rule=rule), 1))
        c[f"crit2_repeat_option_{svtype}"] = case([(0, svtype, seeds)], cfg=dict(repeat=True), expect=exp)
        # the same under a tandem repeat that holds the first seed only / the second only, and without any
        trs = {0: [(s["bin"] * 100 - 1, s["bin"] * 100 + 1) for s in seeds[0:4:2]] + [(s["bin"] * 100 - 1, s["bin"] * 100 + 1) for s in seeds[5::2]]}
        exp_tr = [e if j < 4 else (0, svtype, "cmp", dict(outer=1100, rep=True, rule=None), 1) for j, e in enumerate(exp)]
        c[f"crit2_one_seed_in_a_repeat_{svtype}"] = case([(0, svtype, seeds), (1, svtype, seeds)], trs=trs,
                                                         expect=exp_tr + [(1, svtype, "cmp", dict(rep=False, rule=None), 2 * len(table) - 1)])
    # 150 leads: the mean is sum / 100.  150 x 200 -> 300, and (300 + 300) * 1.5 = 900 = outer merges; the mean of the leads (200) would not
    c["crit2_inflated_mean_150_leads"] = case([(0, "DEL", _rep_pair(10, 8, 200, 300, n_a=150) + _rep_pair(10 + FAR, 8, 300, 200, n_b=150) + _rep_pair(10 + 2 * FAR, 8, 200, 300, n_a=CAP))],
                                              cfg=dict(repeat=True),
                                              expect=[(0, "DEL", "cmp", dict(outer=900, mean_a=-300.0, mean_b=-300.0, rule=2), 2), (0, "DEL", "cmp", dict(outer=900, mean_a=-200.0, rule=None), 1)])
    # ... and of a MERGED cluster of 150 leads whose metrics come from added sums: D | a (100 x 200) + b (50 x 200) merge at index 1, mean 300,
    # and ab | c (3 x 300) at outer 900 merges; 151 leads of svlen 199 give 300.49 (merges), 149 give 296.51 (does not)
    for n_b, sv, rule in ((50, 200, 2), (51, 199, 2), (49, 199, None)):
        seeds = [three(2, 1), same(10, CAP, 0, sv), same(11, n_b, 0, sv), same(18, 3, 0, 300)]
        c[f"crit2_inflated_mean_of_{CAP + n_b}_merged_leads"] = case([(0, "DEL", seeds)], cfg=dict(repeat=True),
                                                                      expect=[(0, "DEL", "merge", dict(i=1, n_leads=CAP + n_b, step=1, mean=-sv * (CAP + n_b) / CAP), 1),
                                                                              (0, "DEL", "cmp", dict(i=1, outer=900, mean_b=-300.0, rule=rule), 1)])
    # the flag inherited through a merge decides a later comparison: D | a (in a repeat) + b by criterion 2 at index 1, then ab | c;
    # the second table has the repeat one base off a: nothing merges
    for name, tr, n in (("inherited", (1999, 2001), 2), ("not_inherited", (2000, 2002), 0)):
        seeds = [three(2, 1)] + _rep_pair(20, 4, 300, 300) + [same(28, 3, 0, 300)]
        c[f"crit2_repeat_flag_{name}"] = case([(0, "DUP", seeds)], trs={0: [tr]},
                                              expect=[(0, "DUP", "cmp", dict(rep=True, rule=2), n), (0, "DUP", "merge", dict(i=1), n)] +
                                                     ([(0, "DUP", "cmp", dict(i=1, outer=900, inner=300, rep=True, rule=2), 1)] if n else []))
    # cluster_repeat_h_max beyond int: seeds 500 bins apart merge by criterion 2 alone
    seeds = _rep_pair(10, 500, 100_000, 100_000) + _rep_pair(10 + 1000, 500, 10_000, 10_000)
    c["crit2_h_max_3e9"] = case([(0, "DEL", seeds)], cfg=dict(repeat=True, cluster_repeat_h_max=3e9), plan={None: 0, "0": 1, "100": 1, "-1": 0},
                                expect=[(0, "DEL", "cmp", dict(outer=50_100, rule=2), 1), (0, "DEL", "cmp", dict(outer=50_100, rule=None), 1)])
    return c


# ---------------------------------------------------------------------------------------------- (c) criterion 3
def _crit3():
    c = {}
    for bnd in (1000, 100, 5000):
        n = bnd // 100
        seeds = [same(10, 3), same(10 + n + 1, 3), same(10 + 2 * FAR + n, 3), same(10 + 2 * FAR + 2 * n + 2, 3)]
        guard = [(0, "DEL", _pairs([(40, 40)]))]
        c[f"crit3_bnd_{bnd}"] = case([(0, "BND", seeds)] + guard + [(1, "DEL", seeds)], cfg=dict(cluster_merge_bnd=bnd) if bnd != 1000 else {},
                                     expect=[(0, "BND", "cmp", dict(inner=bnd, rule=3), 1), (0, "BND", "cmp", dict(inner=bnd + 100, rule=None), 1),
                                             (1, "DEL", "cmp", dict(inner=bnd, rule=None), 1)])
    return c


# ---------------------------------------------------------------------------------------------- (d) the repeat lookup
def _repeats():
    """Pairs a (at A) / b (at A + 800, outer 900, svlen 300 + 300): they merge iff a carries the flag."""
    places = [  # (name, repeats relative to A, tr_index the sweep is on at a, within)
        ("in_front_of_the_first", [], 0, False),
        ("inside", [(-1, 1)], 0, True),
        ("on_tr_start", [(0, 1)], 1, False),
        ("on_tr_end", [(-1, 0)], 2, False),
        ("one_behind_tr_end", [(-5, -1)], 4, False),          # (the sweep leaves it for the next repeat, which begins behind the seed)
        ("one_in_front_of_tr_start", [(1, 5)], 4, False),
        ("between_two", [(-300, -200), (1, 799)], 6, False),
        ("long_holds_a_later_short", [(-5000, 5000), (-100, -50)], 7, True),
        ("equal_ends", [(-10, 1), (-5, 1)], 9, True),
        ("behind_the_last", [], 10, False),
    ]
    seeds, trs, exp = [], [], []
    for j, (name, rel, idx, within) in enumerate(places):
        A = (100 + 2 * FAR * j) * 100
        seeds += _rep_pair(A // 100, 8, 300, 300)
        trs += [(A + s, A + e) for s, e in rel]
        exp += [(0, "DEL", "tr", dict(seed=A, tr_index=idx, within=within), 1)]
    exp += [(0, "DEL", "cmp", dict(outer=900, rule=2), sum(p[3] for p in places)), (0, "DEL", "cmp", dict(outer=900, rule=None), sum(not p[3] for p in places))]
    assert trs == sorted(trs)
    # (task 3: the repeats of the tasks lie one behind the other in one table - what follows task 0's last repeat there is a repeat
    # around the coordinate of task 0's seed `behind_the_last`)
    c = {"repeat_lookup_borders": case([(0, "DEL", seeds), (0, "INS", seeds), (1, "DEL", seeds[:4]), (2, "DEL", seeds[:4]), (3, "DEL", seeds[:4])], trs={0: trs, 1: [], 3: [(A - 1, A + 1)]},
                                       expect=exp + [(t, "DEL", "cmp", dict(outer=900, rep=False, rule=None), 2) for t in (1, 2, 3)])}
    return c


# ---------------------------------------------------------------------------------------------- (e) the index rule
WIDE = [same(0, 3, 0), same(1, 3, 99)]          # two adjacent bins (inner 0: they merge) whose union has sd 108.4


def _at(seeds, b):
    return [dict(s, bin=s["bin"] + b) for s in seeds]


def _index_chain(front):
    """`front` clusters that merge with nothing (k = 1, five bins apart), then p (k = 40) | a0 a1 (adjacent, merged sd > 40) | c (k = 40),
    inner 100 on both sides: a0 + a1 merge at list index front + 1, and what is compared next is the index rule."""
    b = 10 + 6 * front
    return [three(10 + 6 * j, 1) for j in range(front)] + [three(b, 40, at=5)] + _at([same(0, 3, 98), same(1, 3, 99)], b + 2) + [three(b + 5, 40)]


def _index():
    c = {}
    # a merge at list index 0 is not compared again: a0 a1 | c (k = 40, inner 100) stay apart although a | c would merge
    c["index_merge_at_0_not_rechecked"] = case([(0, "DEL", _at(WIDE, 10) + [three(13, 40)]), (0, "DUP", [three(2, 1)] + _at(WIDE, 10) + [three(13, 40)])],
                                               expect=[(0, "DEL", "merge", dict(i=0, sd=lambda x: x > 100), 1), (0, "DEL", "cmp", {}, 1),
                                                       (0, "DUP", "merge", dict(i=1), 2), (0, "DUP", "cmp", dict(i=1, inner=100, rule=1), 1)])
    # p | a0: a0 has sd 0, no merge; a0 + a1 merge at index 1 / 2 / 3; at 1 the scan stays (a | c merges, p stays out - p was index 0),
    # at 2 and 3 it steps back: p | a merges, and then at index 1 (stay) / 2 (step back once more) pa | c
    for front in (0, 1, 2):
        i = front + 1
        exp = [(0, "DEL", "merge", dict(i=i, n_leads=6), 1)]
        exp += [(0, "DEL", "cmp", dict(i=i - 1, inner=100, sd_a=40.0, sd_b=lambda x: x > 40, rule=1), 1 if front else 0)]
        c[f"index_merge_at_{i}"] = case([(0, "DEL", _index_chain(front))], expect=exp)
    # the same chains as a later run of their group: behind a cut (inner 2 000) that follows one cluster / three clusters
    for first_run in (1, 3):
        head = [three(2 + 4 * j, 1) for j in range(first_run)]
        for front in (0, 1, 2):
            c[f"index_merge_at_{front + 1}_behind_a_run_of_{first_run}"] = case([(0, "DEL", head + _at(_index_chain(front), 30))],
                                                                                 expect=[(0, "DEL", "merge", dict(i=first_run + front + 1, n_leads=6), 1)], plan={None: 0})
        c[f"index_merge_at_run_start_behind_a_run_of_{first_run}"] = case([(0, "DEL", head + _at(WIDE, 40) + [three(43, 40)])], plan={None: 0},
                                                                          expect=[(0, "DEL", "merge", dict(i=first_run), 2)])
    return c


# ---------------------------------------------------------------------------------------------- (f) run cuts
BLOB = dict(n=CAP, off=40)          # a bin of 100 leads at one position: absorbed, it pulls sd and mean of its cluster down


def _cuts():
    c = {}
    # provably safe / merged across by the serial scan: k = 39 / 40 across inner = 100, cut under SNF_RUN_GAP=0 only
    c["cut_safe_k39"] = case([(0, "DEL", _pairs([(39, 39)]))], plan={None: 0, "0": 0, "100": 0, "-1": 0}, expect=[(0, "DEL", "cmp", dict(inner=100, rule=None), 1)])
    c["cut_merged_across_k40"] = case([(0, "DEL", _pairs([(40, 40)]))], plan={None: 0, "0": 1, "100": 0, "-1": 0}, expect=[(0, "DEL", "cmp", dict(inner=100, rule=1), 1)])
    # the first cluster of a run merges with the run in front in its INITIAL state only: b (k = 40) absorbs a bin of 100 leads at one
    # position, sd 40 -> 7.9.  The serial scan merges a + b first (index 0) and leaves the blob alone
    c["cut_first_state_stdev"] = case([(0, "DEL", [three(10, 40), three(12, 40), same(13, BLOB["n"], BLOB["off"])])], plan={None: 0, "0": 1, "100": 0, "-1": 0},
                                      expect=[(0, "DEL", "merge", dict(i=0, n_leads=6), 1), (0, "DEL", "cmp", {}, 1)])
    # ... by |mean| under a repeat: b (svlen 300) absorbs 100 leads of svlen 10, mean 300 -> 19
    c["cut_first_state_absmean"] = case([(0, "DEL", _rep_pair(10, 8, 300, 300) + [same(19, BLOB["n"], 0, 10)])], cfg=dict(repeat=True), plan={None: 0, "0": 1, "100": 1, "-1": 0},
                                        expect=[(0, "DEL", "cmp", dict(i=0, outer=900, rule=2), 1), (0, "DEL", "cmp", {}, 1)])
    # ... by the flag, which only grows: D | a | b + b' (b' in a repeat): b + b' merge at index 2, the step back merges a | bb' by criterion 2
    c["cut_first_state_repeat"] = case([(0, "DEL", [three(2, 1)] + _rep_pair(20, 7, 300, 300) + [same(28, 3, 0, 300)])], trs={0: [(2799, 2801)]},
                                       plan={None: 0, "0": 1, "100": 1, "-1": 0},
                                       expect=[(0, "DEL", "cmp", dict(i=1, rep=False, rule=None), 1), (0, "DEL", "cmp", dict(i=1, rep=True, outer=900, rule=2), 1)])
    # the default run_gap itself: binsize 1000, r = 5, k = 399 / 400 across inner = 2000 > 1000
    for k, dirty in ((399, 0), (400, 1)):
        c[f"cut_default_gap_k{k}"] = case([(0, "DEL", _pairs([(k, k)], gap_bins=3))], bs=1000, cfg=dict(cluster_r=5.0), plan={None: dirty, "0": dirty, "100": dirty, "-1": 0},
                                          expect=[(0, "DEL", "cmp", dict(inner=2000, rule=1 if dirty else None), 1)])
    # inner = run_gap: not cut; one bin more: cut (the run counts say which)
    c["cut_inner_equals_run_gap"] = case([(0, "DEL", _pairs([(1, 1)], gap_bins=11) + _pairs([(1, 1)], gap_bins=12, base=10 + 2 * FAR)), (0, "INV", _pairs([(1, 1)], gap_bins=2) + _pairs([(1, 1)], gap_bins=3, base=10 + 2 * FAR))],
                                         plan={None: 0, "0": 0, "100": 0, "-1": 0},
                                         expect=[(0, "DEL", "cmp", dict(inner=1000), 1), (0, "DEL", "cmp", dict(inner=1100), 1), (0, "INV", "cmp", dict(inner=100), 1), (0, "INV", "cmp", dict(inner=200), 1)])
    # a boundary the serial scan never compares - the merged index-0 cluster, then a cut: redone, and the same result
    c["cut_behind_merged_index_0"] = case([(0, "DEL", _at(WIDE, 10) + [three(13, 40)])], plan={None: 0, "0": 1, "100": 0, "-1": 0}, expect=[(0, "DEL", "cmp", {}, 1)])
    # a redone group reads the leads at every merge (its seeds carry no sums any more): the union of two seeds whose sd stays just below
    # 40, so that c does not merge, in a group that a pair k = 40 / 40 elsewhere makes dirty
    d = _sd_flip(CAP - 1, 2) - 1
    c["cut_redone_group_reads_the_leads"] = case([(0, "DEL", _merged(CAP - 1, 2, d) + _pairs([(40, 40)], base=10 + 2 * FAR))], plan={None: 0, "0": 1, "100": 0, "-1": 0},
                                                 expect=[(0, "DEL", "cmp", dict(i=1, inner=100, sd_a=lambda x: 39 < x < 40, sd_b=40.0, rule=None), 1)])
    # two groups redone and one not, in one task; an empty task between two others
    c["cut_two_dirty_one_clean"] = case([(0, "DEL", _pairs([(40, 40)])), (0, "INS", _pairs([(41, 40)])), (0, "DUP", _pairs([(39, 40)]))], plan={None: 0, "0": 2, "100": 0, "-1": 0})
    c["cut_empty_task_between"] = case([(0, "DEL", _pairs([(40, 40)])), (2, "DEL", _pairs([(40, 40), (39, 39)]))], n_tasks=3, plan={None: 0, "0": 2, "100": 0, "-1": 0})
    return c


# ---------------------------------------------------------------------------------------------- (g) added sums and compute_metrics
def _split(n, parts):
    q = [n // parts + (1 if j < n % parts else 0) for j in range(parts)]
    assert sum(q) == n and min(q) >= 1
    return q


def _merged(n, parts, d):
    """D | `parts` adjacent bins of n leads in all, each at one position, the first and the last d bp apart | c (k = 40, inner 100):
    the parts merge at index 1 and the union's sd decides about c."""
    q = _split(n, parts) if parts == 2 else [n // 8, n - 2 * (n // 8), n // 8]      # (three: most leads in the middle, sd about d / 4)
    offs = [99, (99 + d) % 100] if parts == 2 else [99, (99 + d // 2) % 100, (99 + d) % 100]
    bins = [0, (99 + d) // 100] if parts == 2 else [0, (99 + d // 2) // 100, (99 + d) // 100]
    assert bins == list(range(parts)), (d, bins)
    return [three(2, 1)] + [same(10 + bins[j], q[j], offs[j]) for j in range(parts)] + [three(10 + parts + 1, 40)]


def _sd_flip(n, parts):
    """The smallest d for which the union of _merged(n, parts, d) reaches the sd (40) that merges c, from the restatement."""
    for d in range(102 if parts == 3 else 2, 199):
        cs = case([(0, "DEL", _merged(n, parts, d))])
        tr = ref.batch_clusters(build(cs), config(cs))[1][(0, "DEL")]
        if ref.has(tr, "cmp", i=1, inner=100, rule=1):
            return d
    raise AssertionError((n, parts))


def _sums():
    c = {}
    for n in (CAP - 1, CAP, CAP + 1, ADDED - 1, ADDED, ADDED + 1, 3 * CAP - 1, 3 * CAP, 3 * CAP + 1):
        for parts in (2, 3):
            d = _sd_flip(n, parts)
            groups, exp = [], []
            for sv, dd, rule in (("DEL", d, 1), ("DUP", d - 1, None)):
                groups.append((0, sv, _merged(n, parts, dd)))
                exp += [(0, sv, "merge", dict(i=1, n_leads=n, step=n // min(n, CAP), n_samples=len(range(0, n, n // min(n, CAP)))), 1), (0, sv, "cmp", dict(i=1, inner=100, sd_b=40.0, rule=rule), 1)]
            c[f"sums_merged_{n}_from_{parts}"] = case(groups, expect=exp)
    # 200 leads of which every second differs from all: seeds a / b of 100 leads whose even-numbered leads lie 1 bp apart (1099 / 1100) and
    # whose odd-numbered ones 199 bp (1000 / 1199).  199 leads are all read (sd 70: c merges), of 200 the even-numbered only (sd 0.5: it does not)
    for n_b, rule in ((CAP - 1, 1), (CAP, None)):
        seeds = [three(2, 1), S(10, [99 * (1 - i % 2) for i in range(CAP)]), S(11, [99 * (i % 2) for i in range(n_b)]), three(13, 40)]
        c[f"sums_merged_{CAP + n_b}_every_second_lead_differs"] = case([(0, "DEL", seeds)], expect=[(0, "DEL", "merge", dict(i=1, n_leads=CAP + n_b, step=(CAP + n_b) // CAP), 1),
                                                                                                    (0, "DEL", "cmp", dict(i=1, inner=100, sd_b=40.0, rule=rule), 1)])
    # parts whose leads are spread (S1 of the joining part is not 0: the cross term 2 dx S1 counts): a 50 leads, b 49 leads over 20 bp
    # each, b shifted until the union's sd reaches 40
    spread = lambda sh: [three(2, 1), S(10, [99 - i % 20 for i in range(50)]), S(11, [sh + i % 20 for i in range(49)]), three(13, 40)]
    flip = next(sh for sh in range(1, 79) if ref.has(ref.resolve("DEL", [(x["bin"] * 100, [(x["bin"] * 100 + o, -300, 0) for o in x["offs"]]) for x in spread(sh)], None, SnifflesConfig())[1],
                                                     "cmp", i=1, inner=100, rule=1))
    c["sums_merged_99_spread_parts"] = case([(0, "DEL", spread(flip)), (0, "DUP", spread(flip - 1))],
                                            expect=[(0, "DEL", "cmp", dict(i=1, inner=100, sd_b=40.0, rule=1), 1), (0, "DUP", "cmp", dict(i=1, inner=100, sd_b=40.0, rule=None), 1)])
    # single seeds of every batch length of the request loop, each with a neighbour k = 40 at inner 100.  Below the sample cap the leads
    # alternate between offsets 0 and 79 (sd 39.5 sqrt(n / (n - 1)): on either side of 40 as n grows); from the cap on between 0 and 81
    # in pairs, so that every second lead (step 2) still meets both and sd stays above 40
    sizes = [1, 2, MCH - 1, MCH, MCH + 1, 2 * MCH - 1, 2 * MCH, 2 * MCH + 1, CAP - 1, CAP, CAP + 1, ADDED - 1, ADDED]
    seeds = []
    for j, n in enumerate(sizes):
        seeds += [S(10 + FAR * j, [79 * (i % 2) if n < CAP else 81 * (i % 4 // 2) for i in range(n)], [300 + i % 7 for i in range(n)]), three(12 + FAR * j, 40)]
    c["sums_single_seeds"] = case([(0, "DEL", seeds)], cfg=dict(dev_min_leads_cluster=1),
                                  expect=[(0, "DEL", "cmp", dict(inner=100, rule=1), None), (0, "DEL", "cmp", dict(inner=100, rule=None), None),
                                          (0, "DEL", "merge", dict(n_leads=ADDED + 3, step=2), 1), (0, "DEL", "merge", dict(n_leads=ADDED + 2, step=2), 1)])
    # a seed of 200 leads (it carries no sums) merging with one of 10; INS seeds with leads without a length interleaved
    c["sums_seed_of_200_and_10"] = case([(0, "DEL", [three(2, 1), S(10, [i % 90 for i in range(ADDED)]), S(11, [3 * i for i in range(10)]), three(13, 40)])],
                                        expect=[(0, "DEL", "merge", dict(i=1, n_leads=ADDED + 10, step=2), 1)])
    c["sums_ins_long_leads_interleaved"] = case([(0, "INS", [three(2, 1), S(10, [i % 50 for i in range(40)], long_every=3), S(11, [50 + i % 50 for i in range(30)], long_every=2),
                                                             S(12, [1, 2, 3], long_every=1), three(13, 40)])],
                                                expect=[(0, "INS", "merge", dict(i=1, n_leads=40 - 14 + 15), 1)])
    # ineligible bins (one lead) between two seeds that merge by criterion 2
    c["sums_ineligible_bins_between"] = case([(0, "DEL", [same(10, 3, 0, 300), same(13, 1), same(15, 1), same(18, 3, 0, 300), same(19, 1), same(20, 4, 0, 300)])], cfg=dict(repeat=True),
                                             expect=[(0, "DEL", "cmp", dict(outer=900, rule=2), 1), (0, "DEL", "merge", dict(n_leads=6), 1)])
    return c


def _wide():
    """Positions further apart than the 64-bit sums hold (few leads, far apart)."""
    c = {}
    # S2m on either side of 2^fits_shift: D (sd 0: merges with nothing) | a | b, dx apart, merge at index 1 under a cluster_r that bridges
    # anything.  a: three leads, k = 1 (S2 = 5); b: 150 leads alternating between two neighbouring positions (S1 = S2 = 75; so many that a contig of 180 Mb
    # is long enough): the added S2 is 5 + 75 + 2 dx 75 + 150 dx^2.  c right behind b merges next and must read the leads where the sums were dropped.  cluster_merge_bnd lifts
    # run_gap above dx: no cut, the sums are in use.  Bins of 1 000 bp keep the bin table small
    lim, nb = 1 << T["fits_shift"], 150
    s2m = lambda x: 5 + nb // 2 + 2 * x * (nb // 2) + nb * x * x
    dx = next(x for x in range(175_000_000, 176_000_000, 1000) if s2m(x) >= lim)
    for name, x in (("below", dx - 1000), ("above", dx)):
        assert (s2m(x) >= lim) == (name == "above") and x % 1000 == 0 and nb + 6 < ADDED
        seeds = [same(2, 3), three(40, 1), S(40 + x // 1000, [i % 2 for i in range(nb)]), three(41 + x // 1000, 1)]
        c[f"wide_added_s2_{name}_the_bound"] = case([(0, "DEL", seeds)], cfg=dict(cluster_r=2e9, cluster_merge_bnd=2_000_000_000), bs=1000, contig_len=180_000_000,
                                                    expect=[(0, "DEL", "merge", dict(i=1, n_leads=nb + 3), 1), (0, "DEL", "merge", dict(i=1, n_leads=nb + 6), 1)], forms=("default", "reread", "nofuse"))
    # deviations of 2^wide_shift - 1 / 2^wide_shift inside one seed, with a neighbour whose merge depends on that seed's sd: bins of
    # 140 Mb (a little more than 2^27 bp) on a contig of three, a three-lead seed in bin 0 and a like one in bin 2 (inner = one bin), and
    # a cluster_r that puts min(sd) * r a few parts in 10^9 on either side of inner - so the sd must be right to nine digits
    w, bs = 1 << T["wide_shift"], 140_000_000
    for name, dev in (("last_narrow", w - 1), ("first_wide", w)):
        # (DEL: the seed whose sd decides - the smaller one, its third lead in the middle - has its first lead leftmost, the deviations are
        # positive; DUP: rightmost, they are negative.  The other seed of each group is the mirror image with its third lead near one end:
        # an sd 15 % larger, which decides - wrongly - as soon as the first seed's sd comes out too large)
        seeds = [S(0, [5000, 5000 + dev, 5000 + dev // 2]), S(2, [5000 + dev, 5000, 6000])]
        mirror = [S(0, [5000 + dev, 5000, 5000 + dev - dev // 2]), S(2, [5000, 5000 + dev, 6000])]
        pos = lambda x: [(x["bin"] * bs + o, -300, 0) for o in x["offs"]]
        cl = [ref.Cl(0, 0, pos(x), False, None) for x in seeds]
        for x in cl:
            x.compute_metrics()
        sd = min(x.stdev_start for x in cl)
        assert max(abs(p[0] - x.leads[0][0]) for x in cl for p in x.leads) == dev and sd == cl[0].stdev_start
        for side, r, rule in (("merges", bs / sd * (1 + 4e-9), 1), ("stays", bs / sd * (1 - 4e-9), None)):
            c[f"wide_deviation_{name}_{side}"] = case([(0, "DEL", seeds), (0, "DUP", mirror)], bs=bs, contig_len=3 * bs, cfg=dict(cluster_r=r),
                                                      expect=[(0, sv, "cmp", dict(i=0, inner=bs, sd_a=sd, rule=rule), 1) for sv in ("DEL", "DUP")], forms=("default", "reread", "nofuse"))
    return c


for _f in (_crit1, _crit2, _crit3, _repeats, _index, _cuts, _sums, _wide):
    for _k, _v in _f().items():
        assert _k not in CASES
        CASES[_k] = _v
CUT_CASES = sorted(k for k, v in CASES.items() if v["plan"] and set(v["plan"]) == set(GAPS))


# ---------------------------------------------------------------------------------------------- (h) the small space, whole
SPACE_K, SPACE_GAPS, SPACE_SEEDS = (1, 39, 40), (1, 2, 3), 5
SPACE_N = len(SPACE_K) ** SPACE_SEEDS * len(SPACE_GAPS) ** (SPACE_SEEDS - 1)          # 19 683 groups of 15 leads
SPACE_PER_TASK = 60                                                                     # groups of one type in a task


def space_group(g):
    """Group g of the space: five three-lead seeds, k of each and the bins between them as the digits of g."""
    seeds, b = [], 0
    for j in range(SPACE_SEEDS):
        g, kd = divmod(g, len(SPACE_K))
        seeds.append((b, SPACE_K[kd]))
        if j + 1 < SPACE_SEEDS:
            g, gd = divmod(g, len(SPACE_GAPS))
            b += SPACE_GAPS[gd]
    return seeds


def space_tasks(ids):
    """The groups `ids` as tasks of 3 x SPACE_PER_TASK groups (DEL, DUP, INV), 40 bins apart: built as columns, without a dict per lead."""
    per = 3 * SPACE_PER_TASK
    tis = []
    for t0 in range(0, len(ids), per):
        chunk = ids[t0:t0 + per]
        leads = []
        for j, g in enumerate(chunk):
            svtype = ("DEL", "DUP", "INV")[j % 3]
            base = 10 + 40 * (j // 3)
            for si, (b, k) in enumerate(space_group(g)):
                for i in range(3):
                    leads.append(_lead(svtype, (base + b) * 100 + i * k, None, f"h{j}_{si}_{i}", i, si, False))
        L = (10 + 40 * SPACE_PER_TASK + FAR) * 100
        tis.append(cases.mk_task(leads, cases._reads(24, 0, L), L, task_id=len(tis), contig=f"chrH{len(tis)}"))
    return tis
