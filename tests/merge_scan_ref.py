"""A plain restatement of the reference's seed stage and adaptive merge scan - Cluster.compute_metrics (cluster.py:48-61) and the seed,
repeat and merge part of cluster.resolve (cluster.py:219-308) - that says WHY it decided what it decided.

It works on Python ints, `statistics.stdev` and the reference's own float expressions, one (task, svtype) sequence at a time, and shares
nothing with sniffles_amd/csrc: the directed cases of tests/merge_scan_cases.py are planned on its trace (a case that no longer sits on
the comparison it was written for fails when its table is built), and tests/test_merge_scan_edges.py compares the library's clusters
with its clusters.  tests/golden/merge_scan_edges.json.gz holds the unmodified reference's clusters for the same tables, so the
restatement itself is held against cluster.resolve with and without the reference at hand.

    bins    [(seed, [(ref_start, svlen or None, row), ...]), ...]     every occupied bin of the sequence, leads in arrival order
    trs     None, or [(start, end), ...]                               the task's tandem repeats
    cfg     anything with the reference's option names

The trace holds one tuple per repeat lookup, per comparison and per merge:
    ("tr", seed, tr_index, within)
    ("cmp", i, inner, outer, sd_a, sd_b, mean_a, mean_b, rep, rule)     rule: 1 / 2 / 3 the criterion that merged, None: no merge
    ("merge", i, n_leads, step, n_samples, mean, sd)                     the merged cluster as compute_metrics left it
"""
import statistics

from sniffles_amd.soa import SVLEN_NONE, SVTYPES, SVT

MAX_N = 100          # compute_metrics(max_n=100)


class Cl:
    def __init__(self, start, end, leads, repeat, leads_long):
        self.start, self.end, self.leads, self.repeat, self.leads_long = start, end, leads, repeat, leads_long
        self.mean_svlen = self.stdev_start = None
        self.step = self.n_samples = 0

    def compute_metrics(self):
        n = min(len(self.leads), MAX_N)
        if n == 0:
            self.mean_svlen, self.stdev_start, self.step, self.n_samples = 0, 0, 0, 0
            return
        step = int(len(self.leads) / n)
        picked = range(0, len(self.leads), step)
        self.step, self.n_samples = step, len(picked)
        if n > 1:
            self.mean_svlen = sum(self.leads[i][1] for i in picked) / float(n)
            self.stdev_start = statistics.stdev(self.leads[i][0] for i in picked)
        else:
            self.mean_svlen = self.leads[0][1]
            self.stdev_start = 0


def resolve(svtype, bins, trs, cfg, scan=True):
    """-> (clusters, trace); a cluster is dict(start, end, repeat, n_leads_long, leads [row ...], svlens [...])."""
    trace = []
    seeds = sorted(s for s, _ in bins)
    table = dict(bins)
    assert len(table) == len(bins)
    if not seeds:
        return [], trace
    tr = trs
    tr_index = 0
    if tr is not None:
        if len(tr) == 0:
            tr = None
        else:
            tr_start, tr_end = tr[tr_index]
    clusters = []
    for seed in seeds:
        within = False
        if tr is not None and tr_index < len(tr):
            while tr_end < seed and tr_index + 1 < len(tr):
                tr_index += 1
                tr_start, tr_end = tr[tr_index]
            if tr_start < seed < tr_end:
                within = True
            trace.append(("tr", seed, tr_index, within))
        if svtype == "INS":
            leads = [ld for ld in table[seed] if ld[1] is not None]
            leads_long = [ld for ld in table[seed] if ld[1] is None]
        else:
            leads, leads_long = list(table[seed]), None
        if len(leads) >= cfg.dev_min_leads_cluster:
            c = Cl(seed, seed + cfg.cluster_binsize, leads, within or cfg.repeat, leads_long)
            c.compute_metrics()
            clusters.append(c)
    i = 0
    while scan and i < len(clusters) - 1:
        a, b = clusters[i], clusters[i + 1]
        inner = b.start - a.end
        outer = b.end - a.start
        rule = None
        if inner <= min(a.stdev_start, b.stdev_start) * cfg.cluster_r:
            rule = 1
        elif (cfg.repeat or a.repeat or b.repeat) and outer <= min(cfg.cluster_repeat_h_max, (abs(a.mean_svlen) + abs(b.mean_svlen)) * cfg.cluster_repeat_h):
            rule = 2
        elif svtype == "BND" and inner <= cfg.cluster_merge_bnd:
            rule = 3
        trace.append(("cmp", i, inner, outer, a.stdev_start, b.stdev_start, a.mean_svlen, b.mean_svlen, bool(cfg.repeat or a.repeat or b.repeat), rule))
        if rule is not None:
            clusters.pop(i + 1)
            a.leads += b.leads
            if svtype == "INS":
                a.leads_long += b.leads_long
            a.end = b.end
            a.repeat = a.repeat or b.repeat
            a.compute_metrics()
            trace.append(("merge", i, len(a.leads), a.step, a.n_samples, a.mean_svlen, a.stdev_start))
            i = max(0, i - 2)
        i += 1
    out = [dict(start=c.start, end=c.end, repeat=bool(c.repeat), n_leads_long=len(c.leads_long) if c.leads_long is not None else 0,
                leads=[ld[2] for ld in c.leads], svlens=[ld[1] for ld in c.leads]) for c in clusters]
    return out, trace


def seed_clusters(svtype, bins, trs, cfg):
    """The seed clusters before the scan (fetch_clusters(0))."""
    return resolve(svtype, bins, trs, cfg, scan=False)[0]


# ---------------------------------------------------------------------------------------------- tasks in, columns out
def task_bins(ti, cfg):
    """{svtype name: bins} of one TaskInput: the lead table as LeadProvider.record_lead fills it (leads outside the contig dropped)."""
    L = ti.leads
    out = {}
    bs = cfg.cluster_binsize
    for row in range(len(L["ref_start"])):
        rs = int(L["ref_start"][row])
        if not 0 <= rs < ti.contig_len:
            continue
        sv = int(L["svlen"][row])
        name = SVTYPES[int(L["svtype"][row])]
        out.setdefault(name, {}).setdefault(rs // bs * bs, []).append((rs, None if sv == int(SVLEN_NONE) else sv, row))
    return {k: sorted(v.items()) for k, v in out.items()}


def task_trs(ti):
    return None if ti.tr_start is None else [(int(a), int(b)) for a, b in zip(ti.tr_start, ti.tr_end)]


def batch_clusters(tis, cfg, stage=1):
    """[(task index, svtype index, start, end, repeat, n_leads_long, (rows ...), (svlens ...))] in the order of Batch.fetch_clusters, and
    {(task index, svtype name): trace}."""
    rows, traces = [], {}
    for t, ti in enumerate(tis):
        bins = task_bins(ti, cfg)
        for name in SVTYPES:
            if name not in bins:
                continue
            if stage == 0:
                cl, tr = seed_clusters(name, bins[name], task_trs(ti), cfg), []
            else:
                cl, tr = resolve(name, bins[name], task_trs(ti), cfg)
            traces[(t, name)] = tr
            rows += [(t, SVT[name], c["start"], c["end"], c["repeat"], c["n_leads_long"], tuple(c["leads"]), tuple(c["svlens"])) for c in cl]
    return rows, traces


def library_clusters(cols):
    """The same rows from the columns of Batch.fetch_clusters."""
    off = cols["lead_off"]
    return [(int(cols["task_index"][k]), int(cols["svtype"][k]), int(cols["start"][k]), int(cols["end"][k]), bool(cols["repeat"][k]),
             int(cols["n_leads_long"][k]), tuple(int(x) for x in cols["lead"][off[k]:off[k + 1]]),
             tuple(int(x) for x in cols["lead_svlen"][off[k]:off[k + 1]])) for k in range(len(cols["start"]))]


def has(trace, kind, **want):
    """The tuples of `trace` of one kind whose named fields have the wanted values (a callable: a predicate on the field)."""
    names = dict(tr=("seed", "tr_index", "within"), cmp=("i", "inner", "outer", "sd_a", "sd_b", "mean_a", "mean_b", "rep", "rule"),
                 merge=("i", "n_leads", "step", "n_samples", "mean", "sd"))[kind]
    out = []
    for t in trace:
        if t[0] != kind:
            continue
        d = dict(zip(names, t[1:]))
        if all(v(d[k]) if callable(v) else d[k] == v for k, v in want.items()):
            out.append(d)
    return out

