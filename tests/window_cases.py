"""Builders for the directed cases of the window front end (snf_stage_window.h; tests/test_window_edges.py runs them, three tables
are registered in tests/cases.py with fixtures from the unmodified reference).

The front end buckets the leads of a batch by WINDOW - 2^W consecutive bins of one (task, svtype) - and hands every 64 positions of
the bucket array to one wave, so what a wave meets is decided by where in that array a window begins and ends.  The bucket order is
known without running anything: task, then svtype in soa.SVTYPES order, then window, ascending; leads outside their contig have no
window.  A PLAN is a list of entries

    (task, svtype, bin, n leads, kind)          or          (task, svtype, bin, n leads, kind, name)

`bin` the bin of `cluster_binsize` bp all n leads lie in, `kind` what the leads are:
    plain      n leads of cases._ladder_lead
    long4      INS: leads 0, 4, 8 ... in ARRIVAL order carry no length (svlen None: `leads_long`), so the seed lead of the bin is long
    long       INS: no lead carries a length
    len:k      INS: the LAST k leads in arrival order carry a length, the others none
    hap        plain leads with hap 0 / 1 / 2 in turn and a phase set
    ins20      INS leads whose sequences differ from the allele in every fifth base: a vote over fewer of them gives another string
    at:p       plain leads at ref_start p exactly (p < 0 or p >= contig_len: the lead is dropped and has no window; `bin` is ignored)
A batch is a list of SECTIONS (order, entries): the leads of a section arrive in the order `plan` (entry after entry), `shuffle`
(seeded permutation - the rank sort of a window then has work to do) or `robin` (one lead of every entry in turn); the sections of a
task arrive one after the other.  layout() computes from the plan alone what the handle must report for a width W."""
import numpy as np

import cases
import size_classes as sc
from sniffles_amd.soa import SVTYPES, SVT

NTYPES = len(SVTYPES)


def _lead(e, i, rng, bs, contig_len, allele, tag):
    task, svtype, b, n, kind = e[:5]
    base = kind.split(":")[0]
    d = cases._ladder_lead(svtype, rng, 0, f"{tag}_{i}", i, allele, abs(b or 0) % 50)
    if base == "at":
        d["ref_start"] = int(kind.split(":")[1])
    else:
        assert b * bs < contig_len, (e, contig_len)
        d["ref_start"] = b * bs + (7 * i + 3) % min(bs, 30, contig_len - b * bs)      # (the contig's last bin may be a few bases long)
    if base in ("long4", "long", "len"):
        assert svtype == "INS"
        is_long = (i % 4 == 0) if base == "long4" else True if base == "long" else i < n - int(kind.split(":")[1])
        if is_long:
            d.update(svlen=None, seq=None)
    elif base == "hap":
        d.update(hap=i % 3, ps=f"P{task}" if i % 3 else "NULL")
    elif base == "ins20":
        assert svtype == "INS"
        d["seq"] = cases._mutate(rng, allele, 0.2)
    else:
        assert base in ("plain", "at"), kind
    return d


def is_valid(e, bs, contig_len):
    if not e[4].startswith("at:"):
        return True
    p = int(e[4].split(":")[1])
    return 0 <= p < contig_len


def bin_of(e, bs):
    return int(e[4].split(":")[1]) // bs if e[4].startswith("at:") else e[2]


def build(sections, contig_len, n_tasks=None, bs=100, seed=0, depth=24):
    """The tasks of a batch.  contig_len: one length or {task: length}."""
    entries = [e for _, es in sections for e in es]
    T = n_tasks if n_tasks is not None else 1 + max(e[0] for e in entries)
    clen = lambda t: contig_len[t] if isinstance(contig_len, dict) else contig_len
    rng = np.random.default_rng([seed, 4007])
    allele = cases._rng_seq(rng, 90)
    per_task = [[] for _ in range(T)]
    k = 0
    for order, es in sections:
        slots = [[] for _ in range(T)]                      # (entry number, entry) per lead, in arrival order
        if order == "robin":
            left = [e[3] for e in es]
            while any(left):
                for j, e in enumerate(es):
                    if left[j]:
                        left[j] -= 1
                        slots[e[0]].append((k + j, e))
        else:
            for j, e in enumerate(es):
                slots[e[0]] += [(k + j, e)] * e[3]
            if order == "shuffle":
                slots = [[s[i] for i in rng.permutation(len(s))] for s in slots]
            else:
                assert order == "plan", order
        k += len(es)
        for t in range(T):
            seen = {}
            for num, e in slots[t]:
                i = seen.get(num, 0)
                seen[num] = i + 1
                per_task[t].append(_lead(e, i, rng, bs, clen(t), allele, f"t{t}e{num}"))
    tis = []
    for t in range(T):
        L = clen(t)
        reads = cases._reads(depth, 0, L) + cases._reads(7, 0, max(1, L // 2), 1) + cases._reads(5, L // 3, L, 2)
        tis.append(cases.mk_task(per_task[t], reads, L, task_id=t, contig=f"chrW{t}"))
    return tis


def layout(sections, W, contig_len, n_tasks=None, bs=100):
    """What the front end forms for window width W, from the plan alone: dict(W, NW window slots, N leads, n_valid leads inside their
    contig, occupied windows, largest window, big64 windows of more than 64 leads, start {name: first bucket position of the window
    of a named entry}, wins [(first position, leads)] ascending)."""
    entries = [e for _, es in sections for e in es]
    T = n_tasks if n_tasks is not None else 1 + max(e[0] for e in entries)
    clen = lambda t: contig_len[t] if isinstance(contig_len, dict) else contig_len
    wins = {}
    for e in entries:
        if is_valid(e, bs, clen(e[0])):
            key = (e[0], SVT[e[1]], bin_of(e, bs) >> W)
            assert key[2] < (((clen(e[0]) // bs + 1) >> W) + 1)
            wins[key] = wins.get(key, 0) + e[3]
    start, pos = {}, 0
    for key in sorted(wins):
        start[key] = pos
        pos += wins[key]
    named = {e[5]: start[(e[0], SVT[e[1]], bin_of(e, bs) >> W)] for e in entries if len(e) > 5}
    counts = [c for c in wins.values() if c]
    return dict(W=W, NW=sum(NTYPES * ((((clen(t) // bs) + 1) >> W) + 1) for t in range(T)), N=sum(e[3] for e in entries), n_valid=pos,
                occupied=len(counts), largest=max(counts, default=0), big64=sum(c > sc.WAVE for c in counts), start=named,
                wins=[(start[k], wins[k]) for k in sorted(wins)])


def chosen_width(sections, contig_len, n_tasks=None, bs=100, w_max=None, forced=0):
    """The width do_upload takes (None: the front end switches itself off), by its rule with the literals as size_classes reads them:
    from the widest width down, the first whose largest window fits the 256-lead instance; failing that the widest whose largest
    window fits the largest instance."""
    t = sc.window_thresholds()
    w_max = t["w_max_default"] if w_max is None or not t["w_max_lo"] <= w_max <= t["w_max_hi"] else w_max
    if forced and not t["w_min"] <= forced <= w_max:
        forced = 0
    best = None
    for W in ([forced] if forced else range(w_max, t["w_min"] - 1, -1)):
        m = layout(sections, W, contig_len, n_tasks, bs)["largest"]
        if m <= t["win_mid"] or (best is None and m <= t["win_maxcap"]):
            best = W
        if m <= t["win_mid"]:
            break
    return best


def profile_text(info, launches="one launch"):
    """The handle's own report of the layout (the [SNF_PROF] line of do_upload) for a planned layout."""
    return (f"window front end: on (W = {info['W']}: {info['NW']} windows, {info['occupied']} occupied, largest {info['largest']} leads, "
            f"{info['big64']} of more than 64: w4s_segment in {launches})")


# ---------------------------------------------------------------------------------------------- pieces the tables are composed from
def lone(task, svtype, wins, W, per=1, first=0, bin_in=5):
    """`per` leads in a bin of their own window each, for `wins` consecutive windows of width W from window `first`: they fill bucket
    positions in front of what a case is about (one lead: a window that seeds nothing)."""
    return [(task, svtype, ((first + k) << W) + bin_in, per, "plain") for k in range(wins)]


def clusters(task, svtype, first_win, W, sizes, kind="plain"):
    """Ordinary clusters: one bin of sizes[k] leads in window first_win + k."""
    return [(task, svtype, ((first_win + k) << W) + 40 + 3 * k, n, kind) for k, n in enumerate(sizes)]


def bins_in_window(task, svtype, win, W, sizes, kinds=None, gap=30, name=None):
    """Bins of sizes[k] leads, `gap` bins apart, ascending inside window `win`: in the sorted window bin k begins behind the leads of
    the bins in front of it."""
    assert gap * len(sizes) < (1 << W)
    out = [(task, svtype, (win << W) + 7 + gap * k, n, (kinds[k] if kinds else "plain")) for k, n in enumerate(sizes)]
    if name:
        out[0] = out[0] + (name,)
    return out


# ---------------------------------------------------------------------------------------------- the three tables with fixtures
# One task each, default width (every window holds at most 256 leads), registered in tests/cases.py: the unmodified reference's records
# for them are tests/golden/window_edges_*.json.gz, so they also run through test_oracle_golden.py, test_simt_tier.py and
# test_gpu_parity.py.  tests/test_window_edges.py asserts their layouts.
TABLE_W = 10
TABLE_BINS = (64 + 2) << TABLE_W


def bins_sections():
    """The per-bin rules: INS bins of 9 / 10 / 11 / 12 leads (the sequence cap counts every lead), bins in which every fourth lead has
    no length (the seed lead among them), hap counters, bins with dev_min_leads_cluster - 1 / + 0 leads with a length for 2 and 3, bins
    of long leads only."""
    sizes = [9, 10, 11, 12, 9, 10, 11, 12, 12, 13, 4, 5, 6, 3, 7, 11, 12]
    kinds = ["ins20"] * 4 + ["long4"] * 4 + ["hap", "hap", "len:1", "len:2", "len:3", "long", "long", "len:10", "len:11"]
    return [("shuffle", bins_in_window(0, "INS", 0, TABLE_W, sizes, kinds) + bins_in_window(0, "DEL", 1, TABLE_W, [9, 10, 11, 12, 2, 3], ["hap"] * 4 + ["plain"] * 2))]


def borders_sections(W, contig_len, bs=100):
    """Bins 2^W - 1 and 2^W (the last bin of a window and the first of the next) with four leads each, a cluster in the contig's last
    bin, and three leads each at ref_start -1, 0, contig_len - 1 and contig_len."""
    last = (contig_len - 1) // bs
    es = []
    for svtype in ("DEL", "INS"):
        es += [(0, svtype, (1 << W) - 1, 4, "plain"), (0, svtype, 1 << W, 4, "plain")]
    if last > (1 << W) + 1:
        es += [(0, "DEL", last, 5, "plain")]
    es += [(0, "DEL", None, 3, "at:-1"), (0, "DEL", None, 3, "at:0"), (0, "DEL", None, 3, f"at:{contig_len - 1}"), (0, "DEL", None, 3, f"at:{contig_len}")]
    return [("shuffle", es)]


def blocks_rounds_sections():
    """Blocks and rounds in one batch: 62 lone INS windows, an INS pair on positions 62 - 63, 256 INS leads from position 64 whose bins
    straddle positions 128, 192 and 256, a lone lead, then 130 leads from position 321 (first owned position 1 of its block) in which a
    bin of 20 leads covers positions 55 ... 74 of the window; DEL: a window that ends on a block's last position, one of 65 leads on
    position 0 of the next, one that ends the bucket array in a partial block."""
    W = TABLE_W
    ins = lone(0, "INS", 62, W) + [(0, "INS", (62 << W) + 5, 2, "plain", "pair")] + \
        bins_in_window(0, "INS", 63, W, [12, 40, 22, 50, 14, 60, 22, 36], ["long4", "hap", "ins20", "len:30", "long", "long4", "ins20", "len:2"], name="mid") + \
        lone(0, "INS", 1, W, first=64) + bins_in_window(0, "INS", 65, W, [25, 22, 8, 20, 49, 6], ["long4", "hap", "len:2", "ins20", "long4", "len:1"], name="two_rounds")
    n_ins = sum(e[3] for e in ins)
    dels = [(0, "DEL", 5, -n_ins % 64 + 60, "plain", "ends_on_63"), (0, "DEL", (1 << W) + 5, 4, "plain"), (0, "DEL", (2 << W) + 5, 65, "plain", "on_0"),
            (0, "DEL", (3 << W) + 5, 7, "hap"), (0, "DEL", (5 << W) + 5, 3, "plain")]
    return [("shuffle", ins + dels)]


def table_blocks_rounds():
    return build(blocks_rounds_sections(), TABLE_BINS * 100, seed=11)[0]


def table_bins():
    return build(bins_sections(), TABLE_BINS * 100, seed=3)[0]


TABLE_BORDERS_LEN = 100 * (1 << TABLE_W) * 3 + 1


def table_borders():
    return build(borders_sections(TABLE_W, TABLE_BORDERS_LEN), TABLE_BORDERS_LEN, seed=5)[0]
