"""The window index (snf_stage_window.h: w1_hist, w2, w3_scatter -> wbase, wlist, blk_k0, the bucket array) built once, at upload, and
resident for the life of the handle: a pass starts at w4s_segment and writes none of it.

What can go wrong: a later pass finds the index consumed or half reset (the cursors of the scatter, `Counts` zeroed by z0_init, rcflag
left from the pass before); n_valid / n_occ no longer reach the counters; the index is used after the sort path has overwritten the
bucket array (fetch_clusters); a captured pass differs from an eager one; one handle's index shows in another.

One batch of four tasks, built from a tests/window_cases.py plan whose windows are the same for every width 6 .. 12: windows that end
on the last position of a 64-position block and begin on the first of the next, windows that straddle a block edge, one window of
more than 64 leads and one of more than 256 (both large instances of w4s_segment, in rounds; with more than 256 leads in one window
the upload walks every width and lays the first one out again), more than 64 leads outside their contig, a task without a lead,
n_valid = 64 m - 1 / 64 m / 64 m + 1, arrival order shuffled.  Every comparison is bit-exact against the C oracle and from pass to pass;
every case has a host-tier form (tests/emu) and a `-m gpu` form, but the two threads and the captured graph, which the host tier has
not."""
import functools
import re
import threading

import numpy as np
import pytest

import size_classes as sc
import window_cases as wc
from sniffles_amd import abi, lib
from sniffles_amd.config import SnifflesConfig
from test_size_classes import final, prof, same_as_oracle, use_tier

TIERS = [pytest.param("host", id="host"), pytest.param("gpu", id="gpu", marks=pytest.mark.gpu)]
WAVE = sc.WAVE
T = sc.window_thresholds()
W0 = T["w_max_default"]
WW = 12                                     # entries are placed by windows of the widest width any form uses, bins less than 64 apart
L = (6 << WW) * 100                         # six such windows per (task, svtype)
FORMS = [{}, {"SNF_CHAIN": "0", "SNF_GRAPH": "0"}, {"SNF_GRAPH": "1"}, {"SNF_W4_SPLIT": "1"}, {"SNF_WIN_BITS": "6"},
         {"SNF_WIN_BITS_MAX": "12", "SNF_WIN_BITS": "12"}]
ids = lambda env: "-".join(f"{k}={v}" for k, v in env.items()) or "default"
INDEX_KERNELS = ("w1_hist", "w2a_sums", "w2b_offsets", "w3_scatter")
COUNTS = re.compile(r"counts: valid (\d+) windows (\d+) ")


# ---------------------------------------------------------------------------------------------- the batch
def sections(d, pad=False):
    """n_valid = 64 m + d.  Bucket order: task, svtype (soa.SVTYPES), window.  pad: 24 windows of 60 leads more - with SNF_W4_SPLIT the large
    instance only gets a launch of its own where the blocks are more than eight times the windows of more than 64 leads."""
    bins = lambda t, sv, win, sizes, kinds=None, name=None: wc.bins_in_window(t, sv, win, WW, sizes, kinds, gap=5, name=name)
    t0 = [(0, "INS", (0 << WW) + 5, 60, "plain"), (0, "INS", (1 << WW) + 5, 4, "plain", "ends_on_63"), (0, "INS", (2 << WW) + 5, 42, "hap", "on_0")] + \
        bins(0, "INS", 3, [12, 30, 22, 9, 27], ["long4", "hap", "ins20", "len:2", "long4"], name="over_64") + \
        bins(0, "DEL", 0, [44, 120, 11, 95, 30], name="over_256") + [(0, "DEL", (1 << WW) + 9, 9, "hap", "straddles")]
    t1 = wc.clusters(1, "DEL", 0, WW, [5, 3, 8]) + [(1, "DEL", None, 40, "at:-1"), (1, "INS", None, 30, f"at:{L}")]
    t3 = wc.clusters(3, "DUP", 0, WW, [6, 2, 13]) + wc.clusters(3, "INV", 1, WW, [4, 70])
    if pad:
        t1 += [(1, sv, (w << WW) + 11, 60, "plain") for sv in ("INS", "DUP", "INV", "BND") for w in range(6)]
    have = sum(e[3] for e in t0 + t1 + t3 if wc.is_valid(e, 100, L))
    fill = 2 + (d - have - 2) % WAVE                                     # one more DEL bin: 2 .. 65 leads
    return [("shuffle", t0 + t1 + t3 + [(3, "DEL", (2 << WW) + 5, fill, "plain")])]


@functools.lru_cache(maxsize=None)
def batch(d=1, pad=False):
    """Tasks, configuration and the oracle's result, computed once and shared; nothing changes them."""
    import oracle
    tis = wc.build(sections(d, pad), L, n_tasks=4, seed=17 + d)
    cfg = SnifflesConfig()
    return tis, cfg, oracle.run(cfg, list(tis), True)


def planned(d, W=W0, pad=False):
    return wc.layout(sections(d, pad), W, L, n_tasks=4)


@pytest.mark.parametrize("d", [-1, 0, 1])
def test_the_batch_is_what_it_claims(d, oracle_mod):
    infos = [planned(d, W) for W in (6, 8, W0, 12)]
    info = infos[2]
    for other in infos:                                                  # the same windows at every width the forms use
        assert other["wins"] == info["wins"] and other["start"] == info["start"]
    assert info["n_valid"] % WAVE == d % WAVE and info["N"] - info["n_valid"] == 70 > WAVE
    st = info["start"]
    assert st["ends_on_63"] + 4 == WAVE == st["on_0"]                    # a window's last lead on position 63, the next window on position 0
    assert st["straddles"] // WAVE != (st["straddles"] + 8) // WAVE      # nine leads on either side of a block edge
    sizes = dict(info["wins"])
    assert WAVE < sizes[st["over_64"]] == 100 <= T["win_mid"] < sizes[st["over_256"]] == 300 == info["largest"] and info["big64"] >= 2
    assert st["over_64"] % WAVE and st["over_256"] % WAVE                # both begin inside a block
    tis, cfg, exp = batch(d)
    assert [ti.n_leads for ti in tis][2] == 0 and info["N"] == sum(ti.n_leads for ti in tis) < 800
    assert wc.chosen_width(sections(d), L, n_tasks=4) == W0              # no width gives 256: the widest, laid out again behind the loop
    recs = final(exp, list(tis))
    assert sum(len(r) for r in recs) >= 20 and any(not r["qc"] for t in recs for r in t) and any(r["qc"] for t in recs for r in t)


# ---------------------------------------------------------------------------------------------- pass after pass
def as_execute(recs, cfg):
    """CallTask.execute's two statements (parallel.py:265-271) over the candidates' records."""
    out = []
    for t in recs:
        if isinstance(t, dict):
            out.append(t)
            continue
        keep = [r for r in t if cfg.no_qc or r["qc"]]
        out.append(sorted(keep, key=lambda r: r["pos"]) if cfg.sort else keep)
    return out


def counters(capfd):
    m = COUNTS.search(prof(capfd)["counts"][-1])
    return int(m.group(1)), int(m.group(2))


def passes_on(b, tis, cfg, exp, capfd, info, n):
    """n passes with the output mode alternating candidates / execute: every pass gives the oracle's records, the same block as the pass
    of its mode before it, and the counters the plan gives."""
    want = {abi.OUT_CANDIDATES: final(exp, tis)}
    want[abi.OUT_EXECUTE] = as_execute(want[abi.OUT_CANDIDATES], cfg)
    last = {}
    for k in range(n):
        mode = (abi.OUT_CANDIDATES, abi.OUT_EXECUTE)[k % 2]
        b.set_output(mode)
        b.run_pass()
        capfd.readouterr()
        got = b.fetch(1)
        assert counters(capfd) == (info["n_valid"], info["occupied"]), k
        assert final(got, tis) == want[mode], k
        if mode == abi.OUT_CANDIDATES:
            same_as_oracle(got, exp, tis)
        block = (got.calls.tobytes(), got.alt_pool.tobytes(), got.task_call_off.tobytes(), got.coverage_average_total.tobytes())
        assert last.setdefault(mode, block) == block, k
    return last


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("d", [-1, 0, 1])
@pytest.mark.parametrize("form", FORMS, ids=ids)
def test_passes_on_one_handle(form, d, tier, oracle_mod, monkeypatch, capfd):
    """Four passes (six where passes are replayed from a graph - the default of a batch this small, and SNF_GRAPH=1: a mode's first pass
    is eager, its second captured, its third a replay)."""
    use_tier(tier, monkeypatch)
    monkeypatch.setenv("SNF_PROF", "1")
    for k, v in form.items():
        monkeypatch.setenv(k, v)
    pad = "SNF_W4_SPLIT" in form
    tis, cfg, exp = batch(d, pad)
    tis = list(tis)
    graphs = form.get("SNF_GRAPH", "1") == "1"
    info = planned(d, int(form.get("SNF_WIN_BITS", W0)), pad)
    if pad:
        assert 0 < 8 * info["big64"] < (info["N"] + WAVE - 1) // WAVE and info["n_valid"] % WAVE == d % WAVE
    capfd.readouterr()
    with lib.Batch(cfg, tis) as b:
        lines = prof(capfd)["window front end"]
        assert len(lines) == 1 and wc.profile_text(info, "two launches" if pad else "one launch") in lines[0], lines
        passes_on(b, tis, cfg, exp, capfd, info, 6 if graphs else 4)
        b.call_candidates(); b.finalize()                               # ... and the two calls on their own behind them
        assert final(b.fetch(1), tis) == as_execute(final(exp, tis), cfg)


@pytest.mark.gpu
def test_a_replayed_pass_is_an_eager_pass(oracle_mod, monkeypatch, capfd):
    """The same six passes replayed from graphs (the default of a batch this small) and eagerly (SNF_GRAPH=0): identical blocks."""
    use_tier("gpu", monkeypatch)
    monkeypatch.setenv("SNF_PROF", "1")
    tis, cfg, exp = batch(1)
    tis = list(tis)
    blocks = []
    for graph in (None, "0"):
        if graph:
            monkeypatch.setenv("SNF_GRAPH", graph)
        with lib.Batch(cfg, tis) as b:
            blocks.append(passes_on(b, tis, cfg, exp, capfd, planned(1), 6))
    assert blocks[0] == blocks[1]


@pytest.mark.gpu
def test_passes_are_captured_on_the_device(oracle_mod, monkeypatch, capfd):
    use_tier("gpu", monkeypatch)
    monkeypatch.setenv("SNF_PROF", "1")
    tis, cfg, exp = batch(1)
    tis = list(tis)
    with lib.Batch(cfg, tis) as b:
        capfd.readouterr()
        for _ in range(3):
            b.run_pass()
            same_as_oracle(b.fetch(1), exp, tis)
        lines = capfd.readouterr().err
    assert "pass graph: captured" in lines and "capture failed" not in lines and "gave up" not in lines, lines[-800:]


# ---------------------------------------------------------------------------------------------- the switch
@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("d", [-1, 0, 1])
def test_index_rebuilt_in_every_pass_gives_the_same_records(d, tier, oracle_mod, monkeypatch, capfd):
    """SNF_READPREP_EACH_PASS: both indexes are built again in every call_candidates - identical blocks, pass after pass."""
    use_tier(tier, monkeypatch)
    monkeypatch.setenv("SNF_PROF", "1")
    tis, cfg, exp = batch(d)
    tis = list(tis)
    blocks = []
    for each in (False, True):
        if each:
            monkeypatch.setenv("SNF_READPREP_EACH_PASS", "1")
        with lib.Batch(cfg, tis) as b:
            blocks.append(passes_on(b, tis, cfg, exp, capfd, planned(d), 4))
    assert blocks[0] == blocks[1]


def timing_names(tier, env, monkeypatch):
    use_tier(tier, monkeypatch)
    monkeypatch.setenv("SNF_TIME_ALL", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    tis, cfg, exp = batch(1)
    tis = list(tis)
    with lib.Batch(cfg, tis) as b:
        b.timing_every(1)
        names = []
        for _ in range(2):
            b.run_pass()
            same_as_oracle(b.fetch(1), exp, tis)
            names.append([n for n, _, _ in b.timings()])
    return names


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("form", [{}, {"SNF_CHAIN": "0"}], ids=ids)
def test_a_default_pass_begins_at_w4s_segment(form, tier, oracle_mod, monkeypatch):
    for names in timing_names(tier, form, monkeypatch):
        assert {"w4s_segment", "front_window", "w6t_emit"} <= set(names), names
        assert not set(INDEX_KERNELS + ("w2c_offsets",)) & set(names), names


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("form", [{}, {"SNF_CHAIN": "0"}], ids=ids)
def test_with_the_switch_the_index_kernels_are_in_the_pass(form, tier, oracle_mod, monkeypatch):
    """(a batch this small scans in one launch unless SNF_CHAIN=0: w2c_offsets in the place of the w2a / w2b pair)"""
    for names in timing_names(tier, dict(form, SNF_READPREP_EACH_PASS="1"), monkeypatch):
        assert {"w4s_segment", "front_window", "w6t_emit"} <= set(names), names
        assert set(INDEX_KERNELS if form else ("w1_hist", "w2c_offsets", "w3_scatter")) <= set(names), names
        assert names.index("w1_hist") < names.index("w3_scatter") < names.index("w4s_segment")


# ---------------------------------------------------------------------------------------------- the sort path takes the arrays
@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("form", [{}, {"SNF_CHAIN": "0", "SNF_GRAPH": "0"}], ids=ids)
def test_pass_fetch_clusters_pass(form, tier, oracle_mod, monkeypatch):
    """fetch_clusters redoes the candidate stage on the sort path, which writes its keys where the bucket array was: the passes behind
    it must not take the short front end again.  The calls are the ones from before (cluster_seed_index apart, which that path
    counts over every occupied bin)."""
    use_tier(tier, monkeypatch)
    for k, v in form.items():
        monkeypatch.setenv(k, v)
    tis, cfg, exp = batch(1)
    tis = list(tis)
    with lib.Batch(cfg, tis) as b:
        for _ in range(2):
            b.run_pass()
            before = b.fetch(1)
            same_as_oracle(before, exp, tis)
        cl = b.fetch_clusters(2)
        assert len(cl["task_index"]) > 0
        for _ in range(3):
            b.run_pass()
            got = b.fetch(1)
            assert final(got, tis) == final(exp, tis)
            assert len(got.calls) == len(before.calls) and np.array_equal(got.task_call_off, before.task_call_off)
            for f in got.calls.dtype.names:
                if f != "cluster_seed_index":
                    assert np.array_equal(got.calls[f], before.calls[f], equal_nan=got.calls[f].dtype.kind == "f"), f


# ---------------------------------------------------------------------------------------------- edge sizes
def edge_sections(name):
    if name == "no_lead":
        return None
    if name == "every_lead_dropped":
        return [("shuffle", [(0, "DEL", None, 40, "at:-1"), (1, "INS", None, 30, f"at:{L}"), (1, "DEL", None, 5, f"at:{L + 7}")])]
    if name == "single_lead":
        return [("plan", [(1, "DEL", (1 << WW) + 5, 1, "plain")])]
    if name == "n_128":
        return [("shuffle", wc.clusters(0, "DEL", 0, WW, [20, 44, 30]) + wc.clusters(1, "INS", 1, WW, [9, 25], "long4"))]
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def edge_batch(name):
    import cases
    import oracle
    secs = edge_sections(name)
    if secs is None:
        tis = [cases.mk_task([], cases._reads(12, 0, 50_000), 50_000, task_id=t, contig=f"chrE{t}") for t in range(2)]
    else:
        tis = wc.build(secs, L, n_tasks=2, seed=29)
    cfg = SnifflesConfig()
    return tis, cfg, oracle.run(cfg, list(tis), True)


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("name", ["no_lead", "every_lead_dropped", "single_lead", "n_128"])
def test_edge_sizes(name, tier, oracle_mod, monkeypatch):
    use_tier(tier, monkeypatch)
    tis, cfg, exp = edge_batch(name)
    tis = list(tis)
    n = sum(ti.n_leads for ti in tis)
    assert n == dict(no_lead=0, every_lead_dropped=75, single_lead=1, n_128=128)[name]
    if name == "n_128":
        assert wc.layout(edge_sections(name), W0, L, n_tasks=2)["n_valid"] == 128 and len(exp.calls) >= 5
    else:
        assert len(exp.calls) == 0
    want = final(exp, tis)
    with lib.Batch(cfg, tis) as b:
        for k in range(4):
            b.set_output((abi.OUT_CANDIDATES, abi.OUT_EXECUTE)[k % 2])
            b.run_pass()
            assert final(b.fetch(1), tis) == (as_execute(want, cfg) if k % 2 else want), k
        b.set_output(abi.OUT_CANDIDATES)
        b.call_candidates(); b.finalize()
        same_as_oracle(b.fetch(1), exp, tis)


# ---------------------------------------------------------------------------------------------- handle beside handle
@pytest.mark.parametrize("tier", TIERS)
def test_two_handles_keep_their_own_index(tier, oracle_mod, monkeypatch, capfd):
    """Two batches of nearly the same size open at once (n_valid 64 m and 64 m + 1: another block layout from the last DEL window on),
    their passes in turn; then a third in the memory the first gave back."""
    use_tier(tier, monkeypatch)
    monkeypatch.setenv("SNF_PROF", "1")
    monkeypatch.delenv("SNF_NO_SLAB_CACHE", raising=False)
    (ta, cfg, ea), (tb, _, eb), (tc, _, ec) = batch(0), batch(1), batch(-1)
    ta, tb, tc = list(ta), list(tb), list(tc)
    with lib.Batch(cfg, ta) as a:
        with lib.Batch(cfg, tb) as b:
            for _ in range(3):
                a.run_pass(); b.run_pass()
                same_as_oracle(a.fetch(1), ea, ta)
                same_as_oracle(b.fetch(1), eb, tb)
        with lib.Batch(cfg, tc) as c:
            for _ in range(2):
                c.run_pass(); a.run_pass()
                same_as_oracle(c.fetch(1), ec, tc)
                same_as_oracle(a.fetch(1), ea, ta)


@pytest.mark.gpu
def test_two_handles_from_two_threads(oracle_mod, monkeypatch):
    """Two handles over the same tasks, each driven by a thread of its own, four passes each: identical blocks, the oracle's."""
    use_tier("gpu", monkeypatch)
    tis, cfg, exp = batch(1)
    tis = list(tis)
    out, errs = [[], []], []

    def drive(k):
        try:
            with lib.Batch(cfg, tis) as b:
                for _ in range(4):
                    b.run_pass()
                    out[k].append(b.fetch(1))
        except BaseException as e:  # noqa: BLE001 - reported by the test's thread
            errs.append(e)
    threads = [threading.Thread(target=drive, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    assert len(out[0]) == len(out[1]) == 4
    for got in out[0] + out[1]:
        same_as_oracle(got, exp, tis)
        for f in ("calls", "alt_pool", "task_call_off"):
            assert getattr(got, f).tobytes() == getattr(out[0][0], f).tobytes(), f
