"""View::skip_single (snf_lib.hip run_pass, snf_stage_window.h w4s_segment, snf_stage_cluster.h a4_binstats_body): a whole pass
(`snf_batch_pass`) that returns the execute block with QC on forms no cluster of the single-breakend types - `qc_sv` fails every
SINGLE_LEFT / SINGLE_RIGHT candidate (reference `postprocessing.py:244-246`), so the block can never hold one.

What can go wrong: a wave that leaves early leaves stale words behind for w6t_emit (another pass of the handle has written flags
there), or words of a window that reaches into its block unwritten; a wave with windows of both kinds drops or keeps the wrong
ones; `sv_id`s, `task_status`, `coverage.mean()` or a BND's carried `end` move; the switch leaks into a pass that is asked for the
candidates (candidates mode, `no_qc`, `dev_output_candidates`, `SNF_OUT_ALL_CANDIDATES`, the two calls, a stage-0 fetch); the launch-size hints one state
learned (no cluster of more than 64 leads) are used by the other; a replayed graph carries the wrong state.

Every case compares the execute block - records with their `sv_id`s, read names, ALT pool, `task_status`, `task_call_off`,
`coverage_average_total` - byte for byte with the block under `SNF_OUT_ALL_CANDIDATES` (every candidate formed), and with the oracle's candidates filtered by `qc`
and sorted by position; the number of waves that left early with the number the plan gives (bucket order: task, svtype, window).
Contigs of 200 kb, a few hundred leads; a host-tier form (tests/emu) and a `-m gpu` form of every case."""
import functools
import re

import numpy as np
import pytest

import cases
import size_classes as sc
import window_cases as wc
from sniffles_amd import abi, lib, records
from sniffles_amd.config import SnifflesConfig
from sniffles_amd.soa import SVT
from test_size_classes import final, prof, same_as_oracle, use_tier
from test_window_index import as_execute

TIERS = [pytest.param("host", id="host"), pytest.param("gpu", id="gpu", marks=pytest.mark.gpu)]
WAVE = sc.WAVE
L = 200_000
SINGLES = ("SINGLE_LEFT", "SINGLE_RIGHT")
LEFT = re.compile(r"skip single: (\d+) of (\d+) waves")


# ---------------------------------------------------------------------------------------------- batches from a plan
def build(entries, n_tasks, seed, shuffle=True):
    """Tasks from window_cases entries (task, svtype, bin, n leads, kind): the five reference types by window_cases._lead, the two
    single-breakend types as the leads the extraction gives them (svlen 0, no sequence).  Arrival order shuffled."""
    rng = np.random.default_rng([seed, 977])
    allele = cases._rng_seq(rng, 90)
    tis = []
    for t in range(n_tasks):
        leads = []
        for num, e in enumerate(entries):
            if e[0] != t:
                continue
            for i in range(e[3]):
                if e[1] in SINGLES:
                    leads.append(dict(svtype=e[1], ref_start=e[2] * 100 + (7 * i + 3) % 30, svlen=0, read=f"t{t}e{num}_{i}", strand="+-"[i % 2]))
                else:
                    leads.append(wc._lead(e, i, rng, 100, L, allele, f"t{t}e{num}"))
        if shuffle:
            leads = [leads[i] for i in rng.permutation(len(leads))]
        reads = cases._reads(24, 0, L) + cases._reads(7, 0, L // 2, 1) + cases._reads(5, L // 3, L, 2)
        tis.append(cases.mk_task(leads, reads, L, task_id=t, contig=f"chrK{t}"))
    return tis


def plan_of(entries, W):
    """From the plan alone: dict(n_valid, blocks, left = the blocks all of whose windows are single-breakend ones, mixed = those with
    windows of both kinds, start {(task, svtype, window): first bucket position}, size {...: leads})."""
    size = {}
    for e in entries:
        key = (e[0], SVT[e[1]], e[2] >> W)
        size[key] = size.get(key, 0) + e[3]
    start, pos = {}, 0
    for key in sorted(size):
        start[key] = pos
        pos += size[key]
    left, mixed = [], []
    for blk in range((pos + WAVE - 1) // WAVE):
        kinds = {k[1] >= SVT["SINGLE_LEFT"] for k, s in start.items() if WAVE * blk <= s < WAVE * blk + WAVE}
        if kinds == {True}:
            left.append(blk)
        if kinds == {True, False}:
            mixed.append(blk)
    return dict(n_valid=pos, blocks=(pos + WAVE - 1) // WAVE, left=left, mixed=mixed, start=start, size=size)


def win(W, k, bin_in=9):
    return (k << W) + bin_in


def entries_of(name, W):
    E = lambda t, sv, k, n, kind="plain": (t, sv, win(W, k), n, kind)
    if name == "singles_only":
        return [E(0, "SINGLE_LEFT", 0, 9), E(0, "SINGLE_LEFT", 1, 70), E(0, "SINGLE_RIGHT", 0, 5), E(0, "SINGLE_RIGHT", 1, 12)]
    if name == "mixed_waves":
        # block 0: DEL, BND, SINGLE_LEFT windows of task 0 (the last BND window and the first SINGLE_LEFT one in one block); block 1: a
        # SINGLE_RIGHT window alone, which covers block 2; block 3: the last SINGLE_RIGHT window of task 0 and the first INS window of
        # task 1; block 4: the single windows of task 1
        return [E(0, "DEL", 0, 10), E(0, "DEL", 1, 12, "hap"), E(0, "BND", 1, 14), E(0, "SINGLE_LEFT", 0, 10), E(0, "SINGLE_LEFT", 1, 60),
                E(0, "SINGLE_RIGHT", 0, 90), E(0, "SINGLE_RIGHT", 1, 30),
                E(1, "INS", 0, 20, "long4"), E(1, "INV", 1, 9), E(1, "BND", 0, 11), E(1, "SINGLE_LEFT", 1, 6), E(1, "SINGLE_RIGHT", 0, 3),
                E(1, "SINGLE_RIGHT", 1, 40)]
    if name.startswith("big_single_"):
        # a single window of n leads behind a BND window in the same block: it reaches into the blocks behind, which the earlier wave
        # owns; a SINGLE_RIGHT block that owns windows of its own only; task 1 behind it
        n = int(name.split("_")[2])
        return [E(0, "DEL", 0, 8), E(0, "INS", 1, 12, "ins20"), E(0, "BND", 0, 10), E(0, "SINGLE_LEFT", 1, n), E(0, "SINGLE_RIGHT", 0, 7),
                E(0, "SINGLE_RIGHT", 1, 66), E(1, "INS", 0, 15), E(1, "DEL", 1, 30, "hap"), E(1, "SINGLE_LEFT", 0, 4)]
    if name.startswith("split_"):
        # SNF_W4_SPLIT (width 6: 32 windows per type): the large instance gets a launch of its own where the blocks are more than eight times
        # the windows of more than 64 leads - sixteen windows of 60 leads more.  The window of n single leads starts in a block of its own
        # kind (left early by the small instance, whatever its size) ...
        n = int(name.split("_")[1])
        pad = [E(0, "DUP", k, 60) for k in range(16)]
        return pad + [E(0, "DEL", 0, 8), E(0, "BND", 3, 18), E(0, "SINGLE_LEFT", 2, 50), E(0, "SINGLE_LEFT", 5, n), E(0, "SINGLE_RIGHT", 7, 60),
                      E(1, "INS", 4, 15), E(1, "DEL", 9, 30, "hap"), E(1, "BND", 2, 90), E(1, "SINGLE_LEFT", 0, 4), E(1, "SINGLE_LEFT", 3, 60)]
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def batch(name, W=10, **cfg_kw):
    """Tasks, configuration and the oracle's result, computed once and shared; nothing changes them."""
    import oracle
    entries = entries_of(name, W)
    tis = build(entries, 1 + max(e[0] for e in entries), seed=len(name))
    cfg = SnifflesConfig(**cfg_kw)
    return tuple(tis), cfg, oracle.run(cfg, tis, True)


def block(res):
    return (res.calls.tobytes(), res.rnames.tobytes(), res.alt_pool.tobytes(), res.task_status.tobytes(), res.task_call_off.tobytes(),
            res.coverage_average_total.tobytes())


def n_single(res):
    return int(np.isin(res.calls["svtype"], [SVT[s] for s in SINGLES]).sum())


def execute_passes(tis, cfg, exp, capfd, skip, n=3, left=None):
    """n whole passes in execute mode on one handle (eager, captured, replayed where passes are replayed): the oracle's kept calls every
    time, one block throughout - which is returned."""
    want = as_execute(final(exp, tis), cfg)
    with lib.Batch(cfg, tis) as b:
        b.set_output(abi.OUT_EXECUTE if skip else abi.OUT_EXECUTE | abi.OUT_ALL_CANDIDATES)
        blocks = []
        for k in range(n):
            b.run_pass()
            capfd.readouterr()
            got = b.fetch(1)
            lines = prof(capfd)["skip single"]
            assert len(lines) == (1 if skip else 0), (k, lines)
            if skip and left is not None:
                m = LEFT.search(lines[0])
                assert (int(m.group(1)), int(m.group(2))) == left, (k, lines[0])
            assert final(got, tis) == want, k
            assert np.array_equal(got.task_status, exp.task_status) and np.array_equal(got.coverage_average_total, exp.coverage_average_total, equal_nan=True)
            blocks.append(block(got))
    assert all(x == blocks[0] for x in blocks)
    return blocks[0]


def both_values(name, tier, monkeypatch, capfd, env=None, W=10, front=True):
    """The execute block with the switch on (the default) and off: equal, the oracle's, and as many waves left early as the plan says."""
    use_tier(tier, monkeypatch)
    monkeypatch.setenv("SNF_PROF", "1")
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    tis, cfg, exp = batch(name, W)
    tis = list(tis)
    info = plan_of(entries_of(name, W), W)
    assert n_single(exp) > 0 and not exp.calls["qc"][np.isin(exp.calls["svtype"], [SVT[s] for s in SINGLES])].any()
    on = execute_passes(tis, cfg, exp, capfd, True, left=(len(info["left"]) if front else 0, (sum(ti.n_leads for ti in tis) + WAVE - 1) // WAVE))
    assert execute_passes(tis, cfg, exp, capfd, False) == on
    return info


# ---------------------------------------------------------------------------------------------- 1. nothing but single leads
@pytest.mark.parametrize("tier", TIERS)
def test_a_task_of_single_leads_only(tier, oracle_mod, monkeypatch, capfd):
    info = both_values("singles_only", tier, monkeypatch, capfd)
    tis, cfg, exp = batch("singles_only")
    assert info["left"] == list(range(info["blocks"])) and info["blocks"] == 2
    assert as_execute(final(exp, list(tis)), cfg) == [[]] and int(exp.task_status[0]) == 0 and exp.coverage_average_total[0] > 0


# ---------------------------------------------------------------------------------------------- 2. waves with windows of both kinds
@pytest.mark.parametrize("tier", TIERS)
def test_waves_that_own_windows_of_both_kinds(tier, oracle_mod, monkeypatch, capfd):
    info = both_values("mixed_waves", tier, monkeypatch, capfd)
    st = info["start"]
    B, SL, SR, INS = SVT["BND"], SVT["SINGLE_LEFT"], SVT["SINGLE_RIGHT"], SVT["INS"]
    assert st[(0, B, 1)] // WAVE == st[(0, SL, 0)] // WAVE == 0                       # the last BND window and the first SINGLE_LEFT one of task 0
    assert st[(0, SR, 1)] // WAVE == st[(1, INS, 0)] // WAVE == 3                     # the last SINGLE_RIGHT window of task 0, the first INS one of task 1
    assert info["mixed"] == [0, 3] and info["left"] == [1, 4] and info["blocks"] == 5          # (block 2 owns nothing)
    tis, cfg, exp = batch("mixed_waves")
    assert sum(len(t) for t in as_execute(final(exp, list(tis)), cfg)) >= 5


# ---------------------------------------------------------------------------------------------- 3. large single windows
@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("n", [65, 257, 1100])
def test_a_large_single_window(n, tier, oracle_mod, monkeypatch, capfd):
    """65 leads: rounds of the 256-lead instance; 257: the 1024-lead instance; 1100: more than the largest instance holds at the narrowest
    width - the sort path (a4_binstats_body), where no wave leaves early."""
    T = sc.window_thresholds()
    name = f"big_single_{n}"
    assert (n > T["win_maxcap"]) == (n == 1100) and (n > T["win_mid"]) == (n >= 257) and n > WAVE
    assert wc.chosen_width([("shuffle", entries_of(name, 10))], L, n_tasks=2) == (None if n == 1100 else 10)
    info = both_values(name, tier, monkeypatch, capfd, front=n != 1100)
    st, size = info["start"], info["size"]
    big = (0, SVT["SINGLE_LEFT"], 1)
    assert size[big] == n and st[big] // WAVE == st[(0, SVT["BND"], 0)] // WAVE == 0      # begins in a block with a BND window ...
    reached = range(1, (st[big] + n - 1) // WAVE + 1)
    assert len(reached) >= 1 and not set(reached[:-1]) & set(info["left"] + info["mixed"])   # ... and the blocks it covers own nothing
    assert len(info["left"]) >= 1


# ---------------------------------------------------------------------------------------------- 4. the launch-size hints
@pytest.mark.parametrize("tier", TIERS)
def test_hints_are_kept_per_state(tier, oracle_mod, monkeypatch, capfd):
    """A single cluster of more than 64 leads and no other: the execute passes hand nothing to x_big and learn that they may skip it, the
    candidates passes of the same handle need it (a skipped launch with work fails the fetch)."""
    use_tier(tier, monkeypatch)
    tis, cfg, exp = batch("big_single_65")
    tis = list(tis)
    sizes = exp.calls["support"][np.isin(exp.calls["svtype"], [SVT[s] for s in SINGLES])]
    assert sizes.max() > WAVE and exp.calls["support"][~np.isin(exp.calls["svtype"], [SVT[s] for s in SINGLES])].max() < WAVE
    with lib.Batch(cfg, tis) as b:
        b.run_pass()
        fresh = b.fetch(1)
    same_as_oracle(fresh, exp, tis)
    want = {abi.OUT_CANDIDATES: block(fresh)}
    with lib.Batch(cfg, tis) as b:
        for k, mode in enumerate([abi.OUT_EXECUTE, abi.OUT_EXECUTE, abi.OUT_CANDIDATES, abi.OUT_EXECUTE, abi.OUT_CANDIDATES, abi.OUT_CANDIDATES,
                                  abi.OUT_EXECUTE, abi.OUT_CANDIDATES]):
            b.set_output(mode)
            b.run_pass()
            got = b.fetch(1)
            assert want.setdefault(mode, block(got)) == block(got), k
            if mode == abi.OUT_EXECUTE:
                assert final(got, tis) == as_execute(final(exp, tis), cfg), k
    with lib.Batch(cfg, tis) as b:
        b.set_output(abi.OUT_EXECUTE | abi.OUT_ALL_CANDIDATES)
        b.run_pass()
        assert block(b.fetch(1)) == want[abi.OUT_EXECUTE]


# ---------------------------------------------------------------------------------------------- 5. where the candidates are asked for
@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("where", ["candidates", "no_qc", "dev_output_candidates", "two_calls", "all_candidates"])
def test_singles_stay_where_the_candidates_are_asked_for(where, tier, oracle_mod, monkeypatch, capfd):
    use_tier(tier, monkeypatch)
    monkeypatch.setenv("SNF_PROF", "1")
    kw = dict(no_qc=dict(no_qc=True), dev_output_candidates=dict(dev_output_candidates="x.tsv")).get(where, {})
    tis, cfg, exp = batch("mixed_waves", 10, **kw)
    tis = list(tis)
    assert n_single(exp) >= 4
    with lib.Batch(cfg, tis) as b:
        b.set_output(dict(candidates=abi.OUT_CANDIDATES, all_candidates=abi.OUT_EXECUTE | abi.OUT_ALL_CANDIDATES).get(where, abi.OUT_EXECUTE))
        capfd.readouterr()
        for k in range(3):
            if where == "two_calls":
                b.call_candidates()
                got0 = b.fetch(0)
                assert records.records(got0, tis, "cand") == records.records(oracle_mod.run(cfg, tis, False), tis, "cand") and n_single(got0) == n_single(exp), k
                b.finalize()
            else:
                b.run_pass()
            got = b.fetch(1)
            assert b.n_candidates() == len(exp.calls), k          # (what Task.sv_id of the drop-in task advances by)
            if where == "candidates":
                same_as_oracle(got, exp, tis)
            assert final(got, tis) == (final(exp, tis) if where == "candidates" else as_execute(final(exp, tis), cfg)), k
            assert (n_single(got) == n_single(exp)) == (where in ("candidates", "no_qc")), k
            if where == "dev_output_candidates":       # (qc_sv lets them through to the other filters)
                kept = np.isin(exp.calls["svtype"], [SVT[s] for s in SINGLES]) & (exp.calls["qc"] != 0)
                assert n_single(got) == int(kept.sum()) > 0, k
        assert not prof(capfd)["skip single"]


# ---------------------------------------------------------------------------------------------- 6. modes switched between replays
@pytest.mark.parametrize("tier", TIERS)
def test_the_mode_switched_between_passes_of_one_handle(tier, oracle_mod, monkeypatch, capfd):
    """A batch this small replays its passes from a graph per output mode (eager, captured, replayed): the stale words of the other
    mode's pass lie in key_out every time the mode changes."""
    use_tier(tier, monkeypatch)
    monkeypatch.setenv("SNF_PROF", "1")
    tis, cfg, exp = batch("mixed_waves")
    tis = list(tis)
    want = {abi.OUT_CANDIDATES: final(exp, tis), abi.OUT_EXECUTE: as_execute(final(exp, tis), cfg)}
    seen = {}
    E, C = abi.OUT_EXECUTE, abi.OUT_CANDIDATES
    with lib.Batch(cfg, tis) as b:
        capfd.readouterr()
        for k, mode in enumerate([E, E, E, C, C, C, E, C, E, E, C]):
            b.set_output(mode)
            b.run_pass()
            got = b.fetch(1)
            assert final(got, tis) == want[mode], k
            assert seen.setdefault(mode, block(got)) == block(got), k
            assert len(prof(capfd)["skip single"]) == (mode == E), k
        err = capfd.readouterr().err
    assert "capture failed" not in err and "gave up" not in err
    with lib.Batch(cfg, tis) as b:
        b.set_output(E | abi.OUT_ALL_CANDIDATES)
        b.run_pass()
        assert block(b.fetch(1)) == seen[E]


# ---------------------------------------------------------------------------------------------- 7. a task that raises
@pytest.mark.parametrize("tier", TIERS)
def test_a_bnd_first_task_keeps_its_status(tier, oracle_mod, monkeypatch, capfd):
    """The first candidate of the task is a BND (postprocessing.coverage raises, SNF_TASK_ERR_UNBOUND_END); single leads behind it."""
    use_tier(tier, monkeypatch)
    monkeypatch.setenv("SNF_PROF", "1")
    import oracle
    leads = [dict(svtype="BND", ref_start=5000 + i % 2, read=f"b{i}", strand="+-"[i % 2], mate=("chr2", 70000 + i, True, False)) for i in range(6)]
    leads += [dict(svtype=sv, ref_start=p + i % 3, svlen=0, read=f"{sv}{i}") for sv, p in (("SINGLE_LEFT", 9000), ("SINGLE_RIGHT", 15000)) for i in range(5)]
    tis = [cases.mk_task(leads, cases._reads(20, 0, 20000), 20000), batch("mixed_waves")[0][1]]
    cfg = SnifflesConfig()
    exp = oracle.run(cfg, tis, True)
    assert int(exp.task_status[0]) == abi.TASK_ERR_UNBOUND_END and int(exp.task_status[1]) == 0
    blocks = []
    for skip in (True, False):
        blocks.append(execute_passes(tis, cfg, exp, capfd, skip))
    assert blocks[0] == blocks[1]


# ---------------------------------------------------------------------------------------------- 8. w4s_segment in two launches
@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("n", [65, 300])
def test_the_split_form(n, tier, oracle_mod, monkeypatch, capfd):
    name = f"split_{n}"
    info = plan_of(entries_of(name, 6), 6)
    big64 = sum(c > WAVE for c in info["size"].values())
    assert 0 < 8 * big64 < info["blocks"]
    big = (0, SVT["SINGLE_LEFT"], 5)
    assert info["start"][big] // WAVE in info["left"] and info["mixed"]
    use_tier(tier, monkeypatch)
    monkeypatch.setenv("SNF_PROF", "1")
    monkeypatch.setenv("SNF_W4_SPLIT", "1")
    monkeypatch.setenv("SNF_WIN_BITS", "6")
    tis, cfg, exp = batch(name, 6)
    capfd.readouterr()
    with lib.Batch(cfg, list(tis)):
        assert "w4s_segment in two launches" in capfd.readouterr().err
    both_values(name, tier, monkeypatch, capfd, env=dict(SNF_W4_SPLIT="1", SNF_WIN_BITS="6"), W=6)
