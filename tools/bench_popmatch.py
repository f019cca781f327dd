#!/usr/bin/env python3
"""Population annotation of a merge (`--combine-population`): what `snf_population_match_batch` costs, and what the same answer costs
with the entry points the library had before it.

Workload: the synthetic population of `bench.py --config 4` (tools/bench_population.py: S HG002-shaped samples, shared SV sites, own
reads) is merged once; its merged calls are written as a population SNF with `snfp.PopulationWriter`; then the same population is
merged again with `config.combine_population` = that file - every merged call is one query against the variant list of its (contig,
block, SV type).

  new       `lib.population_match_batch`: ONE launch, a wave per query; the survivors of the positional gate are aligned in ascending
            (dist, index) order and the search ends at the first accepted one
  baseline  the positional gate on the host (numpy, per list) and EVERY gate-passing insertion pair through
            `snf_edit_distance_batch_k` with the cut-off the acceptance test implies - what the parent commit offers; the best variant
            is picked on the host

Both produce the same (best, dist) per query (checked).  They run alternately, `--rounds` times (at least three), in one process on one
device.  Reported: per round the wall time of each (C-ABI call + host work around it), the new kernel's time (HIP events), alignments and
DP cells of both, and the share of the annotation in the merge step (`candstore.last_timing`).  One JSON line at the end.

    python tools/bench_popmatch.py --samples 10 --scale 0.05 --rounds 5
"""
from __future__ import annotations

import argparse
import io
import json
import math
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def cutoff(svlen: int, pctseq: float, dcap: int) -> int:
    """snf_combine.hip::align_cutoff: the largest d with (svlen - d) / svlen > pctseq, at most dcap; -1: none."""
    d0 = min(max(int(math.floor(svlen * (1.0 - pctseq))), 0), dcap)
    while d0 < dcap and (svlen - (d0 + 1)) / svlen > pctseq:
        d0 += 1
    while d0 >= 0 and not (svlen - d0) / svlen > pctseq:
        d0 -= 1
    return d0


def baseline(lib, cfg, table, q, device):
    """(best, dist, stats): the gate on the host, every gate-passing insertion pair through snf_edit_distance_batch_k."""
    n = len(q["alt_off"]) - 1
    best, dist = np.full(n, -1, np.int32), np.zeros(n, np.int32)
    loff, vpos, vlen = table["list_off"], table["v_pos"].astype(np.int64), np.abs(table["v_svlen"].astype(np.int64))
    vpool, voff = table["v_alt_pool"].tobytes(), table["v_alt_off"]
    qpool, qoff = np.asarray(q["alt_pool"], np.uint8).tobytes(), q["alt_off"]
    pct = float(cfg.combine_pctseq)
    survivors, pairs, bounds, owner = [], [], [], []
    t0 = time.perf_counter()
    for k in range(n):
        li = int(q["list"][k])
        if li < 0:
            survivors.append(None)
            continue
        a, b = int(loff[li]), int(loff[li + 1])
        clen = abs(int(q["svlen"][k]))
        d = np.abs(vpos[a:b] - int(q["pos"][k])) + np.abs(vlen[a:b] - clen)
        ok = (d <= cfg.combine_match * np.sqrt(np.minimum(vlen[a:b], clen).astype(np.float64))) & (d <= cfg.combine_match_max)
        idx = np.flatnonzero(ok)
        survivors.append((a + idx, d[idx]))
        if table["list_is_ins"][li] and pct:
            qa = qpool[int(qoff[k]):int(qoff[k + 1])]
            for gi in (a + idx).tolist():
                va = vpool[int(voff[gi]):int(voff[gi + 1])]
                pairs.append((va, qa))
                bounds.append(cutoff(int(table["v_svlen"][gi]), pct, max(len(va), len(qa))))
                owner.append((k, gi))
    t_gate = time.perf_counter() - t0
    t0 = time.perf_counter()
    todo = [i for i, kmax in enumerate(bounds) if kmax >= 0]
    dd = lib.edit_distance_batch([pairs[i] for i in todo], device=device, max_dist=[bounds[i] for i in todo]) if todo else []
    t_align = time.perf_counter() - t0
    t0 = time.perf_counter()
    accepted = set()
    for i, d in zip(todo, np.asarray(dd).tolist()):
        svlen = int(table["v_svlen"][owner[i][1]])
        if d >= 0 and (svlen - d) / svlen > pct:
            accepted.add(owner[i])
    for k, sv in enumerate(survivors):
        if sv is None or len(sv[0]) == 0:
            continue
        gi, d = sv
        if table["list_is_ins"][int(q["list"][k])] and pct:
            keep = np.fromiter(((k, int(g)) in accepted for g in gi), bool, len(gi))
            gi, d = gi[keep], d[keep]
        if len(gi):
            j = int(np.argmin(d))                       # the first among equals
            best[k], dist[k] = gi[j], d[j]
    t_pick = time.perf_counter() - t0
    cells = sum(len(pairs[i][0]) * len(pairs[i][1]) for i in todo)
    return best, dist, dict(gate_ms=t_gate * 1e3, align_call_ms=t_align * 1e3, pick_ms=t_pick * 1e3, alignments=len(todo), dp_cells=cells)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--samples", type=int, default=10)
    ap.add_argument("--coverage", type=float, default=15.0)
    ap.add_argument("--scale", type=float, default=0.05, help="fraction of the GRCh38 contig lengths")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    rounds = max(3, args.rounds)
    from sniffles_amd import candstore, lib, parallel, snfp, synth, vcf
    from sniffles_amd.config import SnifflesConfig
    from tools.bench_common import emu_lib
    from tools.bench_population import build_sample
    emu_lib()                                            # SNF_BENCH_EMU=1: the test suite's host tier (plumbing only, never a result)

    S = max(2, args.samples)
    contigs = [(ci, c, max(200000, int(synth.GRCH38[c] * args.scale))) for ci, c in enumerate(synth.CONTIGS)]
    call_cfg = SnifflesConfig()
    readers, n_cands = {}, 0
    for s in range(S):
        tasks = [synth.gen_task(ci, c, L, args.coverage, seed=100 + s, site_seed=501) for ci, c, L in contigs]
        readers[s], n = build_sample(call_cfg, tasks, args.device, s)
        n_cands += n

    def config(population=None):
        cfg = SnifflesConfig()
        cfg.mode = "combine"
        cfg.snf_input_info = [dict(internal_id=s, sample_id=f"S{s}") for s in range(S)]
        cfg.sample_ids_vcf = [(s, f"S{s}") for s in range(S)]
        cfg.combine_population = population
        return cfg

    def merge_tasks(cfg):
        return [parallel.CombineTask(id=ci, sv_id=0, contig=c, start=0, end=L - 1, config=cfg, device=args.device) for ci, c, L in contigs]
    # ---- the population file of this very population, by the new writer
    cfg = config()
    pop_path = os.path.join(tempfile.mkdtemp(prefix="bench_popmatch_"), "population.snf")
    out = snfp.PopulationWriter(pop_path, cfg)
    tasks = merge_tasks(cfg)
    n_calls = 0
    for task, calls in zip(tasks, parallel.CombineTask.execute_many(tasks, readers)):
        out.add_task(task.id, task.contig, calls)
        n_calls += len(calls)
    n_variants = out.finish([c for _, c, _ in contigs])
    # ---- the annotated merge: text path; the queries of its one launch are kept for the baseline
    cfg = config(pop_path)
    seen = {}
    real = lib.population_match_batch

    def recording(config_, table, queries, device=0):
        t0 = time.perf_counter()
        r = real(config_, table, queries, device=device)
        seen.update(table=table, queries=queries, result=r, call_ms=(time.perf_counter() - t0) * 1e3)
        return r
    lib.population_match_batch = recording
    merges = []
    try:
        for _ in range(2):                               # the first one opens the file and grows the arena
            w = vcf.VCF(cfg, io.TextIOWrapper(io.BytesIO(), encoding="utf-8", newline="", write_through=True))
            t0 = time.perf_counter()
            n_rec = sum(w.write_merged(part) for part in parallel.CombineTask.execute_many(merge_tasks(cfg), readers, text_writer=w))
            merges.append(dict(merge_ms=(time.perf_counter() - t0) * 1e3, population_step_ms=candstore.last_timing.get("population_gpu", 0.0) * 1e3,
                               records=n_rec))
    finally:
        lib.population_match_batch = real
    table, q = seen["table"], seen["queries"]
    want_best, want_dist = seen["result"]
    n_q = len(q["alt_off"]) - 1
    log = []
    for r in range(rounds):                              # alternating, one session
        t0 = time.perf_counter()
        best, dist = lib.population_match_batch(cfg, table, q, device=args.device)
        new_ms = (time.perf_counter() - t0) * 1e3
        st = lib.population_last_stats(args.device)
        t0 = time.perf_counter()
        b_best, b_dist, bst = baseline(lib, cfg, table, q, args.device)
        base_ms = (time.perf_counter() - t0) * 1e3
        same = bool(np.array_equal(best, b_best) and np.array_equal(dist, b_dist) and np.array_equal(best, want_best))
        row = dict(round=r, new_call_ms=round(new_ms, 3), new_kernel_ms=round(st["kernel_ms"], 3), new_alignments=st["alignments"],
                   new_dp_cells=st["dp_cells"], new_staged_bytes=st["staged_bytes"], baseline_ms=round(base_ms, 3),
                   baseline_align_call_ms=round(bst["align_call_ms"], 3), baseline_gate_ms=round(bst["gate_ms"], 3),
                   baseline_pick_ms=round(bst["pick_ms"], 3), baseline_alignments=bst["alignments"], baseline_dp_cells=bst["dp_cells"],
                   same_answer=same)
        log.append(row)
        print(json.dumps(row), flush=True)
    med = lambda k: float(np.median([row[k] for row in log]))  # noqa: E731
    print(json.dumps(dict(
        workload=f"population merge: {S} samples at {args.coverage:g}x, scale {args.scale:g}, {len(contigs)} contig tasks; annotated against its own "
                 f"population file", candidates=n_cands, merged_calls=n_calls, population_variants=n_variants, queries=n_q,
        matched=int((want_best >= 0).sum()), lists=int(len(table["list_off"]) - 1), longest_list=int(np.diff(table["list_off"]).max(initial=0)),
        rounds=rounds, same_answer=all(row["same_answer"] for row in log),
        new=dict(call_ms=med("new_call_ms"), kernel_ms=med("new_kernel_ms"), alignments=log[-1]["new_alignments"], dp_cells=log[-1]["new_dp_cells"]),
        baseline=dict(total_ms=med("baseline_ms"), align_call_ms=med("baseline_align_call_ms"), gate_ms=med("baseline_gate_ms"),
                      alignments=log[-1]["baseline_alignments"], dp_cells=log[-1]["baseline_dp_cells"]),
        merge=dict(merge_ms=round(merges[-1]["merge_ms"], 2), population_step_ms=round(merges[-1]["population_step_ms"], 2),
                   share=round(merges[-1]["population_step_ms"] / merges[-1]["merge_ms"], 4), records=merges[-1]["records"],
                   first_merge_ms=round(merges[0]["merge_ms"], 2), first_population_step_ms=round(merges[0]["population_step_ms"], 2)))))


if __name__ == "__main__":
    main()
