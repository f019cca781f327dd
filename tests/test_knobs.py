"""The library's environment switches (sniffles_amd/csrc/snf_knobs.h): a handle takes its switches from the environment at
snf_batch_create and keeps them; the README's table lists exactly the switches the sources read."""
import os
import re

from sniffles_amd import lib, records, synth
from sniffles_amd.config import SnifflesConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def forms_lines(capfd):
    return [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("[SNF_PROF] forms:")]


def test_a_handle_keeps_the_switches_of_its_creation(oracle_mod, monkeypatch, capfd):
    """Three handles open at once, each created under another environment; their passes run after the environment has been emptied
    again.  Every handle reports (the [SNF_PROF] forms line of its upload) and runs the forms its own environment asked for."""
    import emu.emu as E
    E.lib()
    tis = [synth.gen_fuzz(4242 + k, task_id=k) for k in range(3)] + [synth.gen_task(3, "chrS", 150_000, 40.0, seed=5)]
    cfg = SnifflesConfig()
    exp = records.records(oracle_mod.run(cfg, tis, True), tis, "final")
    for name in ("SNF_NO_WAVE", "SNF_D4"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("SNF_PROF", "1")
    capfd.readouterr()
    handles, forms = [], []
    try:
        for env in ({}, {"SNF_NO_WAVE": "1"}, {"SNF_D4": "thread"}):
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            handles.append(lib.Batch(cfg, tis))
            forms.append(forms_lines(capfd))
            for k in env:
                monkeypatch.delenv(k)
        monkeypatch.delenv("SNF_PROF")
        for b in handles:                                 # first pass of each, then the second: the environment is empty throughout
            b.run_pass()
            assert records.records(b.fetch(1), tis, "final") == exp
        for b in handles:
            b.call_candidates(); b.finalize()
            assert records.records(b.fetch(1), tis, "final") == exp
    finally:
        for b in handles:
            b.close()
    assert [len(f) for f in forms] == [1, 1, 1], forms
    assert "forms: wave path," in forms[0][0] and "coverage by d4s_coverage," in forms[0][0], forms[0]
    assert "forms: thread path," in forms[1][0], forms[1]
    assert "forms: wave path," in forms[2][0] and "coverage by d4_coverage," in forms[2][0], forms[2]


def table_names(section):
    """First column of the README's switch table, the rows whose scope column is one of `section`."""
    with open(os.path.join(ROOT, "README.md")) as f:
        rows = [ln.split("|") for ln in f if ln.startswith("| `SNF_")]
    names = [re.fullmatch(r"\s*`(SNF_[A-Z0-9_]+)`\s*", r[1]).group(1) for r in rows if r[2].strip() in section]
    assert len(names) == len(set(names)), sorted(n for n in names if names.count(n) > 1)
    return set(names)


def test_readme_table_lists_the_switches_the_sources_read():
    csrc = os.path.join(ROOT, "sniffles_amd", "csrc")
    with open(os.path.join(csrc, "snf_knobs.h")) as f:
        code = "\n".join(ln.split("//")[0] for ln in f)                  # (comments name switches too)
    read_by_lib = set(re.findall(r'\(\s*"(SNF_[A-Z0-9_]+)"', code))      # the string literals handed to getenv / the env_* helpers
    for name in os.listdir(csrc):                                         # ... and nothing else under csrc/ reads the environment
        if name != "snf_knobs.h":
            with open(os.path.join(csrc, name), errors="replace") as f:
                assert "getenv" not in f.read(), name
    assert len(read_by_lib) == 60
    assert table_names({"process", "handle", "entry point"}) == read_by_lib
    read_by_py = set()
    pkg = os.path.join(ROOT, "sniffles_amd")
    for name in os.listdir(pkg):
        if name.endswith(".py"):
            with open(os.path.join(pkg, name)) as f:
                read_by_py |= set(re.findall(r'environ(?:\.get|\.setdefault|\.pop)?[\[(]\s*"(SNF_[A-Z0-9_]+)"', f.read()))
    assert table_names({"Python"}) == read_by_py - read_by_lib               # (server.py sets SNF_STAGE_ARENA_MB for the library)
