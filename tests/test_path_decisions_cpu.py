"""recovery_rl_amd/paths.py: the switch table is complete, and every decision made from it equals what the code before the
table decided -- tests/golden/path_decisions.json, written by profiles/path_decisions.py in a checkout of that commit."""
import glob
import json
import os
import re
import sys

import pytest

from recovery_rl_amd import paths

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
import path_decisions as PD  # noqa: E402

# the variables of the package that are no boolean switches: integers, strings and a library path, read where they are used
NOT_BOOLEAN = {"RRL_PACK_PAIR_BLOCK_MAX_SEEDS", "RRL_HIP_LIB", "RRL_DIST_BACKEND", "RRL_GRAPH_PACKET_CAPTURE"}


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(HERE, "golden", "path_decisions.json")))


def test_the_record_covers_the_grids_the_script_states(golden):
    assert golden["values_of"] == json.loads(json.dumps(PD.VALUES))
    assert set(golden["grids"]) == set(PD.GRIDS)
    for name, (switches, axes) in PD.GRIDS.items():
        g = golden["grids"][name]
        assert (g["switches"], g["axes"]) == (switches, axes), name
        want = 3 ** len(switches)
        for a in axes:
            want *= len(PD.VALUES.get(a, PD.BOOL))
        assert g["rows"] == want == len(PD.decode(g)), name
    assert {tuple(v) for v in golden["values_of"]["given"]} == {(a, b) for a in (False, True) for b in (False, True)}
    assert golden["values_of"]["seeds_per_gpu"] == [2, 8, 9] and golden["values_of"]["num_envs"] == [1, 4]
    assert golden["values_of"]["hidden_size"][0] == 256 and len(golden["values_of"]["env_name"]) == 4


@pytest.mark.parametrize("name", sorted(PD.GRIDS))
def test_every_decision_is_the_parents(golden, name):
    """Every row of the grid, replayed on this code: the same path, scoring or refusal text (byte for byte), or no refusal."""
    g = golden["grids"][name]
    want = PD.decode(g)
    call = PD.calls()[name]
    saved = {s: os.environ.get(s) for s in g["switches"]}
    try:
        i = -1
        for i, (env, cfg) in enumerate(PD.rows(g["switches"], g["axes"])):
            got = call(cfg)
            if got != want[i]:
                pytest.fail("%s row %d: %r, the parent decided %r\n  environment %s\n  cfg %s" % (
                    name, i, got, want[i], dict(zip(g["switches"], env)), {a: getattr(cfg, a) for a in g["axes"]}))
        assert i + 1 == len(want)
    finally:
        for s, v in saved.items():
            os.environ.pop(s, None) if v is None else os.environ.__setitem__(s, v)


def test_the_record_holds_refusals_and_both_paths(golden):
    """The grids reach what they are there for: both answers of every path function, and each refusal of the two ladders (but
    "a run without --use_constraint_sampling": with that flag SQRL's ladder, which comes first, always refuses)."""
    for name, g in golden["grids"].items():
        if name != "run_packed":
            assert sorted(map(str, g["values"])) in (["hip", "modules"], ["f16x3", "f32"], ["False", "True"]), name
    texts = [t for t in golden["grids"]["run_packed"]["values"] if t]
    assert None in golden["grids"]["run_packed"]["values"]
    for piece in ("set RRL_FAST_SQRL=1", "set RRL_FAST_BASELINES=1", "a run without a recovery policy", "the kernel's Q_risk width; got 32",
                  "rrl_sqrl_act kernel (Gaussian policy, fixed alpha", "seeds; got 9", "set RRL_FAST_QSAMPLE=1", "a run without --MF_recovery",
                  "the kernels' Q_risk width; got 32",
                  "rrl_qsample_act kernels (Gaussian policy, fixed alpha", "does not pack --use_constraint_sampling"):
        assert any(piece in t for t in texts), piece


# ---- the table ---------------------------------------------------------------------------------------------------------
def test_every_switch_the_package_reads_is_a_row_or_a_named_exception():
    names = {s.name for s in paths.SWITCHES}
    assert len(names) == len(paths.SWITCHES)
    read, asked = set(), set()
    for path in glob.glob(os.path.join(ROOT, "recovery_rl_amd", "*.py")):
        src = open(path).read()
        read |= set(re.findall(r"environ(?:\.get\(|\[|\.setdefault\(|\.pop\()\s*[\"'](RRL_[A-Z0-9_]+)", src))
        read |= set(re.findall(r"[\"'](RRL_[A-Z0-9_]+)[\"']\s+(?:not\s+)?in\s+os\.environ", src))
        asked |= set(re.findall(r"\bswitch\(\s*[\"'](RRL_[A-Z0-9_]+)", src))
    assert read and read <= names | NOT_BOOLEAN, sorted(read - names - NOT_BOOLEAN)
    assert not read & names, "a table row is read outside paths.switch: %s" % sorted(read & names)
    assert asked <= names, sorted(asked - names)                   # paths.switch("...") names rows only


def test_every_row_is_documented():
    readme = open(os.path.join(ROOT, "README.md")).read()
    for s in paths.SWITCHES:
        assert s.name in readme, s.name
        assert s.rule in (paths.ON, paths.NOT_OFF, paths.SET) and s.doc.endswith(".") and s.read
        assert any(s.read.startswith(when) for when in (paths.IMPORT, paths.LOOP, paths.EXPERIMENT, paths.CALL)), s


@pytest.mark.parametrize("rule,unset,empty,zero,one,other", [
    (paths.ON, False, False, False, True, False), (paths.NOT_OFF, True, True, False, True, True),
    (paths.SET, False, False, False, True, True)])
def test_each_row_keeps_its_parsing_rule(monkeypatch, rule, unset, empty, zero, one, other):
    rows = [s for s in paths.SWITCHES if s.rule == rule]
    assert rows
    for s in rows:
        monkeypatch.delenv(s.name, raising=False)
        assert paths.switch(s.name) is unset
        for val, want in (("", empty), ("0", zero), ("1", one), ("yes", other)):
            monkeypatch.setenv(s.name, val)
            assert paths.switch(s.name) is want, (s.name, val)
    assert {s.name for s in paths.SWITCHES if s.rule == paths.NOT_OFF} == {"RRL_W2_FRAG", "RRL_CARRY_ACTOR", "RRL_DRAW_AHEAD"}
    assert {s.name for s in paths.SWITCHES if s.rule == paths.SET} == {"RRL_PLAN_F16X3", "RRL_ROCTX", "RRL_DIST_FORCE_INIT"}


def test_paths_imports_neither_torch_nor_the_library():
    import subprocess
    code = ("import importlib.util, sys; spec = importlib.util.spec_from_file_location('paths', %r); "
            "m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m); "
            "assert 'torch' not in sys.modules and 'ctypes' not in sys.modules, sorted(sys.modules)"
            % os.path.join(ROOT, "recovery_rl_amd", "paths.py"))
    subprocess.run([sys.executable, "-c", code], check=True, timeout=60)


def test_the_pinned_names_stay_importable_from_fast_update():
    from recovery_rl_amd import fast_update
    for name in ("fast_baselines_enabled", "fast_sqrl_enabled", "fast_qsample_enabled", "fast_eval_enabled", "fast_eval_maze_enabled",
                 "fast_eval_qsample_enabled", "fast_eval_sqrl_enabled", "pack_sqrl_enabled", "pack_qsample_enabled",
                 "sqrl_f16x3_enabled", "qsample_f16x3_enabled", "eval_sqrl_f16x3_enabled", "eval_qsample_f16x3_enabled",
                 "sqrl_acting_path", "qsample_acting_path", "sqrl_scoring", "qsample_scoring", "eval_rollout_path", "eval_scoring",
                 "eval_sqrl_line", "eval_qsample_line", "fast_path_supported", "uses_baseline_terms", "BASELINE_FLAGS"):
        assert getattr(fast_update, name) is getattr(paths, name), name
