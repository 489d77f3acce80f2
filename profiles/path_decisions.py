"""The decisions of the acting, evaluation and packing switches over a grid of environments and configurations, as a record the
suite replays (tests/test_path_decisions_cpu.py against tests/golden/path_decisions.json).  No GPU.

    python profiles/path_decisions.py [ROOT]      # ROOT: the checkout whose decisions are recorded (default: this one)

The committed record was written with ROOT = a checkout of the commit BEFORE the switch readers moved into
recovery_rl_amd/paths.py: it says what that code decided, not what the present code decides.  It goes through the names that commit
and every later one export from fast_update / experiment, so the same file records either.

A grid is (switches, axes): every switch at unset / "0" / "1", times every value of every axis, in itertools.product order, the
switches first.  The axes are cfg fields (`given`, eval_scoring's second argument, rides on the cfg as one more).  The four
acting functions and fast_path_supported get every switch and every cfg field they read, two values each.  The evaluation
functions and run_packed read as many again through fast_path_supported, and the full product (3e7 .. 6e8 rows) is out of a test's
reach: their grids take every switch they read and every field their OWN body (run_packed: the body of its two acting-pass
ladders) reads, and `policy` -- Gaussian or not -- stands for the nine fields of fast_path_supported, whose own grid is complete.
The outputs are one byte per row (the index into "values"), deflated, in base64.
"""
import base64
import itertools
import json
import os
import sys
import types
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "..", "tests", "golden", "path_decisions.json")

BOOL = (False, True)
VALUES = {"hidden_size": (256, 32), "env_name": ("navigation1", "navigation2", "maze", "other"), "num_envs": (1, 4),
          "policy": ("Gaussian", "Deterministic"), "target_update_interval": (1, 2), "seeds_per_gpu": (2, 8, 9),
          "given": ((False, False), (False, True), (True, False), (True, True))}
BASE = dict(policy="Gaussian", automatic_entropy_tuning=False, target_update_interval=1, cnn=False, DGD_constraints=False,
            update_nu=False, nu_schedule=False, use_constraint_sampling=False, RCPO=False, use_recovery=False, MF_recovery=False,
            Q_sampling_recovery=False, hidden_size=256, no_fast_path=False, env_name="navigation1", num_envs=4, seeds_per_gpu=2,
            dp_mode="replicas", resume="", checkpoint_every=0, seed=1, logdir_suffix="", given=None)

FUSED = ["policy", "automatic_entropy_tuning", "DGD_constraints", "update_nu", "nu_schedule", "use_constraint_sampling", "RCPO",
         "target_update_interval", "cnn"]
SQRL = ["use_recovery", "hidden_size", "no_fast_path"] + FUSED
QSAMPLE = ["use_recovery", "Q_sampling_recovery", "MF_recovery", "hidden_size", "no_fast_path"] + FUSED
EVAL = ["use_constraint_sampling", "use_recovery", "MF_recovery", "Q_sampling_recovery", "hidden_size", "no_fast_path", "env_name",
        "num_envs", "policy"]
EVAL_SWITCHES = ["RRL_FAST_EVAL", "RRL_FAST_EVAL_MAZE", "RRL_FAST_EVAL_QSAMPLE", "RRL_FAST_EVAL_SQRL", "RRL_FAST_BASELINES"]
GRIDS = {
    "fast_path_supported": (["RRL_FAST_BASELINES"], FUSED),
    "sqrl_acting_path": (["RRL_FAST_SQRL", "RRL_FAST_BASELINES", "RRL_W2_FRAG"], SQRL),
    "sqrl_scoring": (["RRL_SQRL_F16X3", "RRL_FAST_SQRL", "RRL_FAST_BASELINES", "RRL_W2_FRAG"], SQRL),
    "qsample_acting_path": (["RRL_FAST_QSAMPLE", "RRL_FAST_BASELINES", "RRL_W2_FRAG"], QSAMPLE),
    "qsample_scoring": (["RRL_QSAMPLE_F16X3", "RRL_FAST_QSAMPLE", "RRL_FAST_BASELINES", "RRL_W2_FRAG"], QSAMPLE),
    "eval_rollout_path": (EVAL_SWITCHES, EVAL),
    "eval_scoring": (["RRL_EVAL_SQRL_F16X3", "RRL_EVAL_QSAMPLE_F16X3"] + EVAL_SWITCHES, EVAL),
    "eval_scoring_given": (EVAL_SWITCHES, ["given"] + EVAL),
    "run_packed": (["RRL_PACK_SQRL", "RRL_PACK_QSAMPLE", "RRL_FAST_SQRL", "RRL_FAST_QSAMPLE", "RRL_FAST_BASELINES", "RRL_W2_FRAG"],
                   ["seeds_per_gpu", "num_envs", "use_constraint_sampling", "use_recovery", "Q_sampling_recovery", "MF_recovery",
                    "hidden_size", "no_fast_path", "policy"]),
}


class _Built(Exception):
    """run_packed refused nothing and went on to build its first Experiment."""


def calls():
    """name -> f(cfg) -> a JSON value, on the package that is importable now."""
    from recovery_rl_amd import experiment, fast_update as fu

    def built(cfg):
        raise _Built()

    def run_packed(cfg):
        real, experiment.Experiment = experiment.Experiment, built
        try:
            experiment.run_packed(cfg)
        except ValueError as err:
            return str(err)
        except _Built:
            return None
        finally:
            experiment.Experiment = real
        raise AssertionError("run_packed returned without building an Experiment")

    out = {name: getattr(fu, name) for name in GRIDS if hasattr(fu, name)}
    out["eval_scoring_given"] = lambda cfg: fu.eval_scoring(cfg, cfg.given)
    out["run_packed"] = run_packed
    return out


def rows(switches, axes):
    """Every (environment, cfg) of a grid, in the record's order; the cfg is one object, rewritten for every row."""
    cfg = types.SimpleNamespace(**BASE)
    for env in itertools.product((None, "0", "1"), repeat=len(switches)):
        for name, val in zip(switches, env):
            if val is None:
                os.environ.pop(name, None)
            else:
                os.environ[name] = val
        for point in itertools.product(*[VALUES.get(a, BOOL) for a in axes]):
            for a, v in zip(axes, point):
                setattr(cfg, a, v)
            yield env, cfg


def decide(name, switches, axes, call):
    """The grid's outputs in order (the environment is put back afterwards)."""
    saved = {s: os.environ.get(s) for s in switches}
    try:
        return [call(cfg) for _, cfg in rows(switches, axes)]
    finally:
        for s, v in saved.items():
            os.environ.pop(s, None) if v is None else os.environ.__setitem__(s, v)


def encode(outputs):
    """One byte per row (the index into "values"), deflated, base64 in lines of 200 characters."""
    values = []
    for o in outputs:
        if o not in values:
            values.append(o)
    text = base64.b64encode(zlib.compress(bytes(values.index(o) for o in outputs), 9)).decode()
    return {"values": values, "rows_deflated": [text[i:i + 200] for i in range(0, len(text), 200)]}


def decode(rec):
    return [rec["values"][i] for i in zlib.decompress(base64.b64decode("".join(rec["rows_deflated"])))]


def main():
    root = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, ".."))
    sys.path.insert(0, root)
    import recovery_rl_amd
    assert os.path.dirname(os.path.dirname(os.path.abspath(recovery_rl_amd.__file__))) == root, recovery_rl_amd.__file__
    for name in [n for n in os.environ if n.startswith("RRL_")]:
        del os.environ[name]
    fns = calls()
    record = {"values_of": {k: list(v) for k, v in VALUES.items()}, "grids": {}}
    for name, (switches, axes) in GRIDS.items():
        out = decide(name, switches, axes, fns[name])
        record["grids"][name] = dict(switches=switches, axes=axes, rows=len(out), **encode(out))
        print("%-22s %8d rows, %d values" % (name, len(out), len(record["grids"][name]["values"])))
    with open(OUT, "w") as f:       # (JSON, one line per grid's description and per 200 characters of its rows)
        f.write('{"values_of": %s,\n "grids": {\n' % json.dumps(record["values_of"]))
        for k, (name, g) in enumerate(record["grids"].items()):
            rows = g.pop("rows_deflated")
            f.write('  %s: %s, "rows_deflated": [\n' % (json.dumps(name), json.dumps(g)[:-1]))
            f.write(",\n".join("   " + json.dumps(t) for t in rows))
            f.write("]}%s\n" % ("," if k + 1 < len(record["grids"]) else ""))
        f.write(" }\n}\n")
    print("wrote %s (%d bytes)" % (os.path.normpath(OUT), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
