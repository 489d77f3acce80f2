"""The checks behind csrc/ens_model.hpp (the ensemble's model and loss stated once for both training entries), for whichever
library RRL_HIP_LIB names (default: the in-tree one):
    python profiles/ens_model_once.py dump OUT.pt          every case of tests/ens_train_cases.py at its seed: all output buffers
    python profiles/ens_model_once.py compare A.pt B.pt    differing elements per case and buffer (bit compare); exit 1 if any
    python profiles/ens_model_once.py ab PARENT.so [runs] [OUT.json]
                                                           ens_train_probe.py and ens_big_probe.py, parent library and in-tree
                                                           one alternating, a fresh process per run -> every run, the medians,
                                                           the parent's min-max spread"""
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def dump(out):
    import torch
    import ens_train_cases as EC
    res = {}
    for name in EC.names():
        c = EC.BY_NAME[name]
        b = EC.Device(EC.operands(name), "cuda:0").run(c.entry)
        res[name] = {f: b[f + "_flat"].cpu() for f in EC.OUTPUT_FIELDS}
    torch.save(res, out)
    print("dumped %d cases x %d buffers to %s" % (len(res), len(EC.OUTPUT_FIELDS), out))


def compare(pa, pb):
    import torch
    a, b = torch.load(pa), torch.load(pb)
    assert set(a) == set(b) and len(a) > 0
    diff = {}
    for name in sorted(a):
        for f in a[name]:
            n = int((a[name][f].view(torch.int32) != b[name][f].view(torch.int32)).sum())
            if n:
                diff["%s %s" % (name, f)] = n
    print(json.dumps({"cases": len(a), "buffers_per_case": len(next(iter(a.values()))), "differing_elements": sum(diff.values()),
                      "where": diff}))
    return 1 if diff else 0


def probe(script, lib):
    env = dict(os.environ)
    env.pop("RRL_HIP_LIB", None)
    if lib:
        env["RRL_HIP_LIB"] = lib
    r = subprocess.run([sys.executable, os.path.join(ROOT, "profiles", script)], env=env, capture_output=True, text=True,
                       timeout=240)
    if r.returncode != 0:
        sys.exit("%s failed (%d) with %r:\n%s" % (script, r.returncode, lib, r.stderr[-2000:]))
    return r.stdout


def ab(parent, runs, out):
    parent = os.path.abspath(parent)
    res = {"parent": {}, "branch": {}}
    for i in range(runs):
        for who, lib in (("parent", parent), ("branch", "")):
            text = probe("ens_train_probe.py", lib)
            small = {"small_epoch_us_per_step": float(re.search(r"step: ([\d.]+) us", text).group(1)),
                     "small_grad_us_per_launch": float(re.search(r"launch: ([\d.]+) us", text).group(1))}
            big = json.loads(probe("ens_big_probe.py", lib).strip().splitlines()[-1])
            small.update(big_step_ms=big["hip_step_ms"], big_grad_ms=big["hip_grad_only_ms"])
            for k, v in small.items():
                res[who].setdefault(k, []).append(v)
            print(i, who, small, flush=True)
    verdict = {}
    for k, pv in res["parent"].items():
        med = statistics.median(res["branch"][k])
        verdict[k] = {"parent_median": statistics.median(pv), "parent_min": min(pv), "parent_max": max(pv), "branch_median": med,
                      "branch_median_within_parent_spread": min(pv) <= med <= max(pv), "branch_not_slower": med <= max(pv)}
    res["verdict"] = verdict
    res["parent_so"] = parent
    text = json.dumps(res, indent=1)
    print(text)
    if out:
        open(out, "w").write(text + "\n")


if __name__ == "__main__":
    mode = sys.argv[1]
    if mode == "dump":
        dump(sys.argv[2])
    elif mode == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        ab(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 5, sys.argv[4] if len(sys.argv) > 4 else None)
