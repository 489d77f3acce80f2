"""The placement of the packed launches (csrc/pack.hpp: place + locate, place_members + locate_grid) walked on the host, in a
stand-alone program built with the host sanitizers (tests/pack_placement_main.hip holds the cases and the properties).  The
program runs as a child process, once per setting of RRL_PACK_PINNED: the switch is read once per process."""
import os
import subprocess

import pytest

from recovery_rl_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
# which S get a pinned mapping: pack.hpp's table (tests/test_stack_forward_cpu.py restates it); the switch adds 5 and 6
PINNED = {"": [1, 2, 3, 4, 7, 8, 14, 15, 16], "1": [1, 2, 3, 4, 5, 6, 7, 8, 14, 15, 16]}


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path_factory.mktemp("placement") / "pack_placement")
    cmd = [hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=undefined", "-I", _lib.INCLUDE, "-I", _lib.CSRC, "-o", exe,
           os.path.join(HERE, "pack_placement_main.hip")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


@pytest.mark.parametrize("pinned", ["", "1"], ids=["default", "always_pinned"])
def test_every_seed_workgroup_is_placed_exactly_once_on_the_smallest_grid(program, pinned):
    env = {k: v for k, v in os.environ.items() if k != "RRL_PACK_PINNED"}
    if pinned:
        env["RRL_PACK_PINNED"] = pinned
    r = subprocess.run([program], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    lines = dict(line.split(":", 1) for line in r.stdout.splitlines() if ":" in line)
    assert [int(s) for s in lines["pinned"].split()] == PINNED[pinned]
    assert int(lines["failures"]) == 0 and int(lines["patterns"]) == 16 * (7 + 9 + 2 + 8)
