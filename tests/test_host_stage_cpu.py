"""The layout of the host-pointer calls over a grown device buffer (csrc/host_stage.h), on the CPU: for the declaration lists of all
eight call sites, at n = 1, 5 and 67 and with each optional array absent in turn, the slices lie in declaration order, disjoint and
8-byte aligned; an absent array takes no bytes and has a null view; the total is the end of the last slice; an output that is staged
whatever the caller asked for keeps its slice, and no download, when the caller passed null.

The checks are a stand-alone program (tests/host/host_stage_main.cpp), compiled here with the host compiler and its address and
undefined-behaviour sanitizers: it writes every slice of every layout into a heap block of exactly the layout's total, so a slice past
the end ends it with a report.  Nothing of it is loaded into this process."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "robot-control-stack_amd", "csrc")


def test_slices_are_ordered_disjoint_and_aligned(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no host C++ compiler"
    prog = str(tmp_path / "host_stage")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-I{CSRC}",
                           os.path.join(ROOT, "tests", "host", "host_stage_main.cpp"), "-o", prog])
    run = subprocess.run([prog], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().splitlines()[-1] == "ok"
