"""The owning type every resource of a handle lives in (csrc/owned.h), on the CPU: a resource is released exactly once -- by the
destructor, by reset() or when another owner is moved in --, never by release() or by an empty owner, and a group that is built in
locals and fails half way releases what it had and leaves the group attached before untouched.

The checks are a stand-alone program (tests/host/owned_main.cpp) with a counting release function, compiled here with the host compiler
and its address and undefined-behaviour sanitizers: a double release, a leak or a use after release ends it with a report.  Nothing of
it is loaded into this process."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "robot-control-stack_amd", "csrc")


def test_an_owner_releases_exactly_once(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no host C++ compiler"
    prog = str(tmp_path / "owned")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-I{CSRC}",
                           os.path.join(ROOT, "tests", "host", "owned_main.cpp"), "-o", prog])
    run = subprocess.run([prog], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().splitlines()[-1] == "ok"
