"""No GPU: the host half of the lab stage harness (frankensearch_amd/csrc/lab_guard.hpp: guard bands and bodies of an output, guard rows
behind a slab, the padded bitmap), checked by tests/host/lab_guard_check.cpp — a plain program built here with the address and
undefined-behaviour sanitizers and run as a child process.  A wrong offset in that header would let a stage test stop seeing
out-of-bounds writes while staying green; this is the test of the harness itself."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "frankensearch_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
def test_lab_guard_header_under_host_sanitizers(tmp_path):
    exe = str(tmp_path / "lab_guard_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                            "-I", CSRC, os.path.join(ROOT, "tests", "host", "lab_guard_check.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip() == "lab_guard_check: ok" and not run.stderr, (run.returncode, run.stdout, run.stderr)
    # the header stays host-only: no HIP header, so that g++ alone compiles it
    text = open(os.path.join(CSRC, "lab_guard.hpp")).read()
    assert "#include <hip" not in text and "hip_runtime" not in text
    # and LabStage goes through it: the logic exists once
    lab = open(os.path.join(CSRC, "fsgpu_lab_api.cpp")).read()
    assert lab.count("struct Out") == 0 and text.count("struct Out") == 1
    for name in ("lab::collect_out(", "lab::with_guard_tail(", "lab::padded_bitmap("):
        assert lab.count(name) == 1, name
