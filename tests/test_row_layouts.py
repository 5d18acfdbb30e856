"""Where a row layout keeps what a rule names, as include/cilqr/row_layouts.hpp states it once, on the host.  Host and
device read that one table, so a wrong table agrees with itself; tests/cpp/row_layouts_test.cc holds it against the numbers
written out a second time.  No GPU involved; what the same table carries on a GPU is held in tests/test_gpu_row_layouts.py."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_table_rules_and_warm_geometry_under_address_sanitizer(tmp_path):
    """tests/cpp/row_layouts_test.cc, built with g++ alone and -fsanitize=address,undefined and run as a child process: the
    five layouts against the columns include/cilqr.h documents, as literals; for every rule (resample, carry, frenet, track,
    margins, the audits, the kernels templated on the row width) the columns it reads against the tuples it hard-coded
    before the table; the map from trajectory to plan rows against {0,-1,1,2,3,7,4,5,6,8,9}; the warm geometry against
    (10, K, 8), (11, K, 9), (2, K - 1, 0) and its refusal of COARSE and POINTS; unknown layouts (-1, 5, and 3 or 4 where
    the entry point does not take them) against fields == 0 or the refusal."""
    exe = tmp_path / "row_layouts_test"
    # (the runtimes linked statically: the program then does not care what else a machine loads into its processes)
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "cilqr_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "row_layouts_test.cc"), "-o", str(exe)])
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    m = re.fullmatch(r"(\d+) checks, 0 failures", run.stdout.strip())
    assert m and int(m.group(1)) > 200, run.stdout
