"""The caller arrays of a solve as cilqr_amd/csrc/solve_io.hpp states them, on the host: the widths per problem, problems
[b0, b1) of a batch (lane groups, shards), the packed input and output staging blocks of HOST arrays and the hand-out of
the output block.  No GPU involved: the header has no HIP dependency, which building it with g++ alone also pins.  What the
same statements carry on a GPU is held in tests/test_gpu_solve_io_edges.py."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layouts_slices_and_hand_out_under_address_sanitizer(tmp_path):
    """tests/cpp/solve_io_test.cc, built with -fsanitize=address,undefined and run as a child process: every offset and
    size of both blocks against byte counts worked out from the array shapes (B = 1 plain, with station, with warm rows of
    each layout with and without shift, outputs with and without iterates and alpha trace, odd B and M for the pad, either
    side of 4 MiB), the first and last element of every array of a sub-range (arrays of exactly their size, so a width
    one too large is a heap overflow), null members staying null, and the scatter of live Cost rows from packed and from
    dense rows for n_cost of 0, 1, M + 1, negative and beyond M + 1 into an array whose other rows must stay untouched."""
    exe = tmp_path / "solve_io_test"
    # (the runtimes linked statically: the program then does not care what else a machine loads into its processes)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-I" + os.path.join(ROOT, "cilqr_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "solve_io_test.cc"), "-o", str(exe)])
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    m = re.fullmatch(r"(\d+) checks, 0 failures", run.stdout.strip())
    assert m and int(m.group(1)) > 1000, run.stdout
