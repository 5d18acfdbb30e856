"""The stop rule as the header states it (include/cilqr/trajectory_queries.hpp: stop_rows), alone and under the sanitizers
of the host compiler.  No GPU and no library involved: tests/test_stop.py holds the C-ABI call to the NumPy statement,
tests/test_gpu_stop.py the kernel to the call."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_statement_under_address_sanitizer(tmp_path):
    """tests/cpp/stop_rows_test.cc, built with g++ alone and -fsanitize=address,undefined and run as a child process: arrays
    of exactly their size at n_knots = 2, 51, 256 and n_out = 1, 2, 256 in every layout, the exact dyadic cases, every
    status, the zero rows of a refusal, the pose against resample_rows."""
    exe = tmp_path / "stop_rows_test"
    # (the runtimes linked statically: the program then does not care what else a machine loads into its processes)
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "stop_rows_test.cc"), "-o", str(exe)])
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    m = re.fullmatch(r"(\d+) checks, 0 failures", run.stdout.strip())
    assert m and int(m.group(1)) > 150, run.stdout
