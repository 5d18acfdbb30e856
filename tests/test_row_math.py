"""The arithmetic host statements and kernels share (include/cilqr/row_math.hpp), against its plain forms written out a second
time in tests/cpp/row_math_test.cc.  No GPU and no library involved."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shared_row_arithmetic_against_its_plain_forms_under_address_sanitizer(tmp_path):
    """Built with g++ alone and -fsanitize=address,undefined and run as a child process: normalize_angle against fmod by bits
    at the edges of its short paths, slerp at and around 1e-10 and across +-pi, the bracket against std::lower_bound (and, on
    unsorted and NaN keys, the halving written out), hypot_ref against sqrtl, the pair step and its instances on two-row
    trajectories of every layout and key."""
    exe = tmp_path / "row_math_test"
    # (the runtimes linked statically: the program then does not care what else a machine loads into its processes)
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "row_math_test.cc"), "-o", str(exe)])
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    m = re.fullmatch(r"(\d+) checks, 0 failures", run.stdout.strip())
    assert m and int(m.group(1)) > 40000, run.stdout
