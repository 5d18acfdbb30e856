"""The loopback rendezvous (cilqr_amd/csrc/loopback.hpp) on the host: the registry, the mailboxes, the matching and the
bounded waits behind cilqr_comm_create_loopback, with threads as ranks and memcpy as the copy.  No GPU involved: the header
has no HIP dependency, which building it with g++ alone also pins.  What the same rendezvous carries on a GPU is held in
tests/test_gpu_gather_ranks.py."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rendezvous_under_thread_sanitizer(tmp_path):
    """tests/cpp/loopback_test.cc, built with -fsanitize=thread and run as a child process: W in {2, 3, 8} with every
    root and several groups in a row on one communicator, both directions inside one group, a count (and a type) mismatch
    that fails on both sides while a third rank's operation of the same group completes, a missing peer that ends at a
    bound of 300 ms, and a registry that is empty after every create / destroy sequence."""
    exe = tmp_path / "loopback_test"
    # (the runtime linked statically: the program then does not care what else a machine loads into its processes)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=thread", "-static-libtsan", "-pthread",
                           "-I" + os.path.join(ROOT, "cilqr_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "loopback_test.cc"), "-o", str(exe)])
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "ThreadSanitizer" not in run.stderr, run.stderr
    m = re.fullmatch(r"(\d+) checks, 0 failures", run.stdout.strip())
    assert m and int(m.group(1)) > 1000, run.stdout
