"""The staging helper of the load entries (neural_amd/csrc/staging.h) without a device: tests/staging_main.cpp drives
its control flow against stub allocate / synchronise / free functions, built with the address and undefined-behaviour
sanitizers as a program of its own.  It checks that finish() and the destructor each free exactly once, that the
synchronise precedes the free in every order of failure, and that the first error is the one reported."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_staging_control_flow_under_sanitizers(tmp_path):
    exe = str(tmp_path / "staging_main")
    cc = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", os.path.join(HERE, "staging_main.cpp"), "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "staging ok" and r.stderr == ""
