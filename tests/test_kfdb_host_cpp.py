"""Host bookkeeping of the keyframe database as a stand-alone C++ program (tests/cpp/
kfdb_host_check.cpp, its own main, no GPU and no library): the adapter's pointer <-> slot map
(mcs::KfSlots of host/mcs_multicol.hpp) and the capacity account the C-ABI keeps with the caller's
upper bounds (csrc/kfdb_host.hpp).  Built plain and with -fsanitize=address,undefined, run directly."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", *flags, os.path.join(ROOT, "tests", "cpp", "kfdb_host_check.cpp"),
                           "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "ok", r.stdout


def test_kfdb_host_check(tmp_path):
    _build_and_run(tmp_path, "kfdb_host_check", ["-O2"])


def test_kfdb_host_check_sanitized(tmp_path):
    _build_and_run(tmp_path, "kfdb_host_check_san",
                   ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
