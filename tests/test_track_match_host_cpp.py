"""The C++ side of the tracking matchers' device form: mcs::SearchByProjection(F, MPs, th) and
mcs::SearchByProjection(Current, Last, th) of host/mcs_multicol.hpp compile against the C-ABI
and link libmcs_amd.so (tests/cpp/track_match_demo.cpp), the ABI structs have the size of their
ctypes mirrors, the argument checks answer before any device is opened, and the same program
built with -fsanitize=address,undefined (host code only: the argument checks' callers and the
adapter's packing) runs clean.  No GPU is needed; without one a good call answers
MCS_ERR_NO_DEVICE (there is no CPU fallback)."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["mcs_track_workspace_create", "mcs_track_workspace_destroy", "mcs_frame_grid_build_device",
           "mcs_track_unpack_keys_device", "mcs_track_queries_mappoints_device",
           "mcs_track_queries_lastframe_device", "mcs_track_search_device", "mcs_track_select_device",
           "mcs_track_search", "mcs_track_queries_mappoints", "mcs_track_queries_lastframe"]


def build_demo(tmp_path, extra=()):
    lib = os.path.join(ROOT, "multicol-slam-annotation_amd", "lib")
    exe = str(tmp_path / ("track_match_demo" + ("_san" if extra else "")))
    subprocess.check_call(["g++", "-O1" if extra else "-O2", "-g", "-std=c++17", "-Wall", "-Werror", *extra,
                           os.path.join(ROOT, "tests", "cpp", "track_match_demo.cpp"),
                           "-I", os.path.join(ROOT, "include"), "-L", lib, "-lmcs_amd",
                           "-Wl,-rpath," + lib, "-o", exe])
    return exe


def _check_abi_output(out, have_device):
    import mcs_amd
    from mcs_amd import track_match as tm
    from mcs_amd import window as mw
    sizes = [int(x) for x in re.search(r"mcs_track_frame (\d+) mcs_track_queries (\d+) mcs_window_frame (\d+)",
                                       out).groups()]
    assert sizes == [ctypes.sizeof(tm.TrackFrame), ctypes.sizeof(tm.TrackQueries), ctypes.sizeof(mw.WindowFrame)]
    codes = dict(re.findall(r"(\w+) (-?\d+)", out.splitlines()[1]))
    assert int(codes.pop("rule2")) == mcs_amd.MCS_ERR_UNSUPPORTED
    assert sorted(codes) == ["bytes", "cams", "masks", "nomatch", "queries", "rule4", "src", "ws"]
    assert all(int(v) == mcs_amd.MCS_ERR_ARG for v in codes.values()), codes
    good = int(re.search(r"good (-?\d+)", out).group(1))
    if not have_device:
        assert good == mcs_amd.MCS_ERR_NO_DEVICE
        assert "adapter threw: mcs_track_queries_mappoints" in out and "(%d)" % mcs_amd.MCS_ERR_NO_DEVICE in out
    else:       # one keypoint under the window, descriptor distance 0
        assert good == 0 and "good 0 match 0 n 1" in out and "adapter n 1 map_point 41" in out


def test_track_adapters_compile_and_abi_agrees(built, tmp_path):
    import mcs_amd
    for s in SYMBOLS:
        assert s in mcs_amd.SIGNATURES and hasattr(mcs_amd.lib(), s), s
    out = subprocess.check_output([build_demo(tmp_path), "abi"], timeout=120).decode()
    _check_abi_output(out, mcs_amd.device_count() > 0)


def test_track_adapters_host_code_under_sanitizers(built, tmp_path):
    exe = build_demo(tmp_path, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    # host code only: no device is visible to this program, so it stops at MCS_ERR_NO_DEVICE
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    p = subprocess.run([exe, "abi"], timeout=120, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert "ERROR: AddressSanitizer" not in p.stderr.decode() and "runtime error" not in p.stderr.decode()
    _check_abi_output(p.stdout.decode(), False)


def test_atan_cr_against_libm(tmp_path):
    """csrc/atan_cr.hpp (rule 1's WorldToImg angle) on the host: the libm's atan is good to under
    one ulp, so a correctly rounded atan never differs from it by more than one, and differs
    only where the libm misrounds: well under one argument in a thousand (measured: 2.5 in ten
    thousand).  Zeros, +-1 and the ends of the range agree."""
    exe = str(tmp_path / "atan_cr_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror",
                           os.path.join(ROOT, "tests", "cpp", "atan_cr_check.cpp"), "-o", exe])
    out = subprocess.check_output([exe], timeout=120).decode()
    n, differ, max_ulp, special = [int(x) for x in re.search(r"n (\d+) differ (\d+) max_ulp (\d+) special (\d+)",
                                                             out).groups()]
    assert max_ulp <= 1 and differ * 1000 < n and special == 0, out
