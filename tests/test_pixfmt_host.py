"""The host side of the camera pixel formats under AddressSanitizer and UBSan: tests/host_check/pixfmt_host.cpp, a stand-alone
program (its own main, no GPU code, never loaded into Python) over xrslam_amd/csrc/host/pixel_format.hpp -- the reduction of the CPU
reference build and the row packing of the pinned upload slots, with source blocks of exactly the bytes a frame has."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_check", "pixfmt_host.cpp")
OUT = os.path.join(ROOT, "tests", "host_check", "_build", "pixfmt_host")
DEPS = [SRC, os.path.join(ROOT, "xrslam_amd", "csrc", "host", "pixel_format.hpp"), os.path.join(ROOT, "include", "xrslam_hip.h")]


def test_host_reduction_and_row_staging_are_clean_under_the_sanitizers():
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(d) for d in DEPS):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", SRC, "-o", OUT])
    p = subprocess.run([OUT], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert p.stdout.strip().splitlines()[-1] == "ok"
