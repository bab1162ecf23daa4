"""The host side of the frame scaling under AddressSanitizer and UBSan: tests/host_check/scale_host.cpp, a stand-alone program (its
own main, no GPU code, never loaded into Python) over xrslam_amd/csrc/host/pixel_format.hpp -- the plain-C++ crop and area mean of
the CPU reference build over the geometry list of tests/test_scale_gpu.py, and the staging of a cropped host frame into a pinned
slot, with source blocks that end at the crop's last needed byte."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_check", "scale_host.cpp")
OUT = os.path.join(ROOT, "tests", "host_check", "_build", "scale_host")
DEPS = [SRC, os.path.join(ROOT, "xrslam_amd", "csrc", "host", "pixel_format.hpp"), os.path.join(ROOT, "include", "xrslam_hip.h")]


def test_host_scaler_and_crop_staging_are_clean_under_the_sanitizers():
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(d) for d in DEPS):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", SRC, "-o", OUT])
    p = subprocess.run([OUT], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert p.stdout.strip().splitlines()[-1] == "ok"
