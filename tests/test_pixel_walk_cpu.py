"""CPU: the incremental pixel walk of the weight gradient (csrc/dj_walk.h: NP 3 of both kernel families, the fp32 MFMA
kernels of dj_igemm_fast.h and the split-bf16 kernels of dj_igemm_h16.h) gives, for every thread row and every K-step of
every K chunk, exactly the (in-bounds flag, byte offset) of the direct pixel decomposition.  tests/pixel_walk_check.cpp
walks the grid (maps 1x1 .. 19x19, strides 1 / 2, dilation 1 / 6, 'same' and 'valid' padding, K-steps of 16 and 32 -- 32
is also the fp32 kernels' step --, chunks that end mid-row and mid-image, batch 1 .. 3), and a second grid of geometries
that differ between the axes (kernels 1x3 / 3x1 / 2x3, strides (2,1) / (1,2), dilations (1,3) / (2,1), non-square maps of both
orientations): sH for sW in a carry of the walk passes the square grid and fails there.  It is built here as a stand-alone
program with the address and undefined-behaviour sanitizers and run directly."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pixel_walk_equals_direct_decomposition(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "pixel_walk_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "jpeg_detection_resnet_ssd_amd", "csrc"),
           os.path.join(ROOT, "tests", "pixel_walk_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"pixel walk: (\d+) launches, (\d+) offsets equal", r.stdout)
    assert m, r.stdout + r.stderr
    assert int(m.group(1)) >= 8000 and int(m.group(2)) >= 70000000
    m = re.search(r"(\d+) launches on geometries that differ between the axes", r.stdout)
    assert m and int(m.group(1)) >= 7000, r.stdout
