"""CPU-only proof of the counted waits of the register-tile k-loops (matinvent_amd/csrc/loop_waits.h): scripts/loop_waits_host_check.cpp
replays each loop's issue order through an in-order queue and checks every wait point of every loop length the kernels run."""
import os
import shutil
import subprocess

from tests.header_util import ROOT


def test_counted_waits_suffice_and_are_tight_at_every_wait_point(tmp_path):
    """edge_gemm1b at 2, 4, 6, 8 and 24 k-tiles, edge_gemm2b at 16, gemm_rt at 2, 4, 6, 16 and 32 (and every even length up to 64): under
    the count the header returns the awaited operation has retired, under count + 1 it need not have; the canonical iteration a kernel
    runs decides its requests as the true iteration does."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "loop_waits_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", os.path.join(ROOT, "scripts", "loop_waits_host_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "75 cases, 6696 wait points, 0 violations" in r.stdout
    for line in ("edge_gemm1b KT=2:", "edge_gemm1b KT=4:", "edge_gemm1b KT=6:", "edge_gemm1b KT=8:", "edge_gemm1b KT=24:", "edge_gemm2b KT=16:",
                 "gemm_rt KT=2:", "gemm_rt KT=4:", "gemm_rt KT=6:", "gemm_rt KT=16:", "gemm_rt KT=32:"):
        assert line in r.stdout, line
