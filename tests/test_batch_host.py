"""The host half of xpic_amd/csrc/batch.h (transposition, sample sizes, the compaction policy, the frozen sample rows of an
open trace) through tools/batch_host.cpp, a stand-alone program with its own main: built here with the plain host
compiler and run.  The program's header gives the command that builds it with the sanitizers."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_batch_host_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "the build needs a host C++ compiler (Makefile: g++)"
    exe = str(tmp_path / "batch_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "xpic_amd", "csrc"),
                    os.path.join(ROOT, "tools", "batch_host.cpp"), "-o", exe], check=True, timeout=120)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "batch.h host staging: ok" in out.stdout, out.stdout + out.stderr
