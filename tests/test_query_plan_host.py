"""
Host test of acoss_amd/csrc/query_plan.hpp (no GPU, no extension): tests/query_plan_check.cpp -- block layouts, the pairs
and destinations of dense and list bands, the FTM2D band tiles, the rows per band -- built with the host compiler under
the address and undefined-behaviour sanitizers and run as a program of its own.
"""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def test_query_plan_check_under_sanitizers(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler found (CXX, g++, c++, clang++)"
    exe = os.path.join(str(tmp_path), "query_plan_check")
    # the sanitizer runtimes linked into the program where the compiler has them as archives: it then runs whatever else
    # the process loads first
    for static in (["-static-libasan", "-static-libubsan"], []):
        build = subprocess.run([cxx] + FLAGS + static + ["-o", exe, os.path.join(ROOT, "tests", "query_plan_check.cpp")],
                               capture_output=True, text=True, timeout=300)
        if build.returncode == 0:
            break
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
