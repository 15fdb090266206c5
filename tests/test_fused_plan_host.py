"""
Host test of acoss_amd/csrc/fused_plan.hpp (no GPU, no extension): tests/fused_plan_check.cpp -- the neighbourhood of a
query, its pairs and their slab slots, the problem descriptors, the chunks under a limit, the block layout -- built with
the host compiler under the address and undefined-behaviour sanitizers and run as a program of its own; what it prints is
compared with a few lines of numpy.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
PROB_BYTES = 40           # sizeof(FusedProb): two int32, four int64


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler found (CXX, g++, c++, clang++)"
    path = os.path.join(str(tmp_path_factory.mktemp("fused_plan")), "fused_plan_check")
    for static in (["-static-libasan", "-static-libubsan"], []):
        build = subprocess.run([cxx] + FLAGS + static + ["-o", path, os.path.join(ROOT, "tests", "fused_plan_check.cpp")],
                               capture_output=True, text=True, timeout=300)
        if build.returncode == 0:
            break
    assert build.returncode == 0, build.stdout + build.stderr
    return path


def _problem_bytes(n, W, M, K, nt, k):
    return n * (n - 1) // 2 * W * 4 + 8 * ((3 * M + 2) * n * n + n) + 12 * M * n * K + 4 * n + PROB_BYTES + nt * (8 * k + 1)


def _run(exe, tmp_path, queries, lists, W, M, K, nt, k, half):
    Q, L = lists.shape
    case = os.path.join(str(tmp_path), "case.txt")
    with open(case, "w") as f:
        f.write("%d %d %d %d %d %d %d %d\n" % (Q, L, W, M, K, nt, k, half))
        f.write(" ".join(str(int(v)) for v in queries) + "\n")
        f.write(" ".join(str(int(v)) for v in lists.reshape(-1)) + "\n")
    run = subprocess.run([exe, case], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    return [line.split() for line in run.stdout.splitlines()]


def _lists(rng, n_tracks, Q, L, lo):
    queries = rng.integers(0, n_tracks, Q)
    lists = np.full((Q, L), -1, np.int64)
    for i in range(Q):
        m = int(rng.integers(lo, L + 1))
        lists[i, rng.choice(L, m, replace=False)] = rng.choice(n_tracks, m, replace=False)     # (may hold the query itself)
    return queries, lists


@pytest.mark.parametrize("seed,W,M,K,nt,k,half_problems", [(0, 2, 2, 20, 1, 10, 1000.0), (1, 4, 4, 20, 2, 7, 2.5), (2, 4, 3, 3, 1, 40, 1.0),
                                                            (3, 2, 2, 5, 1, 3, 4.2)])
def test_plan_matches_numpy(exe, tmp_path, seed, W, M, K, nt, k, half_problems):
    rng = np.random.default_rng(seed)
    Q, L = 9, 30
    queries, lists = _lists(rng, 60, Q, L, K + 1)
    Ts = [np.unique(np.concatenate([[q], row[row >= 0]])) for q, row in zip(queries, lists)]       # sorted, the query once
    ns = np.array([len(T) for T in Ts])
    bytes_ = np.array([_problem_bytes(int(n), W, M, K, nt, k) for n in ns])
    half = int(half_problems * bytes_.max())
    out = _run(exe, tmp_path, queries, lists, W, M, K, nt, k, half)
    assert out[0] == ["bytes"] + [str(b) for b in bytes_]
    assert out[1] == ["unfit", "-1"]
    # chunks: consecutive queries, greedily, while the sum of their bytes stays within half
    ends, acc = [], 0
    for i in range(Q):
        if acc and acc + bytes_[i] > half:
            ends.append(i)
            acc = 0
        acc += bytes_[i]
    ends.append(Q)
    assert out[2] == ["ends"] + [str(e) for e in ends]
    if half_problems < 100:
        assert len(ends) > 1, "the case is meant to take several chunks"
    at, first = 3, 0
    for ci, end in enumerate(ends):
        mat = lst = pr = tr = 0
        sel = range(first, end)
        assert out[at] == ["chunk", str(ci), str(len(sel)), str(ns[first:end].max()),
                           str(sum((3 * M + 2) * int(ns[i]) ** 2 + int(ns[i]) for i in sel)), str(sum(M * int(ns[i]) * K for i in sel)),
                           str(sum(int(ns[i]) * (int(ns[i]) - 1) // 2 for i in sel))]
        at += 1
        cells = []
        for i in sel:
            n, T = int(ns[i]), Ts[i]
            assert out[at] == ["prob", str(n), str(int(np.searchsorted(T, queries[i]))), str(mat), str(lst), str(pr), str(tr)]
            assert out[at + 1] == ["T"] + [str(t) for t in T]
            at += 2
            a, b = np.triu_indices(n, 1)                              # the upper triangle, row by row
            cells += [(int(T[y]), int(T[x]), (pr + j) * W) for j, (x, y) in enumerate(zip(a, b))]
            mat += (3 * M + 2) * n * n + n
            lst += M * n * K
            pr += n * (n - 1) // 2
            tr += n
        cells.sort()                                                   # by the second track, then the first, then the slot
        assert out[at] == ["pairs"] + [str(v) for second, first_, slot in cells for v in (first_, second, slot)]
        assert out[at + 1][0] == "layout"
        at += 2
        first = end
    assert at == len(out)


def test_one_neighbourhood_that_does_not_fit(exe, tmp_path):
    rng = np.random.default_rng(5)
    queries, lists = _lists(rng, 80, 4, 40, 25)
    lists[2] = np.setdiff1d(np.arange(80), [queries[2]])[:40]          # the longest neighbourhood: 41 tracks
    ns = [len(np.unique(np.concatenate([[q], row[row >= 0]]))) for q, row in zip(queries, lists)]
    assert ns[2] == 41 and max(ns[:2]) < 41
    half = _problem_bytes(41, 2, 2, 20, 1, 10) - 1
    out = _run(exe, tmp_path, queries, lists, 2, 2, 20, 1, 10, half)
    assert out[1] == ["unfit", "2"]
    out = _run(exe, tmp_path, queries, lists, 2, 2, 20, 1, 10, half + 1)
    assert out[1] == ["unfit", "-1"]


def test_no_queries(exe, tmp_path):
    out = _run(exe, tmp_path, np.zeros(0, np.int64), np.zeros((0, 3), np.int64), 2, 2, 20, 1, 10, 1 << 20)
    assert out[:3] == [["bytes"], ["unfit", "-1"], ["ends"]] and len(out) == 3
