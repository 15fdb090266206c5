#!/usr/bin/env python3
"""
Golden vectors of the full cross-diffusion early fusion.  RUNS ONLY IN THE AUTHORING CONTAINER (needs the reference tree);
its output (tests/golden/crossfusion.npz) is committed data -- seeded synthetic inputs and the reference's own outputs on them.

acoss/algorithms/utils/similarity_fusion.py loads with numpy and scipy alone.  Per shape (M, N): two smooth random-walk
tracks, the second carrying a copy of a stretch of the first, in three feature spaces; their f32 self- and cross-distance
matrices (Euclidean, Euclidean, cosine: the three features of EarlyFusion) are the inputs.  Recorded: the reference's
getWCSMSSM per feature (W), its doSimilarityFusionWs (D), X = D[0:M, M:] + D[M:, 0:M]^T, the plot B (the round(kappa N) largest
of every row of X = csm_to_binary(exp(-X), kappa)) and the oracle's Smith-Waterman score on B.  The maker asserts that every
row's gap at the cut of X is at least 1e-6: the plot does not hang on the last bits of D.

    python tests/golden/make_crossfusion_goldens.py
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True
import make_goldens  # noqa: E402
import oracle  # noqa: E402

SHAPES = [(12, 30), (40, 33), (64, 65)]
K, NITERS, REG_DIAG, KAPPA = 10, 5, 1.0, 0.1
WIDTHS = (20, 30, 24)
MIN_GAP = 1e-6


def load_reference():
    path = os.path.join(make_goldens.REF, "acoss", "algorithms", "utils", "similarity_fusion.py")
    spec = importlib.util.spec_from_file_location("ref_similarity_fusion", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def walk(rng, n, width):
    x = np.cumsum(rng.standard_normal((n, width)) * 0.3, axis=0) + rng.standard_normal(width)
    return x


def make_pair(rng, M, N, width, positive):
    A = walk(rng, M, width)
    B = walk(rng, N, width)
    L = min(M, N) * 2 // 3
    a0, b0 = int(rng.integers(0, M - L + 1)), int(rng.integers(0, N - L + 1))
    B[b0:b0 + L] = A[a0:a0 + L] + rng.standard_normal((L, width)) * 0.05          # the planted copy
    if positive:                                                                   # chroma-like: non-negative
        A, B = np.abs(A), np.abs(B)
    return A.astype(np.float32), B.astype(np.float32)


def main():
    sf = load_reference()
    out = dict(K=np.int32(K), niters=np.int32(NITERS), reg_diag=np.float64(REG_DIAG), kappa=np.float64(KAPPA),
               shapes=np.array(SHAPES, np.int32))
    for M, N in SHAPES:
        rng = np.random.default_rng(1000 * M + N)
        SA, SB, C = [], [], []
        for f, width in enumerate(WIDTHS):
            A, B = make_pair(rng, M, N, width, positive=f == 2)
            dist = oracle.get_csm_cosine if f == 2 else oracle.get_csm
            SA.append(dist(A, A).astype(np.float32)); SB.append(dist(B, B).astype(np.float32)); C.append(dist(A, B).astype(np.float32))
        SA, SB, C = np.stack(SA), np.stack(SB), np.stack(C)
        Ws = [sf.getWCSMSSM(SA[f].astype(np.float64), SB[f].astype(np.float64), C[f].astype(np.float64), K) for f in range(3)]
        D = sf.doSimilarityFusionWs([np.array(W) for W in Ws], K, NITERS, REG_DIAG)
        X = D[:M, M:] + D[M:, :M].T
        k = oracle.binary_k(KAPPA, N)
        srt = -np.sort(-X, 1)
        gap = srt[:, k - 1] - srt[:, k]
        assert gap.min() >= MIN_GAP, (M, N, gap.min())
        B = np.zeros((M, N), np.uint8)
        B[np.arange(M)[:, None], np.argsort(-X, 1, kind="stable")[:, :k]] = 1
        assert np.array_equal(B, oracle.csm_to_binary(np.exp(-X), KAPPA)), (M, N)
        score = oracle.sw_constrained(B)
        print("(%d, %d): k = %d, smallest gap at the cut %.3g, score %g" % (M, N, k, gap.min(), score))
        tag = "%dx%d_" % (M, N)
        out.update({tag + "SA": SA, tag + "SB": SB, tag + "C": C, tag + "W": np.stack(Ws), tag + "D": D, tag + "X": X, tag + "B": B,
                    tag + "score": np.float64(score)})
    path = os.path.join(HERE, "crossfusion.npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes" % (path, os.path.getsize(path)))
    assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
    main()
