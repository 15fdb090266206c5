#!/usr/bin/env python3
"""
FTM2D golden vectors.  RUNS ONLY IN THE AUTHORING CONTAINER (needs the reference tree); its output
(tests/golden/ftm2d.npz) is committed data -- seeded synthetic inputs and the reference's own outputs on them.

acoss.algorithms.ftm2d cannot run as shipped (it uses `os` and `deepdish` without importing them, SURVEY bug 8): the
module is imported with the stubs of make_goldens.py, `os` and the deepdish stub injected into its namespace,
scipy.fftpack imported explicitly (the module only does `import scipy`), and a librosa.util.sync stub with librosa's
semantics for aggregate=np.median, pad=True (fix_frames: negative -> error, clip to [0, T], 0 and T added, np.unique;
per-bin np.median over [b_k, b_k+1) in the input dtype).  Recorded per seeded track, once with the chroma as f32 (the
reference then runs complex64 FFTs) and once as f64: chrompwr of the synced chroma, btchroma_to_fftmat (a short
track), FTM2D.load_features and FTM2D.similarity over every pair of the group.

    python tests/golden/make_ftm2d_goldens.py
"""
import importlib
import os
import sys
import types

import numpy as np
import scipy.fftpack  # noqa: F401  (ftm2d.py calls scipy.fftpack.fft2 after a bare `import scipy`)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True
import make_goldens  # noqa: E402


def sync(data, idx, aggregate=np.median, pad=True, axis=-1):
    assert pad and axis == -1
    T = data.shape[-1]
    idx = np.asarray(idx)
    if np.any(idx < 0):
        raise ValueError("negative frame index")
    b = np.unique(np.concatenate([[0, T], np.clip(idx, 0, T)]).astype(int))
    out = np.empty(data.shape[:-1] + (len(b) - 1,), data.dtype)
    for k in range(len(b) - 1):
        out[..., k] = aggregate(data[..., b[k]:b[k + 1]], axis=-1)
    return out


# (seed, n_tracks, beats range, PWR, WIN, C): the defaults and a small window with other constants
GROUPS = [(11, 3, (80, 110), 1.96, 75, 5), (12, 3, (20, 40), 0.5, 16, 1)]


def make_track(rng, nb_range):
    nb = int(rng.integers(nb_range[0], nb_range[1] + 1))
    lens = rng.integers(3, 12, nb)
    intro = int(rng.integers(0, 60))
    T = intro + int(lens.sum()) + int(rng.integers(0, 20))
    X = (rng.random((T, 12)) ** 3).astype(np.float32)
    onsets = intro + np.concatenate([[0], np.cumsum(lens)[:-1]])
    # a duplicate, an onset beyond T and one at 0 (fix_frames' cases)
    onsets = np.concatenate([onsets, [onsets[5], T + 7, 0]]).astype(np.int64)
    return X, rng.permutation(onsets)


def main():
    dd = make_goldens.install_stubs()
    sys.modules["librosa.util"].sync = sync
    at = importlib.import_module("acoss.algorithms.algorithm_template")
    ftm = importlib.import_module("acoss.algorithms.ftm2d")
    ftm.os = os
    ftm.dd = dd
    at.CoverAlgorithm.load_features = lambda self, i: self._feats[i]
    out = {}
    for g, (seed, n, nbr, P, W, C) in enumerate(GROUPS):
        rng = np.random.default_rng(seed)
        tracks = [make_track(rng, nbr) for _ in range(n)]
        out["g%d_params" % g] = np.array([P, W, C], np.float64)
        for i, (X, on) in enumerate(tracks):
            out["g%d_X%d" % (g, i)], out["g%d_on%d" % (g, i)] = X, on
        for tag, dt in (("f32", np.float32), ("f64", np.float64)):
            a = object.__new__(ftm.FTM2D)
            a.PWR, a.WIN, a.C, a.chroma_type, a.shingles = P, W, C, "hpcp", {}
            a.cachedir, a.name, a.shortname = "/nonexistent", "FTM2D", "golden%d%s" % (g, tag)
            a._feats = [{"hpcp": X.astype(dt), "madmom_features": {"onsets": on}} for X, on in tracks]
            a.Ds = {"main": np.zeros((n, n), np.float32)}
            S = np.stack([a.load_features(i) for i in range(n)])
            out["g%d_shingle_%s" % (g, tag)] = S
            a.similarity(np.array([(i, j) for i in range(n) for j in range(n)]))
            out["g%d_sim_%s" % (g, tag)] = a.Ds["main"]
            hp = sync(tracks[0][0].astype(dt).T, tracks[0][1], aggregate=np.median)
            out["g%d_synced_%s" % (g, tag)] = hp
            out["g%d_chrompwr_%s" % (g, tag)] = ftm.chrompwr(hp, P)
            if g == 0:
                # btchroma_to_fftmat of a short beat matrix (a few windows)
                out["g%d_fftmat_%s" % (g, tag)] = ftm.btchroma_to_fftmat(ftm.chrompwr(hp, P)[:, :W + 3], W)
    np.savez_compressed(os.path.join(HERE, "ftm2d.npz"), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
