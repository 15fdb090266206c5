"""
Plain numpy FTM2D (acoss/algorithms/ftm2d.py), the checker of the HIP chain -- the role tests/_simple_ref.py plays for
SiMPle.  The beat sync restates librosa.util.sync(X, onsets, aggregate=np.median) with fix_frames(pad=True) (librosa is
not installed: self-pinned, like Serra09's sync): a negative onset raises, onsets are clipped to [0, T], 0 and T are
added, np.unique; segment k is [b_k, b_k+1) and its value the per-bin np.median in the input dtype.  The rest is the
reference's arithmetic (chrompwr, btchroma_to_fftmat, load_features :59-63, similarity :85-97) with np.fft.fft2, in f64
unless the caller passes f32.

`mutant=` switches one step to a plausible wrong version (tests/test_ftm2d_ref.py checks that each one moves the
shingle by far more than the GPU tolerances): "no_fftshift", "shift_one_axis", "mean_sync", "no_log", "no_chrompwr",
"win_minus_one" (the window loop stops one window early).
"""
import numpy as np


def sync_bounds(T, onsets):
    onsets = np.asarray(onsets).astype(np.int64).reshape(-1)
    if np.any(onsets < 0):
        raise ValueError("negative onset")
    b = np.concatenate([[0, T], np.clip(onsets, 0, T)])
    return np.unique(b)


def beat_sync(X, onsets, agg=np.median):
    """X (T, 12) as loaded -> (12, nbeats) in X's dtype."""
    X = np.asarray(X)
    b = sync_bounds(X.shape[0], onsets)
    out = np.empty((X.shape[1], len(b) - 1), X.dtype)
    for k in range(len(b) - 1):
        out[:, k] = agg(X[b[k]:b[k + 1]].T, axis=-1)
    return out


def chrompwr(X, P=.5):
    """ftm2d.py:100-117 (X: (12, nbeats))."""
    nchr, nbts = X.shape
    CMn = np.tile(np.sqrt(np.sum(X * X, axis=0)), (nchr, 1))
    CMn[CMn == 0] = 1
    CMp = np.power(X / CMn, P)
    CMpn = np.tile(np.sqrt(np.sum(CMp * CMp, axis=0)), (nchr, 1))
    CMpn[np.where(CMpn == 0)] = 1.
    return CMn * (CMp / CMpn)


def fftmat(btchroma, win=75, mutant=None):
    """btchroma_to_fftmat (ftm2d.py:120-139) with np.fft: (12 win, nwin), or None when nbeats < win."""
    nchrm, nbeats = btchroma.shape
    if nbeats < win:
        return None
    nwin = nbeats - win + 1 - (1 if mutant == "win_minus_one" else 0)
    out = np.zeros((nchrm * win, nwin))
    for i in range(nwin):
        F = np.abs(np.fft.fft2(btchroma[:, i:i + win]))
        if mutant == "no_fftshift":
            patch = F
        elif mutant == "shift_one_axis":
            patch = np.fft.fftshift(F, axes=1)
        else:
            patch = np.fft.fftshift(F)
        out[:, i] = patch.flatten()
    return out


def stages(X, onsets, pwr=1.96, win=75, C=5, dtype=np.float64, synced=None, mutant=None):
    """Every intermediate of FTM2D.load_features: synced (nbeats, 12) (time-major, in X's dtype), pwr (nbeats, 12),
    logwin (nwin, D), median (D,), shingle (D,).  synced= starts from given beat-synchronous values (the device's)."""
    if synced is None:
        agg = (lambda a, axis: np.mean(a, axis=axis)) if mutant == "mean_sync" else np.median
        S = beat_sync(np.asarray(X), onsets, agg=agg)       # in the chroma's own dtype (f32 as loaded)
    else:
        S = np.asarray(synced).T
    S = S.astype(dtype)
    chroma = S if mutant == "no_chrompwr" else chrompwr(S, dtype(pwr) if dtype == np.float32 else pwr)
    sh = fftmat(chroma, win, mutant=mutant).T
    Norm = np.sqrt(np.sum(sh ** 2, 1))
    Norm[Norm == 0] = 1
    logwin = sh / Norm[:, None] if mutant == "no_log" else np.log(C * sh / Norm[:, None] + 1)
    med = np.median(logwin, 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        shingle = med / np.sqrt(np.sum(med ** 2))
    return dict(synced=S.T, pwr=np.asarray(chroma).T, logwin=logwin, median=med, shingle=shingle)


def shingle(X, onsets, pwr=1.96, win=75, C=5, mutant=None):
    return stages(X, onsets, pwr, win, C, mutant=mutant)["shingle"]


def pair_scores(S, pairs):
    """exp(-sum((s_i - s_j)^2)) in f64 (ftm2d.py:93-96)."""
    S = np.asarray(S, dtype=np.float64)
    pairs = np.asarray(pairs).reshape(-1, 2)
    d = S[pairs[:, 0]] - S[pairs[:, 1]]
    with np.errstate(invalid="ignore"):
        return np.exp(-np.sum(d ** 2, axis=1))
