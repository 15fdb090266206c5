"""
FTM2D: 2D Fourier transform magnitudes of beat-synchronous chroma (Bertin-Mahieux & Ellis, 2012).  Drop-in for
acoss/algorithms/ftm2d.py: same constructor, name, cache prefix, load_features(i), similarity(idxs) writing
Ds['main'], and the `shingles` dict.  The reference's own module cannot run (it uses `os` and `deepdish` without
importing them); the chain it describes runs in libacx's HIP kernels:
  * the shingle of every track -- librosa.util.sync(chroma.T, onsets, aggregate=np.median) (self-pinned, librosa
    is absent), chrompwr, |fft2| of every WIN-beat window in fftshift order, window norm, log(C x + 1), median over
    the windows, L2 norm (ftm2d.py:38-64, 100-139) -- on the device for the whole collection, streamed from the
    feature files in batches of whole tracks (acx_ftm2d_pool_*);
  * exp(-|s_i - s_j|^2) of every pair (:85-97) in f64, stored into the float32 Ds['main'] -- a tile kernel over
    the N x N grid (all_pairwise), or a pair list (similarity(idxs)).
Deliberate differences:
  * no per-track "<prefix>_<i>.h5" shingle cache: the reference's code for it cannot run (`os`, `dd` undefined,
    ftm2d.py:44,47,82); shingles are kept in memory (`shingles`) and on the device;
  * no `do_plot` (load_features(i) accepts and ignores it).
"""
import os

import numpy as np

from .. import _lib
from .algorithm_template import CoverAlgorithm, refused_in_session

__all__ = ["FTM2D"]


class _RawTracks(object):
    """The raw features FTM2D needs, read from the feature files when indexed (a lazy sequence for
    Context.ftm2d_upload_raw_pool: one batch of tracks in host memory at a time)."""

    def __init__(self, algo):
        self.algo = algo

    def __len__(self):
        return self.algo.N

    def __getitem__(self, i):
        return self.algo._raw_track(CoverAlgorithm.load_features(self.algo, i))


class FTM2D(CoverAlgorithm):
    """
    Attributes
    ----------
    Same as CoverAlgorithm, plus
    shingles: {int: ndarray(WIN * 12)}   the shingle of every track computed so far
    chroma_type: string                  key of the chroma in the feature files
    """
    n_chunks = 1
    upload_batch = 256          # tracks per streamed upload batch

    def __init__(self, dataset_csv, datapath, chroma_type='hpcp', shortname='Covers80', PWR=1.96, WIN=75, C=5,
                 device=None, nonfinite="raise"):
        self.PWR = PWR
        self.WIN = WIN
        self.C = C
        self.chroma_type = chroma_type
        self.shingles = {}
        self._device = device
        self._nonfinite = nonfinite
        self._ctx = None
        self._aux_ctx = None
        self._pool_ready = False
        self._bind_collective_device(self._device)      # before the first collective of this object
        CoverAlgorithm.__init__(self, dataset_csv=dataset_csv, name="FTM2D", datapath=datapath, shortname=shortname)

    def get_cacheprefix(self):
        """Return a descriptive file prefix to use for caching features and distance matrices"""
        return "%s/%s_%s_%s" % (self.cachedir, self.name, self.shortname, self.chroma_type)

    def _raw_track(self, feats):
        """What a shingle is made of (ftm2d.py:53-57): the chroma (T, 12) and the beat onsets in frames."""
        return dict(chroma=np.asarray(feats[self.chroma_type], dtype=np.float32),
                    onsets=np.asarray(feats["madmom_features"]["onsets"]).astype(np.int64))

    def _new_context(self):
        dev = self._device if self._device is not None else int(os.environ.get("LOCAL_RANK", "0"))
        return _lib.Context(dev, nonfinite=self._nonfinite)

    # ------------------------------------------------------------------ features
    def load_features(self, i, do_plot=False):
        """The (12 WIN,) f64 shingle of track i, computed on the device (a side context: the collection's pool stays
        where it is); records the track's clique as a side effect."""
        if i in self.shingles:
            return self.shingles[i]
        feats = CoverAlgorithm.load_features(self, i)
        raw = self._raw_track(feats)
        if self._aux_ctx is None:
            self._aux_ctx = self._new_context()
        self.shingles[i] = self._aux_ctx.ftm2d_debug_track(raw["chroma"], raw["onsets"], self.PWR, self.WIN, self.C)["shingle"]
        return self.shingles[i]

    @refused_in_session
    def set_features(self, shingles, labels=None):
        """Inject ready (12 WIN,) f64 shingles for every track (synthetic benchmarks)."""
        assert len(shingles) == self.N
        self.shingles = {i: np.asarray(s, dtype=np.float64) for i, s in enumerate(shingles)}
        if labels is not None:
            for i, l in enumerate(labels):
                self._register_label(i, l)
        self._pool_ready = False

    # ------------------------------------------------------------------ device
    def _context(self):
        if self._ctx is None:
            self._ctx = self._new_context()
        if not self._pool_ready:
            if len(self.shingles) == self.N:
                # shingles injected (set_features) or already computed by load_features
                self._ctx.ftm2d_upload_shingles(np.stack([self.shingles[i] for i in range(self.N)]))
            else:
                # raw features of every track, streamed from the feature files -> shingles on the device
                self._ctx.ftm2d_upload_raw_pool(_RawTracks(self), self.PWR, self.WIN, self.C, batch=self.upload_batch)
                S = self._ctx.ftm2d_download_shingles()
                self.shingles = {i: S[i] for i in range(self.N)}
            self._pool_ready = True
        return self._ctx

    def _check_tracks(self, who, tracks):
        out = []
        for i, t in enumerate(tracks):
            t = np.asarray(t)
            if t.ndim != 1 or t.shape[0] != 12 * int(self.WIN):
                raise ValueError("%s: track %d must be a (%d,) shingle, got shape %s" % (who, i, 12 * int(self.WIN), t.shape))
            if t.dtype.kind != "f":
                raise ValueError("%s: track %d must be a floating-point shingle, got dtype %s" % (who, i, t.dtype))
            out.append(np.asarray(t, dtype=np.float64))
        return out

    def _append_tracks(self, ctx, tracks):
        ctx.ftm2d_append_shingles(np.stack(tracks))
        return None

    def _grid(self):
        return self._context(), _lib.ALGO_FTM2D, None, ["main"]

    @refused_in_session
    def similarity(self, idxs):
        idxs = np.asarray(idxs).reshape(-1, 2)
        if len(idxs) == 0:
            return
        self.Ds['main'][idxs[:, 0], idxs[:, 1]] = self._context().ftm2d_pairs(idxs.astype(np.int32))
