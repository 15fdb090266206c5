"""
SiMPle: similarity matrix profile (Silva, Yeh, Batista & Keogh, ISMIR 2016).  Drop-in for
acoss/algorithms/simple_silva.py: same constructor and methods.  Feature preparation (mean
pooling, Hann smoothing, L2 column normalisation, simple_silva.py:34-43,56-66) runs ONCE
per track (the reference redoes it for every pair) -- on the device for the whole collection
(acx_simple_upload_raw_pool) when the tracks come from feature files, on the host in
load_features(i) for single-track access; OTI + matrix profile + median of every ordered pair
run in libacx's HIP kernel, in f64 like the reference.
"""
import numpy as np

from .. import _lib
from . import _align
from .algorithm_template import CoverAlgorithm, refused_in_session

__all__ = ["Simple"]


def _hann_sym(n):
    """scipy.signal.get_window('hann', n, fftbins=False)."""
    if n == 1:
        return np.ones(1)
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / (n - 1))


class Simple(CoverAlgorithm):
    """
    SSLEN: subsequence length; WIN / SKIP: window and hop of the dimensionality reduction.
    """
    n_chunks = 1
    _identify_symmetric = False      # identify(): benchmark() runs all_pairwise(symmetric=False), row q = the ordered pairs (q, c)

    def __init__(self, dataset_csv, datapath, chroma_type='hpcp', shortname='Covers80',
                 SSLEN=10, WIN=200, SKIP=100, device=None, nonfinite="raise"):
        self.SSLEN = SSLEN
        self.WIN = WIN
        self.SKIP = SKIP
        self.chroma_type = chroma_type
        self.all_feats = {}
        self._device = device
        self._nonfinite = nonfinite
        self._ctx = None
        self._pool_ready = False
        self._bind_collective_device(self._device)      # before the first collective of this object
        CoverAlgorithm.__init__(self, dataset_csv=dataset_csv, name="SiMPle", datapath=datapath,
                                shortname=shortname)

    # ------------------------------------------------------------------ features (host)
    def load_features(self, i, do_plot=False):
        if i not in self.all_feats:
            feats = CoverAlgorithm.load_features(self, i)
            feat_orig = np.asarray(feats[self.chroma_type]).T
            n = int(feat_orig.shape[1] / self.SKIP)
            pooled = np.zeros((feat_orig.shape[0], n))
            for k in range(n):
                pooled[:, k] = np.mean(feat_orig[:, k * self.SKIP:k * self.SKIP + self.WIN], axis=1)
            self.all_feats[i] = self.smooth(pooled)
        return self.all_feats[i]

    @refused_in_session
    def set_features(self, feats, labels=None):
        """Inject ready (12, n_i) f64 features for every track (synthetic benchmarks)."""
        assert len(feats) == self.N
        self.all_feats = {i: np.asarray(f, dtype=np.float64) for i, f in enumerate(feats)}
        if labels is not None:
            for i, l in enumerate(labels):
                self._register_label(i, l)
        self._pool_ready = False

    def smooth(self, feat, win_len_smooth=4):
        """Hann(win+2, symmetric) / sum along time ('same', zero fill), then unit L2 columns
        (librosa.util.normalize: columns with a norm below tiny stay unscaled)."""
        n = win_len_smooth + 2
        win = _hann_sym(n)
        win = win / np.sum(win)
        feat = np.asarray(feat, dtype=np.float64)
        out = np.empty_like(feat)
        lo = (n - 1) // 2
        for c in range(feat.shape[0]):
            out[c] = np.convolve(feat[c], win, mode="full")[lo:lo + feat.shape[1]]
        nrm = np.sqrt(np.sum(out ** 2, axis=0, keepdims=True))
        nrm[nrm < np.finfo(np.float64).tiny] = 1.0
        return out / nrm

    def oti(self, seq_a, seq_b):
        """(seq_b rolled to best match seq_a, ascending argsort of the 12 shift scores)."""
        pa, pb = np.sum(seq_a, 1), np.sum(seq_b, 1)
        v = np.array([np.dot(pa, np.roll(pb, s, axis=0)) for s in range(12)])
        order = np.argsort(v)
        return np.roll(seq_b, order[-1], axis=0), order

    # ------------------------------------------------------------------ device
    def _context(self):
        if self._ctx is None:
            import os
            dev = self._device if self._device is not None else int(os.environ.get("LOCAL_RANK", "0"))
            self._ctx = _lib.Context(dev, nonfinite=getattr(self, "_nonfinite", "raise"))
        if not self._pool_ready:
            if len(self.all_feats) == self.N:
                # features injected (set_features) or already prepared by load_features
                tracks = [np.ascontiguousarray(self.load_features(i).T, dtype=np.float64) for i in range(self.N)]
                offs = np.concatenate([[0], np.cumsum([t.shape[0] for t in tracks])]).astype(np.int64)
                self._ctx.upload_pool_f64(np.concatenate(tracks, axis=0), offs)
            else:
                # raw chroma of every track -> pooling, smoothing and normalisation on the device
                raw = [np.ascontiguousarray(CoverAlgorithm.load_features(self, i)[self.chroma_type], dtype=np.float32)
                       for i in range(self.N)]
                offs = np.concatenate([[0], np.cumsum([t.shape[0] for t in raw])]).astype(np.int64)
                self._ctx.simple_upload_raw_pool(np.concatenate(raw, axis=0), offs, self.WIN, self.SKIP, 4)
            self._pool_ready = True
        return self._ctx

    def simple_sim(self, seq_a, seq_b):
        """median_i min_j ||A[:, i:i+L] - B[:, j:j+L]||^2 of two (12, n) sequences (no OTI).  The two
        sequences become a two-track pool of a side context that lives as long as this object (the
        collection's pool in the main context stays where it is)."""
        import os
        if getattr(self, "_aux_ctx", None) is None:
            self._aux_ctx = _lib.Context(self._device if self._device is not None else int(os.environ.get("LOCAL_RANK", "0")),
                                         nonfinite=getattr(self, "_nonfinite", "raise"))
        ctx = self._aux_ctx
        a = np.ascontiguousarray(np.asarray(seq_a, dtype=np.float64).T)
        b = np.ascontiguousarray(np.asarray(seq_b, dtype=np.float64).T)
        ctx.upload_pool_f64(np.concatenate([a, b]), np.array([0, len(a), len(a) + len(b)], np.int64))
        return float(-ctx.simple_pairs(np.array([[0, 1]], np.int32), self.SSLEN, oti=False)[0])

    def _check_tracks(self, who, tracks):
        out = []
        for i, t in enumerate(tracks):
            t = np.asarray(t)
            if t.ndim != 2 or t.shape[0] != 12:
                raise ValueError("%s: track %d must be (12, n) features, got shape %s" % (who, i, t.shape))
            if t.dtype.kind != "f":
                raise ValueError("%s: track %d must be floating-point features, got dtype %s" % (who, i, t.dtype))
            out.append(np.ascontiguousarray(t.T, dtype=np.float64))
        return out

    def _append_tracks(self, ctx, tracks):
        offs = np.concatenate([[0], np.cumsum([t.shape[0] for t in tracks])]).astype(np.int64)
        ctx.pool_append_f64(np.concatenate(tracks, axis=0), offs)
        return None

    def _grid(self):
        return self._context(), _lib.ALGO_SIMPLE, _lib.SimpleParams(int(self.SSLEN), 1), ["main"]

    # ------------------------------------------------------------------ where the match lies
    # align() / profile() / align_matches(): acx_simple_alignment (include/acx.h).  Rows and columns are subsequence starts in
    # POOLED frames of the query / the reference; the spans are [first, last] inclusive pooled frames
    ALIGN_DTYPE = _lib.SIMPLE_ALIGNMENT_DTYPE

    def _no_match_rows(self, shape):
        """An empty slot of align_matches: -1 in every position, run_len 0, score and best_dist NaN."""
        out = _align.no_match_rows(shape, self.ALIGN_DTYPE)
        for f in ("best_q", "best_r"):
            out[f] = -1
        for f in ("score", "best_dist"):
            out[f] = np.nan
        return out

    def _align_kw(self, who, similarity_type):
        if similarity_type not in (None, "main"):
            raise ValueError("%s: unknown similarity type %r; similarity_type must be one of %s" % (who, similarity_type, list(self._identify_planes)))
        return {}

    def align(self, idxs):
        """WHICH part of the reference did the query match?  idxs: (K, 2) (query, reference) track indices over the uploaded
        collection, ORDERED pairs as similarity() scores them.  Returns a (K,) structured array: score (the f64 value
        similarity() computes for the pair, before Ds['main'] rounds it to f32), shift (the OTI shift applied to the
        reference), best_q / best_r / best_dist (the subsequence of the query that lies closest to the reference, its nearest
        neighbour there and their squared distance: the smallest value of the matrix profile, first row on ties), and the
        matched section: the longest run of consecutive query subsequences q0 .. q1 whose nearest neighbours r0 .. r1 are
        consecutive too (run_len of them; of several longest the first), with q_span = [q0, q1 + SSLEN - 1] and r_span =
        [r0, r1 + SSLEN - 1] in pooled frames.  A pair always has a match (run_len >= 1).  `Ds` is not written; not a
        collective."""
        pairs = _align.check_pairs("align", _align.check_indices("align", idxs), self._n_tracks())
        if len(pairs) == 0:
            return np.zeros(0, self.ALIGN_DTYPE)
        return self._context().simple_profile(pairs, self.SSLEN)

    def profile(self, idxs):
        """align() and the matrix profiles themselves: (al, mps, mpis).  al is exactly what align(idxs) returns; mps[k] is the
        (ma_k,) f64 profile of pair k -- for every subsequence of the query (ma_k = n_query - SSLEN + 1 of them) the squared
        distance to its nearest subsequence of the reference -- and mpis[k] the (ma_k,) int32 index, which subsequence that is
        (the first of equally near ones).  -median(mps[k]) is al['score'][k]."""
        pairs = _align.check_pairs("profile", _align.check_indices("profile", idxs), self._n_tracks())
        if len(pairs) == 0:
            return np.zeros(0, self.ALIGN_DTYPE), [], []
        al, off, mp, mpi = self._context().simple_profile(pairs, self.SSLEN, profiles=True)
        return al, [mp[off[k]:off[k + 1]] for k in range(len(pairs))], [mpi[off[k]:off[k + 1]] for k in range(len(pairs))]

    def align_matches(self, queries, indices):
        """align() for the hits of identify() / rerank(): queries (Q,) track indices, indices the (Q, k) int array either
        returned (-1: an empty slot).  Returns a (Q, k) structured array as align() does, row i slot s being the ORDERED pair
        (queries[i], indices[i, s]) -- the pair identify() scored.  An empty slot comes back as a no-match row: -1 in every
        position, run_len 0, score and best_dist NaN."""
        who = "align_matches"
        idx, rows, slots, pairs = _align.check_matches(who, _align.check_indices(who, queries), _align.check_indices(who, indices), self._n_tracks())
        out = self._no_match_rows(idx.shape)
        if len(pairs):
            out[rows, slots] = self._context().simple_profile(pairs, self.SSLEN)
        return out

    @refused_in_session
    def similarity(self, idxs):
        idxs = np.asarray(idxs).reshape(-1, 2)
        if len(idxs) == 0:
            return
        sim = self._context().simple_pairs(idxs.astype(np.int32), self.SSLEN)
        self.Ds['main'][idxs[:, 0], idxs[:, 1]] = sim
