"""
ChenFusion: Qmax + Dmax late fusion (Chen, Li & Xiao 2018).  Drop-in for
acoss/algorithms/latefusion_chen.py: same constructor, load_features(i), similarity(idxs),
normalize_by_length(), do_late_fusion(), similarity types "qmax" / "dmax" (+ "Late").
The reference builds ONE essentia cross recurrence plot per pair and aligns it twice
(latefusion_chen.py:58-72); here libacx does the same for the whole `idxs` array in one call
(acx_chenfusion_pairs: band kernels once, the bitmap DP twice).
"""
import numpy as np

from .. import _lib
from .rqa_serra09 import Serra09
from .algorithm_template import CoverAlgorithm, refused_in_session
from .similarity_fusion import doSimilarityFusion

__all__ = ["ChenFusion"]


class ChenFusion(Serra09):
    """Serra09's constructor, attributes and keywords.

    Alignments (_align.AlignMixin, as Serra09's: units, spans and formula are those of its docstring): the class scores one plot
    twice, and similarity_type says whose alignment is wanted -- 'qmax' (the default: exactly Serra09's result, with Serra09's
    refusal while engine dmax is set) or 'dmax', the alignment behind the `dmax` score of the same cross recurrence plot
    (acx_chenfusion_align*, plane 1; it does not read the engine's dmax switch, as acx_chenfusion_pairs does not).  'Late' is fused
    from whole score matrices and has no alignment of its own: ValueError.  Dmax adds R[i-1][j] to the (i-2, j-1) predecessor and
    R[i][j-1] to the (i-1, j-2) one, so its start cell's value need not be 1, and the start can be a gap cell whose neighbour
    (q0 - 1, r0) or (q0, r0 - 1) is the recurrence at which the alignment really begins: q_span / r_span can begin one embedded
    frame late.  The sections (align_sections, align_match_sections) are the Qmax alignment's: 'qmax' is the default and the only
    type, 'dmax' a ValueError naming the method."""

    def __init__(self, dataset_csv, datapath, chroma_type='hpcp', shortname='benchmark',
                 oti=True, kappa=0.095, tau=1, m=9, downsample_fac=40, device=None, engine=None, nonfinite="raise"):
        self.oti = oti
        self.kappa = kappa
        self.tau = tau
        self.m = m
        self.chroma_type = chroma_type
        self.downsample_fac = downsample_fac
        self.all_feats = {}
        self._device = device
        self._nonfinite = nonfinite
        self._engine = dict(engine or {})
        self._ctx = None
        self._pool_ready = False
        self._pooled_len = None
        self._bind_collective_device(self._device)      # before the first collective of this object
        CoverAlgorithm.__init__(self, dataset_csv=dataset_csv, name="LateFusionChen", datapath=datapath,
                                shortname=shortname, similarity_types=["qmax", "dmax"])

    _identify_planes = ("qmax", "dmax")
    _identify_fused = ("Late",)
    # do_late_fusion fuses self.Ds in insertion order -- qmax, dmax -- as distances sqrt(T_c) / s (normalize_by_length)
    _fused_planes = {"Late": ("qmax", "dmax")}
    _fused_transform = _lib.FUSED_SQRTLEN

    def _identify_norm(self):
        """identify() / query_rows(): -(sqrt(T_c) / s), normalize_by_length with the sign flip of do_late_fusion."""
        return 2, np.sqrt(self._pooled_lengths().astype(np.float64))

    def _grid(self):
        return self._context(), _lib.ALGO_CHENFUSION, self._params(), ["qmax", "dmax"]

    @refused_in_session
    def similarity(self, idxs):
        idxs = np.asarray(idxs).reshape(-1, 2)
        if len(idxs) == 0:
            return
        sc = self._context().chenfusion_pairs(idxs.astype(np.int32), self._params())
        self.Ds["qmax"][idxs[:, 0], idxs[:, 1]] = sc[:, 0]
        self.Ds["dmax"][idxs[:, 0], idxs[:, 1]] = sc[:, 1]

    # ------------------------------------------------------------------ where the alignment lies: the hooks
    def _align_call(self, pairs, want_paths, plane):
        if plane == 0:                                  # (Serra09's align*() itself)
            return Serra09._align_call(self, pairs, want_paths, plane)
        if not want_paths:
            return self._context().chenfusion_align(pairs, self._params(), plane), None, None
        return self._context().chenfusion_align_paths(pairs, self._params(), plane)

    def _sections_plane(self, who, similarity_type):
        """The sections are the Qmax alignment's: 'dmax' and 'Late' have none, ValueError naming the method."""
        plane = self._align_plane(who, similarity_type)
        if plane != 0:
            raise ValueError("%s: the sections are those of the Qmax alignment; similarity_type must be 'qmax', got '%s'" % (who, similarity_type))
        return plane

    @refused_in_session
    def rerank_tracks_fused(self, tracks, shortlists, k=10, similarity_types=None, K=20, niters=20, raw=False):
        """CoverAlgorithm.rerank_tracks_fused; tracks and raw as in identify_tracks."""
        return self._rerank_tracks_fused(tracks, shortlists, k, similarity_types, K, niters, raw=raw)

    @refused_in_session
    def normalize_by_length(self):
        """D[i, j] = sqrt(T_j) / D[i, j] (latefusion_chen.py:75-85): a DISTANCE, smaller =
        closer; unfilled cells (the diagonal) become +inf exactly as in the reference."""
        if not self.owns_result():
            return
        norm = np.sqrt(self._pooled_lengths().astype(np.float64))
        for key in self.Ds.keys():
            D = self.Ds[key]
            with np.errstate(divide="ignore"):
                for j0 in range(0, self.N, 2048):
                    j1 = min(self.N, j0 + 2048)
                    D[:, j0:j1] = (norm[None, j0:j1] / D[:, j0:j1]).astype(np.float32)

    @refused_in_session
    def do_late_fusion(self):
        """SNF of the two distance matrices (latefusion_chen.py:87-91): Ds["Late"] = fused
        similarity; the two inputs are negated so that larger = closer everywhere.  Runs on the GPU
        (acx_snf_fuse_dists) of the rank that owns the matrices; the other ranks return at once (their
        matrices are empty: 20 N x N sweeps over inf / NaN for nothing)."""
        if not self.owns_result():
            self.Ds["Late"] = np.zeros((0, 0), np.float64)     # same keys on every rank (getEvalStatistics is collective)
            return
        if self._ctx is None:
            import os
            self._ctx = _lib.Context(self._device if self._device is not None else int(os.environ.get("LOCAL_RANK", "0")), nonfinite=getattr(self, "_nonfinite", "raise"))
        DLate = doSimilarityFusion([self.Ds[s] for s in self.Ds], K=20, niters=20, reg_diag=1, ctx=self._ctx,
                                   want_ws=False)[1]
        for key in self.Ds:
            self.Ds[key] *= -1
        self.Ds["Late"] = DLate
