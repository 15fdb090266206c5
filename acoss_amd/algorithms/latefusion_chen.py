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
from . import _align
from .rqa_serra09 import Serra09
from .algorithm_template import CoverAlgorithm, refused_in_session
from .similarity_fusion import doSimilarityFusion

__all__ = ["ChenFusion"]


class ChenFusion(Serra09):
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

    # ------------------------------------------------------------------ where the alignment lies
    # The class scores one plot twice; similarity_type says whose alignment is wanted.  "qmax" (the default) is Serra09's align*()
    # itself; "dmax" is the Dmax alignment of the same plot (acx_chenfusion_align*, plane 1).  The Dmax start need not hold Q = 1 and
    # can be a gap cell beside the recurrence at which the alignment really begins: a span can begin one frame late.
    def _align_plane(self, who, similarity_type):
        """similarity_type -> plane of acx_chenfusion_align; raises for 'Late' and anything else, before any library call."""
        if similarity_type in self._identify_fused:
            raise ValueError("%s: '%s' is fused from whole score matrices and has no alignment of its own; similarity_type must be one of %s"
                             % (who, similarity_type, list(self._identify_planes)))
        if similarity_type not in self._identify_planes:
            raise ValueError("%s: unknown similarity type %r; similarity_type must be one of %s" % (who, similarity_type, list(self._identify_planes)))
        return self._identify_planes.index(similarity_type)

    def _check_align(self, who, idxs, plane=0):
        # (the Dmax alignment does not read the engine's dmax switch, as acx_chenfusion_pairs does not)
        return Serra09._check_align(self, who, idxs) if plane == 0 else _align.check_indices(who, idxs)

    def _align_kw(self, who, similarity_type):
        st = "qmax" if similarity_type is None else similarity_type
        self._check_align(who, np.zeros((0, 2), np.int32), self._align_plane(who, st))
        return {"similarity_type": st}

    def _align_call(self, pairs, want_paths, plane=0):
        if plane == 0:
            return Serra09._align_call(self, pairs, want_paths)
        if not want_paths:
            return self._context().chenfusion_align(pairs, self._params(), plane), None, None
        return self._context().chenfusion_align_paths(pairs, self._params(), plane)

    def align(self, idxs, similarity_type="qmax"):
        """Serra09.align() for the alignment similarity_type names: 'qmax' (the default: exactly Serra09's result) or 'dmax', the
        alignment behind the `dmax` score of the same cross recurrence plot.  Fields and spans are those of Serra09.align().  Dmax
        adds R[i-1][j] to the (i-2, j-1) predecessor and R[i][j-1] to the (i-1, j-2) one, so its start cell's value need not be 1,
        and the start can be a gap cell whose neighbour (q0 - 1, r0) or (q0, r0 - 1) is the recurrence at which the alignment really
        begins: q_span / r_span can begin one embedded frame late.  'Late' has no alignment of its own: ValueError."""
        plane = self._align_plane("align", similarity_type)
        return self._align_pairs(_align.check_pairs("align", self._check_align("align", idxs, plane), self._n_tracks()), None, plane)

    def align_paths(self, idxs, similarity_type="qmax"):
        """Serra09.align_paths() for 'qmax' (the default) or 'dmax': (al, paths), al exactly what align(idxs, similarity_type) returns."""
        plane = self._align_plane("align_paths", similarity_type)
        paths = []
        al = self._align_pairs(_align.check_pairs("align_paths", self._check_align("align_paths", idxs, plane), self._n_tracks()), paths, plane)
        return al, (paths if len(al) else [])

    def _check_plane_matches(self, who, queries, indices, plane):
        return _align.check_matches(who, self._check_align(who, queries, plane), self._check_align(who, indices, plane), self._n_tracks())

    def align_matches(self, queries, indices, similarity_type="qmax"):
        """Serra09.align_matches() for the hits identify() / rerank() list under similarity_type ('qmax', the default, or 'dmax')."""
        plane = self._align_plane("align_matches", similarity_type)
        idx, rows, slots, pairs = self._check_plane_matches("align_matches", queries, indices, plane)
        out = self._no_match_rows(idx.shape)
        out[rows, slots] = self._align_pairs(pairs, None, plane)
        return out

    def align_match_paths(self, queries, indices, similarity_type="qmax"):
        """Serra09.align_match_paths() for 'qmax' (the default) or 'dmax'."""
        plane = self._align_plane("align_match_paths", similarity_type)
        idx, rows, slots, pairs = self._check_plane_matches("align_match_paths", queries, indices, plane)
        out = self._no_match_rows(idx.shape)
        got = []
        out[rows, slots] = self._align_pairs(pairs, got, plane)
        return out, _align.scatter_paths(idx, rows, slots, got)

    def _sections_plane(self, who, similarity_type):
        """The sections are the Qmax alignment's: 'dmax' and 'Late' have none, ValueError naming the method."""
        if self._align_plane(who, similarity_type) != 0:
            raise ValueError("%s: the sections are those of the Qmax alignment; similarity_type must be 'qmax', got '%s'" % (who, similarity_type))

    def align_sections(self, idxs, max_sections=4, min_score=2.0, min_ratio=0.0, pad=0, paths=False, similarity_type="qmax"):
        """Serra09.align_sections() of the plot the class scores twice: the Qmax sections ('qmax', the default and the only one)."""
        self._sections_plane("align_sections", similarity_type)
        return Serra09.align_sections(self, idxs, max_sections, min_score, min_ratio, pad, paths)

    def align_match_sections(self, queries, indices, max_sections=4, min_score=2.0, min_ratio=0.0, pad=0, paths=False, similarity_type="qmax"):
        """Serra09.align_match_sections() for 'qmax' (the default and the only one)."""
        self._sections_plane("align_match_sections", similarity_type)
        return Serra09.align_match_sections(self, queries, indices, max_sections, min_score, min_ratio, pad, paths)

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
