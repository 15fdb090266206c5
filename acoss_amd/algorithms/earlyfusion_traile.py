"""
EarlyFusion (Tralie 2017: early MFCC / HPCP fusion).  Drop-in for the per-pair and fusion
surface of acoss/algorithms/earlyfusion_traile.py: same constructor, load_features(i),
similarity(idxs) writing Ds['mfccs'|'ssms'|'chromas'|'early'], do_late_fusion().

Everything numeric runs in libacx's HIP kernels:
  * block features (beat-synchronous MFCC / SSM / chroma blocks, earlyfusion_traile.py:100-140 with
    resize_block :214-247): acx_ef_block_features for one track (load_features(i)),
    acx_ef_upload_raw_pool for the whole collection, which never leaves the device.  The
    reference resizes blocks with skimage.transform.resize(anti_aliasing=True, mode='constant'), a
    library that is neither pinned by the reference (not in its setup.py) nor installed here: the
    kernel restates skimage's published algorithm -- PARITY UNPINNED for that step;
  * the per-pair chain (three cross-similarity matrices, row-kappa binarisation, constrained
    Smith-Waterman x4, kernel fusion; :157-198);
  * late fusion (similarity network fusion of the N x N score matrices, :200-206).
A track file that already holds block features (keys mfccs (nb,650), ssms (nb,1225), chromas
(nb,480), chroma_med (12,)) is used as is.
"""
import os

import numpy as np

from .. import _lib
from . import _align
from .algorithm_template import CoverAlgorithm, refused_in_session
from .similarity_fusion import doSimilarityFusion

__all__ = ["EarlyFusion"]

_KEYS = ("mfccs", "ssms", "chromas", "chroma_med")


class EarlyFusion(_align.AlignMixin, CoverAlgorithm):
    """Alignments (align, align_paths, align_matches, align_match_paths, align_sections, align_match_sections: _align.AlignMixin):
    the Smith-Waterman alignment of one of the four matrices the device binarises; similarity_type 'mfccs', 'ssms', 'chromas' or
    'early' (the default); 'late' and 'early+late' are fused from whole score matrices and have no alignment of their own:
    ValueError.  score is the value similarity() stores for that ORDERED pair and type.  Positions (q0, r0, q1, r1, the cells of a
    path, the rows a section excludes and its `pad`) are BLOCKS, rows (query) and columns (reference) of the binarised
    cross-similarity matrix (include/acx.h acx_ef_align); q_span / r_span are BEATS of each track: block b starts at beat b and spans
    `blocksize` beats, so a span is [q0, q1 + blocksize - 1] (a track of n beats has n - blocksize blocks: no clipping).
    align_matches() and its kin align the ordered pair (queries[i], indices[i, s]).  identify() of this symmetric class scored the
    cell (min, max) of the two indices: the score listed there is that of the pair (min(queries[i], indices[i, s]), max(...)), and
    passing THAT pair to align() gives the alignment behind the listed score; where the query has the larger index the row of
    align_matches() is the alignment of the transposed matrix, whose score may differ (locate_tracks() aligns the pair the listed
    score belongs to).  A list with a track of more than 1024 blocks takes the strip-wise alignment (ef_align_long), any other list
    runs as it always did; the sections need the bit path: tracks of at most 1024 blocks, NotImplementedError naming the method
    otherwise (align() serves longer ones)."""
    n_chunks = 1

    def __init__(self, dataset_csv, datapath, chroma_type='hpcp', shortname='Covers80', blocksize=20,
                 mfccs_per_block=50, ssm_res=50, chromas_per_block=40, kappa=0.1, K=10, niters=5,
                 log_times=False, device=None, nonfinite="raise", engine=None):
        """The reference's arguments (earlyfusion_traile.py:40-56), plus: `device`, `nonfinite` ("raise" | "propagate" for
        NaN / inf in the features), and `engine`, a dict of the library's arithmetic switches for this chain --
        {"gemm": "f16x2" (default) | "bf16x3" | "f32" | ...} (Context.set_ef_gemm: how the three cross-similarity
        products are evaluated; all within an f32 sgemm's accuracy) and {"fuse": "fast" (default) | "exact"}
        (Context.set_ef_fuse: getWCSM's kernel weights by reciprocal + exp2, or in numpy's own operation order)."""
        self._engine = dict(engine or {})
        unknown = set(self._engine) - {"gemm", "fuse"}
        if unknown:
            raise ValueError("EarlyFusion: unknown engine option(s) %s" % sorted(unknown))
        self.chroma_type = chroma_type
        self.blocksize = blocksize
        self.mfccs_per_block = mfccs_per_block
        self.chromas_per_block = chromas_per_block
        self.kappa = kappa
        self.K = K
        self.niters = niters
        self.all_block_feats = {}
        self.log_times = log_times
        if log_times:
            self.times = {'features': [], 'raw': []}
        self._device = device
        self._nonfinite = nonfinite
        self._ctx = None
        self._pool_ready = False
        self._bind_collective_device(self._device)      # before the first collective of this object
        CoverAlgorithm.__init__(self, dataset_csv=dataset_csv, name="EarlyFusionTraile", datapath=datapath,
                                shortname=shortname, similarity_types=["mfccs", "ssms", "chromas", "early"])

    def get_cacheprefix(self):
        return "%s/%s_%s_%s" % (self.cachedir, self.name, self.shortname, self.chroma_type)

    def load_features(self, i, do_plot=False):
        if i in self.all_block_feats:
            return self.all_block_feats[i]
        feats = CoverAlgorithm.load_features(self, i)
        if all(k in feats for k in _KEYS):
            self.all_block_feats[i] = {k: np.asarray(feats[k]) for k in _KEYS}
        else:
            import time
            tic = time.time()
            raw = self._raw_track(feats)
            self.all_block_feats[i] = self._fusion_context().ef_block_features(
                raw["chroma"], raw["mfcc"], raw["onsets"], self.blocksize, self.mfccs_per_block, self.chromas_per_block)
            if self.log_times:
                self.times['features'].append(time.time() - tic)
        return self.all_block_feats[i]

    def _raw_track(self, feats):
        """What the block features are made of (earlyfusion_traile.py:103-110): the chroma (T, 12), the
        MFCCs time-major (feats['mfcc_htk'].T) and the beat onsets in frames."""
        return dict(chroma=np.asarray(feats[self.chroma_type], dtype=np.float32),
                    mfcc=np.ascontiguousarray(np.asarray(feats["mfcc_htk"], dtype=np.float32).T),
                    onsets=np.asarray(feats["madmom_features"]["onsets"]).astype(np.int64))

    @refused_in_session
    def set_block_features(self, tracks, labels=None):
        assert len(tracks) == self.N
        self.all_block_feats = dict(enumerate(tracks))
        if labels is not None:
            for i, l in enumerate(labels):
                self._register_label(i, l)
        self._pool_ready = False

    def _context(self):
        self._fusion_context()
        if not self._pool_ready:
            feats = None
            if not self.all_block_feats:
                feats = [CoverAlgorithm.load_features(self, i) for i in range(self.N)]
            if feats is not None and not any(all(k in f for k in _KEYS) for f in feats):
                # raw features of every track -> block features built and kept on the device
                self._ctx.ef_upload_raw_pool([self._raw_track(f) for f in feats], self.blocksize,
                                             self.mfccs_per_block, self.chromas_per_block)
            else:
                self._ctx.ef_upload_pool([self.load_features(i) for i in range(self.N)])
            self._pool_ready = True
        return self._ctx

    def _check_tracks(self, who, tracks):
        out = []
        for i, t in enumerate(tracks):
            if not isinstance(t, dict) or not all(k in t for k in _KEYS):
                raise ValueError("%s: track %d must be a dict of block features with the keys %s" % (who, i, list(_KEYS)))
            mats = {k: np.asarray(t[k]) for k in ("mfccs", "ssms", "chromas")}
            for k, m in mats.items():
                if m.ndim != 2 or m.dtype.kind != "f":
                    raise ValueError("%s: track %d: %s must be a floating-point (blocks, dim) array, got %s %s" % (who, i, k, m.dtype, m.shape))
            if len({m.shape[0] for m in mats.values()}) != 1:
                raise ValueError("%s: track %d: mfccs, ssms and chromas must have the same number of blocks" % (who, i))
            ref = self.all_block_feats.get(0) if self.all_block_feats else None
            ref = ref if ref is not None else (out[0] if out else None)
            if ref is not None and any(mats[k].shape[1] != np.asarray(ref[k]).shape[1] for k in mats):
                raise ValueError("%s: track %d: block-feature widths %s differ from the collection's" % (who, i, [mats[k].shape[1] for k in mats]))
            med = np.asarray(t["chroma_med"], dtype=np.float64)
            if med.size != 12:
                raise ValueError("%s: track %d: chroma_med must hold 12 values" % (who, i))
            out.append(dict(mfccs=mats["mfccs"], ssms=mats["ssms"], chromas=mats["chromas"], chroma_med=med.reshape(12)))
        return out

    def _append_tracks(self, ctx, tracks):
        ctx.ef_pool_append(tracks)
        return None

    _identify_planes = ("mfccs", "ssms", "chromas", "early")
    _identify_fused = ("late", "early+late")
    # do_late_fusion's two lists, as distances 1 / (1 + s)
    _fused_planes = {"late": ("chromas", "ssms", "mfccs"), "early+late": ("chromas", "ssms", "mfccs", "early")}
    _fused_transform = _lib.FUSED_INV1P

    def _grid(self):
        return (self._context(), _lib.ALGO_EARLYFUSION, _lib.EfParams(float(self.kappa), int(self.K)),
                ["mfccs", "ssms", "chromas", "early"])

    @refused_in_session
    def similarity(self, idxs, do_plot=False):
        idxs = np.asarray(idxs).reshape(-1, 2)
        if len(idxs) == 0:
            return
        sc = self._context().earlyfusion_pairs(idxs.astype(np.int32), kappa=self.kappa, K=self.K)
        for c, s in enumerate(("mfccs", "ssms", "chromas", "early")):
            self.Ds[s][idxs[:, 0], idxs[:, 1]] = sc[:, c]

    # ------------------------------------------------------------------ the full cross-diffusion fusion for listed pairs
    def _check_full_fusion(self, who):
        """The class's own arguments as the library will refuse them, before the first library call."""
        if int(self.niters) < 1:
            raise ValueError("%s: niters must be >= 1 (got %d)" % (who, int(self.niters)))
        if int(self.K) < 1:
            raise ValueError("%s: K must be >= 1 (got %d)" % (who, int(self.K)))
        if int(self.K) > 64:
            raise NotImplementedError("%s: more than 64 neighbours are not supported on the device (K = %d)" % (who, int(self.K)))

    def full_fusion(self, idxs):
        """The score of the PUBLISHED early fusion (Tralie, ISMIR 2017), the "Step 3" the reference disables
        (earlyfusion_traile.py:142-148) because it was too slow in numpy: idxs (K, 2) ordered (A, B) track indices -> (K,)
        float32.  Per feature the self-similarity matrices of A and B and their cross-similarity matrix become one
        (M + N) x (M + N) affinity matrix (getWCSMSSM, K neighbours split between the blocks); the three are cross-diffused by
        similarity network fusion (doSimilarityFusionWs, K, niters, reg_diag = 1); the two cross blocks of the result are summed,
        binarised (the round(kappa N) largest of every row) and aligned by Smith-Waterman.  The stages are the reference's
        functions, the composition is the method's (include/acx.h acx_ef_crossfusion_pairs).  Tracks of at most 1024 blocks; a
        pair whose k1 = int(K M / (M + N)) or k2 = K - k1 leaves np.partition no room is refused (NotImplementedError naming
        the pair).  `Ds` is not written: this score is not one of similarity_types.  Not a collective."""
        self._check_full_fusion("full_fusion")
        pairs = _align.check_pairs("full_fusion", _align.check_indices("full_fusion", idxs), self._n_tracks())
        if len(pairs) == 0:
            return np.zeros(0, np.float32)
        return self._context().ef_crossfusion(pairs, self.kappa, self.K, self.niters, 1.0)

    def rerank_full(self, queries, shortlists, k=10):
        """rerank() by the full-fusion score: queries (Q,) track indices, shortlists as rerank() takes them ((Q, L) integers or
        Q sequences, -1 an empty slot, no track twice in a row) -> (indices (Q, k) int32, scores (Q, k) float32), the k best
        candidates of every query by score descending, then smaller track index; slots beyond a query's candidates hold -1 and
        NaN.  The cell of (query, candidate) is the pair (min, max) of the two indices, as identify() scores this symmetric class;
        a query's own track is skipped.  Only the listed cells are computed.  `Ds` is not written.  Not a collective."""
        self._check_full_fusion("rerank_full")
        q, _ = self._query_setup("rerank_full", queries, None)
        k = self._check_k("rerank_full", k)
        lists = self._check_shortlists("rerank_full", shortlists, len(q))
        idx = np.full((len(q), k), -1, np.int32)
        score = np.full((len(q), k), np.nan, np.float32)
        rows, slots = np.nonzero((lists >= 0) & (lists != q[:, None]))
        if len(rows) == 0:
            return idx, score
        cand = lists[rows, slots]
        pairs = np.stack([np.minimum(q[rows], cand), np.maximum(q[rows], cand)], axis=1).astype(np.int32)
        uniq, inv = np.unique(pairs, axis=0, return_inverse=True)
        sc = self._context().ef_crossfusion(uniq, self.kappa, self.K, self.niters, 1.0)[np.asarray(inv).reshape(-1)]
        for i in range(len(q)):
            mine = rows == i
            c_i, s_i = cand[mine], sc[mine]
            order = np.lexsort((c_i, -s_i.astype(np.float64)))[:k]
            idx[i, :len(order)] = c_i[order]
            score[i, :len(order)] = s_i[order]
        return idx, score

    # ------------------------------------------------------------------ where the alignment lies: AlignMixin's hooks
    # locate_tracks(): 'early' unless asked otherwise, and the pair the listed score belongs to, (hit, new track)
    _locate_type = "early"
    _locate_hit_first = True

    def _align_call(self, pairs, want_paths, plane):
        ctx = self._context()
        # a listed track of more than 1024 blocks: the strip-wise alignment of the float path (ef_align_long); else ef_align, with the
        # launches it always had
        fn = ctx.ef_align_long if ctx.ef_has_long_track(pairs) else ctx.ef_align
        if not want_paths:
            return fn(pairs, self.kappa, self.K, plane), None, None
        return fn(pairs, self.kappa, self.K, plane, paths=True)

    def _sections_call(self, who, pairs, plane, o, want_paths):
        ctx = self._context()
        if ctx.ef_has_long_track(pairs) and getattr(ctx, "ef_blocks", None) is not None:
            raise NotImplementedError("%s: sections need the bit path: tracks of at most 1024 blocks (align() serves longer ones)" % who)
        return ctx.ef_align_sections(pairs, self.kappa, self.K, plane, o, paths=want_paths)

    def _spans(self, al, pairs):
        """[q0, q1 + blocksize - 1] in beats: block b covers beats b .. b + blocksize - 1."""
        return [np.stack([al[side + "0"], al[side + "1"] + int(self.blocksize) - 1], axis=1) for side in ("q", "r")]

    # every matched section of a pair: this class's positional order, similarity_type right behind the indices
    def align_sections(self, idxs, similarity_type=None, max_sections=4, min_score=2.0, min_ratio=0.0, pad=0, paths=False):
        """AlignMixin.align_sections() -- sections of the Smith-Waterman alignment, rows and `pad` in BLOCKS -- with similarity_type
        right behind the indices.  Tracks of at most 1024 blocks (NotImplementedError naming the method otherwise)."""
        return _align.AlignMixin.align_sections(self, idxs, max_sections, min_score, min_ratio, pad, paths, similarity_type)

    def align_match_sections(self, queries, indices, similarity_type=None, max_sections=4, min_score=2.0, min_ratio=0.0, pad=0, paths=False):
        """AlignMixin.align_match_sections() with similarity_type right behind the indices; as align_sections()."""
        return _align.AlignMixin.align_match_sections(self, queries, indices, max_sections, min_score, min_ratio, pad, paths, similarity_type)

    def _fusion_context(self):
        """The GPU context of the pair grid, or a fresh one (scores loaded with precomputed=True)."""
        if getattr(self, "_ctx", None) is None:
            dev = getattr(self, "_device", None)
            self._ctx = _lib.Context(dev if dev is not None else int(os.environ.get("LOCAL_RANK", "0")), nonfinite=getattr(self, "_nonfinite", "raise"))
            eng = getattr(self, "_engine", {})
            if "gemm" in eng:
                self._ctx.set_ef_gemm(eng["gemm"])
            if "fuse" in eng:
                self._ctx.set_ef_fuse(eng["fuse"])
        return self._ctx

    @refused_in_session
    def do_late_fusion(self):
        """SNF of 1/(1+D) over the three / four score matrices (earlyfusion_traile.py:200-206), on the
        GPU (acx_snf_fuse_dists; no device -> the call fails) of the rank that owns the matrices."""
        if not self.owns_result():
            for key in ("late", "early+late"):                  # same keys on every rank (getEvalStatistics is collective)
                self.Ds[key] = np.zeros((0, 0), np.float64)
            return

        def inv(s):
            return 1.0 / (1.0 + np.array(self.Ds[s], dtype=np.float64))
        ctx = self._fusion_context()
        self.Ds["late"] = doSimilarityFusion([inv(s) for s in ("chromas", "ssms", "mfccs")],
                                             K=20, niters=20, reg_diag=1, ctx=ctx, want_ws=False)[1]
        self.Ds["early+late"] = doSimilarityFusion([inv(s) for s in ("chromas", "ssms", "mfccs", "early")],
                                                   K=20, niters=20, reg_diag=1, ctx=ctx, want_ws=False)[1]
