"""
The Python alignment surface of Serra09, ChenFusion and EarlyFusion: the argument checks and the no-match rows
(every check runs before the first library call), and AlignMixin, which holds the six public methods -- align, align_paths,
align_matches, align_match_paths, align_sections, align_match_sections -- and their skeleton once.  A class fills in the hooks.
"""
import numpy as np

from .. import _lib

NO_MATCH_FIELDS = ("q0", "r0", "q1", "r1", "q_span", "r_span")


def check_indices(who, idxs):
    a = np.asarray(idxs)
    if a.size and not np.issubdtype(a.dtype, np.integer):
        raise ValueError("%s: track indices must be integers, got dtype %s" % (who, a.dtype))
    return a


def check_pairs(who, a, n):
    """align() / align_paths(): checked indices -> (K, 2) int32 pairs over a collection of n tracks."""
    if a.size == 0:
        a = a.reshape(0, 2)
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError("%s: idxs must be (K, 2) (query, reference) track indices, got shape %s" % (who, a.shape))
    if a.size and (a.min() < 0 or a.max() >= n):
        raise ValueError("%s: idxs must be track indices in [0, %d)" % (who, n))
    return np.ascontiguousarray(a, dtype=np.int32)


def check_matches(who, q, idx, n):
    """align_matches() / align_match_paths(): checked queries and indices -> (the (Q, k) index array, rows and slots of its filled
    slots, their (P, 2) pairs)."""
    q = q.reshape(-1)
    if idx.ndim != 2 or idx.shape[0] != len(q):
        raise ValueError("%s: indices must be (Q, k) with one row per query (%d), got shape %s" % (who, len(q), idx.shape))
    if q.size and (q.min() < 0 or q.max() >= n):
        raise ValueError("%s: queries must be track indices in [0, %d)" % (who, n))
    if idx.size and (idx.min() < -1 or idx.max() >= n):
        raise ValueError("%s: indices must be track indices in [0, %d) or -1" % (who, n))
    rows, slots = np.nonzero(idx >= 0)
    pairs = np.stack([q[rows], idx[rows, slots]], axis=1).astype(np.int32).reshape(-1, 2)
    return idx, rows, slots, np.ascontiguousarray(pairs)


def no_match_rows(shape, dtype):
    out = np.zeros(shape, dtype)
    for f in NO_MATCH_FIELDS:
        out[f] = -1
    return out


def scatter_paths(idx, rows, slots, got):
    """The (Q, k) lists of paths of align_match_paths: `got` are the paths of the filled slots, an empty slot has an empty path."""
    paths = [[np.zeros((0, 2), np.int32) for _ in range(idx.shape[1])] for _ in range(idx.shape[0])]
    for r, s, p in zip(rows, slots, got):
        paths[r][s] = p
    return paths


class AlignMixin(object):
    """WHERE the alignment behind a score lies: the six methods below, once for every class that aligns a binary plot of a (query,
    reference) pair by a recursion over its cells (Serra09 and ChenFusion: the cross recurrence plot; EarlyFusion: a binarised
    cross-similarity matrix).  The units of positions and spans, the similarity types and the caveats are the class's: read the
    "Alignments" paragraph of its docstring.  similarity_type None is the class's default type.  Every argument check comes before the
    first library call; `Ds` is not written; none of the methods is a collective.

    What a class provides -- beside _identify_planes / _identify_fused (the types, in the order of the device's planes) and
    _locate_type (the default type; None: the first plane):
      _check_align(who, idxs, plane)                          a refusal of its own for the plane, then check_indices (the default)
      _sections_plane(who, similarity_type)                   the plane whose sections are wanted (default: _align_plane)
      _align_call(pairs, want_paths, plane)                   the library call: (records, offsets, cells), the last two None without paths
      _sections_call(who, pairs, plane, opts, want_paths)     the library call: (records (P, S), counts[, offsets, cells])
      _spans(al, pairs)                                       (q_span, r_span), each (K, 2), of the (K,) records of the (K, 2) pairs"""

    # acx_alignment's fields and the two spans, [first, last] inclusive
    ALIGN_DTYPE = np.dtype(_lib.ALIGNMENT_DTYPE.descr + [("q_span", np.int32, (2,)), ("r_span", np.int32, (2,))])

    # ------------------------------------------------------------------ the checks
    def _align_plane(self, who, similarity_type):
        """similarity_type (None: the class's default) -> the device plane; raises for a fused type and for anything else, before
        anything else is checked."""
        if similarity_type is None:
            similarity_type = self._locate_type or self._identify_planes[0]
        if similarity_type in self._identify_fused:
            raise ValueError("%s: '%s' is fused from whole score matrices and has no alignment of its own; similarity_type must be one of %s"
                             % (who, similarity_type, list(self._identify_planes)))
        if similarity_type not in self._identify_planes:
            raise ValueError("%s: unknown similarity type %r; similarity_type must be one of %s" % (who, similarity_type, list(self._identify_planes)))
        return self._identify_planes.index(similarity_type)

    def _check_align(self, who, idxs, plane):
        return check_indices(who, idxs)

    def _sections_plane(self, who, similarity_type):
        return self._align_plane(who, similarity_type)

    def _align_kw(self, who, similarity_type):
        """CoverAlgorithm's seam for align_tracks() / locate_tracks(): similarity_type checked as the methods below check it."""
        self._check_align(who, np.zeros((0, 2), np.int32), self._align_plane(who, similarity_type))
        return {"similarity_type": similarity_type}

    def _check_align_pairs(self, who, idxs, plane=0):
        """idxs -> (K, 2) int32 pairs."""
        return check_pairs(who, self._check_align(who, idxs, plane), self._n_tracks())

    def _check_align_matches(self, who, queries, indices, plane=0):
        """-> (the (Q, k) index array, rows and slots of its filled slots, their (P, 2) pairs)."""
        return check_matches(who, self._check_align(who, queries, plane), self._check_align(who, indices, plane), self._n_tracks())

    def _no_match_rows(self, shape):
        return no_match_rows(shape, self.ALIGN_DTYPE)

    # ------------------------------------------------------------------ records -> rows
    def _align_rows(self, al, pairs):
        """(K,) records of the library for the (K, 2) pairs -> (K,) ALIGN_DTYPE: the fields, and the class's spans where there is a match."""
        out = self._no_match_rows(len(pairs))
        for f in _lib.ALIGNMENT_DTYPE.names:
            out[f] = al[f]
        hit = al["q0"] >= 0
        for name, span in zip(("q_span", "r_span"), self._spans(al, pairs)):
            out[name][hit] = span[hit]
        return out

    def _align_pairs(self, pairs, plane, paths=None):
        """(K, 2) checked int32 pairs -> (K,) ALIGN_DTYPE.  paths: a list that receives the K (L_k, 2) int32 paths as well."""
        if len(pairs) == 0:
            return self._no_match_rows(0)
        al, off, cells = self._align_call(pairs, paths is not None, plane)
        if paths is not None:
            paths.extend(cells[off[k]:off[k + 1]] for k in range(len(pairs)))
        return self._align_rows(al, pairs)

    def _align_matches(self, who, queries, indices, similarity_type, paths=None):
        """The matches scatter: -> (the (Q, k) rows, an empty slot a no-match row; the index array, rows and slots of its filled slots)."""
        plane = self._align_plane(who, similarity_type)
        idx, rows, slots, pairs = self._check_align_matches(who, queries, indices, plane)
        out = self._no_match_rows(idx.shape)
        out[rows, slots] = self._align_pairs(pairs, plane, paths)
        return out, idx, rows, slots

    def _section_pairs(self, who, pairs, plane, o, want_paths):
        """(P, 2) checked int32 pairs -> (a P-list of (n_k,) ALIGN_DTYPE arrays, a P-list of lists of n_k (L, 2) int32 paths or None)."""
        if len(pairs) == 0:
            return [], ([] if want_paths else None)
        got = self._sections_call(who, pairs, plane, o, want_paths)
        al, n = got[0], got[1]
        S = al.shape[1]
        out = self._align_rows(al.reshape(-1), np.repeat(pairs, S, axis=0)).reshape(al.shape)      # (align()'s rows, a pair's S together)
        sections = [out[k, :n[k]].copy() for k in range(len(pairs))]
        if not want_paths:
            return sections, None
        off, cells = got[2], got[3]
        return sections, [[cells[off[k * S + s]:off[k * S + s + 1]] for s in range(n[k])] for k in range(len(pairs))]

    # ------------------------------------------------------------------ where the alignment lies
    def align(self, idxs, similarity_type=None):
        """WHERE in the two recordings does the alignment lie?  idxs: (K, 2) (query, reference) track indices over the uploaded
        collection (inside an appended() session: over its tracks as well).  Returns a (K,) structured array: score (the value
        similarity() stores for that ordered pair and type, before any normalize_by_length), the path's start (q0, r0) and end
        (q1, r1) -- rows (query) and columns (reference) of the binary plot; the end is the row-major first maximum of the recursion,
        the start is found by following the recursion's predecessors back (include/acx.h acx_alignment) -- and q_span / r_span,
        [first, last] inclusive in each track.  A pair without a match (score 0) has -1 everywhere.  An empty idxs: an empty array."""
        plane = self._align_plane("align", similarity_type)
        return self._align_pairs(self._check_align_pairs("align", idxs, plane), plane)

    def align_paths(self, idxs, similarity_type=None):
        """align() and, for every pair, the PATH of its alignment: (al, paths).  al is exactly what align(idxs, similarity_type)
        returns; paths is a list of K (L_k, 2) int32 arrays, the cells (q, r) of the plot that the recursion's predecessors visit
        between the start and the end, both included, listed from (q0, r0) to (q1, r1) -- which position of the query corresponds to
        which position of the reference.  Consecutive cells differ by (1, 1), (2, 1) or (1, 2); a pair without a match has an empty
        (0, 2) path.  Cells are in the units of (q0, r0)."""
        plane = self._align_plane("align_paths", similarity_type)
        paths = []
        al = self._align_pairs(self._check_align_pairs("align_paths", idxs, plane), plane, paths)
        return al, (paths if len(al) else [])

    def align_matches(self, queries, indices, similarity_type=None):
        """align() for the hits of identify() / rerank(): queries (Q,) track indices, indices the (Q, k) int array either
        returned (-1: an empty slot).  Returns a (Q, k) structured array as align() does, row i slot s being the alignment of the
        ORDERED pair (queries[i], indices[i, s]); an empty slot comes back as a no-match row."""
        return self._align_matches("align_matches", queries, indices, similarity_type)[0]

    def align_match_paths(self, queries, indices, similarity_type=None):
        """align_matches() with the paths: (the (Q, k) array align_matches returns, a Q-list of k-lists of (L, 2) int32 paths as
        align_paths lists them); an empty slot (-1) has an empty path."""
        got = []
        out, idx, rows, slots = self._align_matches("align_match_paths", queries, indices, similarity_type, got)
        return out, scatter_paths(idx, rows, slots, got)

    # ------------------------------------------------------------------ every matched section of a pair (DESIGN.md sections 28, 29)
    def _sections_setup(self, who, similarity_type, max_sections, min_score, min_ratio, pad):
        """The plane, then the options: both before the indices."""
        return self._sections_plane(who, similarity_type), _lib.section_opts(who, max_sections, min_score, min_ratio, pad)

    def align_sections(self, idxs, max_sections=4, min_score=2.0, min_ratio=0.0, pad=0, paths=False, similarity_type=None):
        """EVERY matched section of a pair, not only the best alignment: a cover that repeats the chorus once more, a live version
        with a solo between two matched halves, a medley that quotes two passages of one reference.  idxs and similarity_type as
        for align().  Returns a K-list of (n_k,) structured arrays with align()'s fields and spans, n_k <= max_sections (at most
        16), section 0 first; with paths=True (sections, paths), paths[k] a list of n_k (L, 2) int32 arrays as align_paths() lists them.
          section 0      exactly align()'s row for the pair, provided its score >= min_score; otherwise the pair has no sections
          section k + 1  the alignment of what is left when the QUERY's rows q0 .. q1 of every section found so far, and `pad`
                         rows on either side of each (never across an earlier section), are excluded -- the recursion's value
                         is 0 on those rows, so no alignment runs through them; reported iff its score >=
                         max(min_score, min_ratio * section 0's score).  The search ends at the first section that fails.
        Scores do not increase with k; every QUERY row belongs to at most one section (the row ranges are disjoint), while
        reference columns may be shared: the query repeats a chorus the reference plays once.  The sections segment the query;
        for a segmentation of the reference swap the pair.  min_score must be > 1, 0 <= min_ratio <= 1, pad >= 0."""
        plane, o = self._sections_setup("align_sections", similarity_type, max_sections, min_score, min_ratio, pad)
        pairs = self._check_align_pairs("align_sections", idxs, plane)
        sections, got = self._section_pairs("align_sections", pairs, plane, o, bool(paths))
        return (sections, got) if paths else sections

    def align_match_sections(self, queries, indices, max_sections=4, min_score=2.0, min_ratio=0.0, pad=0, paths=False, similarity_type=None):
        """align_sections() for the hits of identify() / rerank(): queries (Q,) track indices, indices the (Q, k) int array either
        returned (-1: an empty slot).  Returns a Q-list of k-lists of (n,) arrays as align_sections() returns them, slot s of row i
        for the ORDERED pair (queries[i], indices[i, s]) -- an empty slot is an empty array -- and with paths=True (sections,
        paths), paths a Q-list of k-lists of lists of (L, 2) int32 arrays."""
        plane, o = self._sections_setup("align_match_sections", similarity_type, max_sections, min_score, min_ratio, pad)
        idx, rows, slots, pairs = self._check_align_matches("align_match_sections", queries, indices, plane)
        sections, got = self._section_pairs("align_match_sections", pairs, plane, o, bool(paths))
        out = [[np.zeros(0, self.ALIGN_DTYPE) for _ in range(idx.shape[1])] for _ in range(idx.shape[0])]
        out_paths = [[[] for _ in range(idx.shape[1])] for _ in range(idx.shape[0])]
        for t, (r, s) in enumerate(zip(rows, slots)):
            out[r][s] = sections[t]
            if paths:
                out_paths[r][s] = got[t]
        return (out, out_paths) if paths else out
