"""
CoverAlgorithm: the harness every cover-id algorithm subclasses.  Mirrors the interface
of acoss/algorithms/algorithm_template.py (ctor :30-62, load_features :71-95,
get_all_clique_ids :97-119, similarity :121-140, all_pairwise :142-192,
cleanup_memmap :194-203, getEvalStatistics :205-290) so that user subclasses written
against acoss keep working, while device-backed subclasses hand the WHOLE pair list to
libacx in a few calls.

Differences from the reference, all deliberate:
  * the pair list is a numpy (K,2) array, not a Python list of tuples (1.1e8 tuples at
    N = 15 000 would need > 10 GB);
  * getEvalStatistics is vectorised (the reference's N x N Python double loop takes
    hours at N = 15 000) and uses a STABLE argsort so that ties have one defined order;
  * cleanup_memmap really removes the memmap files (the reference calls rmtree on a file
    and always fails);
  * the distance matrices are saved as <prefix>_Ds.h5 (libhdf5 / h5py) and, when small or when no HDF5 library exists, <prefix>_Ds.npz;
  * device-backed subclasses (those with a _grid() method) never build the pair list at all:
    libacx enumerates the N x N grid itself in cost-balanced tiles (acx_pair_grid; under
    torch.distributed, one process per GPU, acx_grid_run + ONE gather of the tile scores to rank 0,
    scattered into the matrices by rank 0).  User subclasses that implement similarity()
    themselves keep the reference's chunked pair-list loop (sharded by pair count over the ranks).
  * under torch.distributed rank 0 owns the result: it alone holds the filled matrices, writes
    the cache / results files and computes the statistics, which are broadcast to the others.
"""
import contextlib
import functools
import os
import warnings

import numpy as np

from .. import _lib
from .. import dist as _dist
from ..featurestore import load_track, load_matrices_h5, save_matrices_h5
from ..utils import create_dataset_filepaths
from . import _align

__all__ = ["CoverAlgorithm", "AppendedSession", "refused_in_session"]


class AppendedSession(object):
    """What `with algo.appended(tracks) as s` yields: the Q appended tracks are tracks first .. total - 1 of the pool while the
    block runs.  indices: np.arange(first, total) int32; first == algo.N; count == Q; total == N + Q; labels: the clique
    labels given for the new tracks (None: evaluate() is refused)."""

    def __init__(self, first, count, labels=None):
        self.first, self.count, self.total = int(first), int(count), int(first) + int(count)
        self.indices = np.arange(self.first, self.total, dtype=np.int32)
        self.labels = labels
        self.col_tail = None            # _identify_norm's column values of the new tracks (_append_tracks returns them)


def refused_in_session(method):
    """Marks a method that writes `Ds`, assumes an N x N result, or changes the pool or the feature caches: inside an
    appended() session it raises a RuntimeError naming itself, before anything else happens."""
    @functools.wraps(method)
    def guarded(self, *args, **kwargs):
        if getattr(self, "_session", None) is not None:
            raise RuntimeError("%s: refused inside an appended() session (the pool holds %d tracks behind the collection's %d); "
                               "leave the `with` block first" % (method.__name__, self._session.count, self.N))
        return method(self, *args, **kwargs)
    return guarded


class CoverAlgorithm(object):
    """
    Attributes
    ----------
    filepaths: list(string)   paths of all feature files of the dataset
    cliques: {label: set(int)}  cover cliques, indexing into filepaths
    N: int
    Ds: {similarity type: (N, N) float32 memmap}   pairwise similarity matrices
    """

    # how many chunks all_pairwise cuts the pair list into before calling similarity();
    # 45 is what the reference does (algorithm_template.py:172); device-backed subclasses
    # override this with 1 (whole list per call).
    n_chunks = 45

    # where getEvalStatistics ranks the score rows: "host" (numpy, eval_statistics) or "device" (libacx's ranking kernels,
    # eval_statistics_device: the same statistics from integer positions counted on the GPU)
    eval_engine = "host"

    def __init__(self, dataset_csv, name="Serra09", datapath="features_benchmark", shortname="full",
                 cachedir="cache", similarity_types=["main"]):
        self.name = name
        self.shortname = shortname
        self.cachedir = cachedir
        self.filepaths = create_dataset_filepaths(dataset_csv, root_audio_dir=datapath, file_format=".h5")
        self.cliques = {}
        self.N = len(self.filepaths)
        if not os.path.exists(cachedir):
            os.makedirs(cachedir, exist_ok=True)
        self.Ds = {}
        # the file names are fixed here: rank 0 owns the reference's names, other ranks (whose matrices
        # stay empty) get a suffix even if the process group is initialised or torn down later
        self._dmat_rank = _dist.world()[0]
        self._dmat_paths = {}
        for s in similarity_types:
            self.Ds[s] = np.memmap(self._dmat_path(s), shape=(self.N, self.N), mode="w+", dtype="float32")
        print("Initialized %s algorithm on %i songs in dataset %s" % (name, self.N, shortname))

    # ------------------------------------------------------------------ files / caches
    def get_cacheprefix(self):
        return "%s/%s_%s" % (self.cachedir, self.name, self.shortname)

    def _dmat_path(self, s):
        if s not in self._dmat_paths:
            rank = self._dmat_rank
            self._dmat_paths[s] = "%s_%s_dmat%s" % (self.get_cacheprefix(), s, "" if rank == 0 else ".rank%d" % rank)
        return self._dmat_paths[s]

    def _bind_collective_device(self, device):
        """Device-backed classes call this from their constructor with the GPU their libacx context will use (None:
        LOCAL_RANK's): under a process group, torch's collectives are bound to THAT device before the first of them
        runs (the clique-table broadcast can precede the first kernel).  A second, different device in one process is
        refused right here, in the constructor, on the rank that asked for it -- not in the middle of all_pairwise
        with the other ranks already waiting in a collective.  Without a process group nothing happens: no device is
        bound, no collective runs (dist.single() does import torch.distributed when torch is installed -- that creates no
        process group and touches no GPU)."""
        dev = int(os.environ.get("LOCAL_RANK", "0")) if device is None else int(device)
        if not _dist.single():
            try:
                import torch.distributed as tdist
                if tdist.get_backend() == "nccl":
                    _dist.bind_device(dev)
            except ImportError:
                pass
        return dev

    def owns_result(self):
        """True on the rank that holds the filled matrices (rank 0, or the only process).  The N x N
        post-processing steps (normalize_by_length, do_late_fusion) return at once everywhere else:
        the other ranks' matrices stay empty by design."""
        return _dist.world()[0] == 0

    def _register_label(self, i, label):
        self.cliques.setdefault(label, set()).add(int(i))

    def load_features(self, i):
        """Feature dict of track i; records its clique (feats['label']) as a side effect."""
        feats = load_track(self.filepaths[i])
        self._register_label(i, feats["label"])
        return feats

    def get_all_clique_ids(self, verbose=False):
        """Clique membership of every track, cached in <prefix>_clique_info.txt ("i,label").
        Under torch.distributed this is a COLLECTIVE (every rank must call it): rank 0 reads the cache
        file -- or builds it from the feature files -- and broadcasts the table; the other ranks touch
        neither the feature files nor the cache (no shared file system is assumed)."""
        path = "%s_clique_info.txt" % self.get_cacheprefix()

        def build():
            table = []
            if os.path.exists(path):
                with open(path) as fin:
                    for line in fin:
                        i, label = line.split(",", 1)
                        table.append((int(i), label.strip()))
            else:
                # written to a temporary name and renamed: nobody ever sees half a file
                tmp = "%s.tmp%d" % (path, os.getpid())
                with open(tmp, "w") as fout:
                    for i in range(len(self.filepaths)):
                        feats = CoverAlgorithm.load_features(self, i)
                        if verbose:
                            print(i)
                        fout.write("%i,%s\n" % (i, feats["label"]))
                        table.append((i, str(feats["label"]).strip()))
                os.replace(tmp, path)
            return table
        table = _dist.on_root(build)          # a failure on rank 0 is re-raised on every rank (no rank is left waiting)
        for i, label in table:
            self._register_label(int(i), label)

    # ------------------------------------------------------------------ pairwise
    @refused_in_session
    def similarity(self, idxs):
        """idxs: (K,2) int array.  Writes Ds[type][i, j] for every row; the return value is
        ignored.  The base class stores zeros."""
        idxs = np.asarray(idxs)
        self.Ds["main"][idxs[:, 0], idxs[:, 1]] = 0.0

    @staticmethod
    def pair_list(N, symmetric):
        """(K,2) int64 array in itertools.combinations / permutations order
        (algorithm_template.py:168-171)."""
        if symmetric:
            i, j = np.triu_indices(N, 1)
        else:
            i, j = np.nonzero(~np.eye(N, dtype=bool))
        return np.stack([i, j], axis=1).astype(np.int64)

    @refused_in_session
    def all_pairwise(self, parallel=0, n_cores=12, symmetric=False, precomputed=False):
        """All pairwise comparisons.  Device-backed classes ignore `parallel` / `n_cores`: their fan-out unit is the GPU
        (one process per GPU under torch.distributed).  User subclasses that bring their own CPU `similarity()` get the
        reference's behaviour: `parallel=1` spreads the 45 chunks over `n_cores` joblib workers (single process group only)."""
        npz = "%s_Ds.npz" % self.get_cacheprefix()
        h5 = "%s_Ds.h5" % self.get_cacheprefix()          # the reference's cache file (algorithm_template.py:163-166,192)
        if precomputed:
            loaded = {}
            if not self.owns_result():
                pass                                           # the cache belongs to rank 0, like the result
            elif os.path.exists(npz):
                with np.load(npz) as z:
                    loaded = {s: z[s] for s in z.files}
            else:
                loaded = load_matrices_h5(h5)                  # a cache written by acoss itself (needs h5py)
            for s, M in loaded.items():
                if s in self.Ds:
                    self.Ds[s][:] = M
                else:
                    self.Ds[s] = M
            self.get_all_clique_ids()
            return
        rank, ws = _dist.world()
        if hasattr(self, "_grid"):
            self._all_pairwise_grid(symmetric)
        else:
            pairs = self.pair_list(self.N, symmetric)
            lo, hi = _dist.shard_bounds(len(pairs), rank, ws)
            mine = pairs[lo:hi]
            chunks = [c for c in np.array_split(mine, max(1, min(self.n_chunks, len(mine)))) if len(c)]
            if parallel and n_cores != 1 and ws == 1 and self._joblib_fanout(chunks, n_cores):
                pass                                           # the reference's joblib fan-out (algorithm_template.py:172-177)
            else:
                for chunk in chunks:
                    self.similarity(chunk)
            if not _dist.single():
                keys = list(self.Ds.keys())
                local = np.stack([np.asarray(self.Ds[s][mine[:, 0], mine[:, 1]]) for s in keys], axis=1)
                full = _dist.gather_scores(local, len(pairs))
                if rank == 0:
                    for c, s in enumerate(keys):
                        self.Ds[s][pairs[:, 0], pairs[:, 1]] = full[:, c]
            if symmetric and rank == 0:
                for s in self.Ds:
                    self.Ds[s] += self.Ds[s].T
        # (a collective decision: a rank whose labels were injected must not skip the broadcast the others wait in)
        if _dist.any_rank(not self.cliques):
            self.get_all_clique_ids()
        if rank == 0:
            self._save_results_cache(npz, h5)

    # a result set up to this size is cached in BOTH formats (the .npz needs no HDF5 library to read back); above it only in
    # the reference's own -- at 15 000 tracks a second copy costs seconds per plane inside all_pairwise
    NPZ_CACHE_BELOW = 256 << 20

    def _save_results_cache(self, npz, h5):
        """The reference's dd.io.save("<prefix>_Ds.h5", self.Ds) (algorithm_template.py:192): <prefix>_Ds.h5 when an HDF5
        backend exists, <prefix>_Ds.npz when none does or the matrices are small; `all_pairwise(precomputed=True)` reads
        whichever is there (a stale .npz of an earlier, smaller run is removed so that it cannot shadow the new .h5)."""
        wrote_h5 = save_matrices_h5(h5, self.Ds)
        total = sum(int(np.asarray(self.Ds[s]).nbytes) for s in self.Ds)
        if not wrote_h5 or total <= self.NPZ_CACHE_BELOW:
            np.savez(npz, **{s: np.asarray(self.Ds[s]) for s in self.Ds})
        elif os.path.exists(npz):
            os.remove(npz)

    def _joblib_fanout(self, chunks, n_cores):
        """User subclasses with their own CPU `similarity()` (README "how to add an algorithm"): `parallel=1` fans the 45
        chunks out over joblib worker processes like the reference does (algorithm_template.py:172-177) -- every worker
        gets a pickled copy of `self` whose `Ds` memmaps joblib re-opens on the same files, so the scores land in the
        owner's matrices.  Returns False (caller runs the chunks serially) when joblib is missing or a matrix is not
        file-backed.  Device-backed classes never come here: their fan-out unit is the GPU."""
        try:
            from joblib import Parallel, delayed
        except ImportError:
            return False
        if not all(isinstance(D, np.memmap) for D in self.Ds.values()):
            return False
        for D in self.Ds.values():
            D.flush()
        Parallel(n_jobs=n_cores, verbose=0)(delayed(self.similarity)(c) for c in chunks)
        return True

    def _all_pairwise_grid(self, symmetric):
        """Device-backed classes: `self._grid()` -> (context with the pool uploaded, ACX_ALGO_*, params
        struct, similarity types in plane order).  One GPU: acx_pair_grid straight into the memmaps.
        N GPUs: every rank runs its tiles into a device buffer, one gather to rank 0, rank 0 scatters."""
        ctx, algo, params, keys = self._grid()
        planes = [self.Ds[k] for k in keys]
        rank, ws = _dist.world()
        if _dist.single():
            ctx.pair_grid(algo, symmetric, params, planes, mirror=symmetric)
            return
        import torch
        # torch's collectives (and its allocator) must work on the GPU libacx works on: one process, one GPU
        if ctx.torch_device().type == "cuda":
            _dist.bind_device(ctx.device)
        lengths = ctx.pool_lengths(algo)
        plan = _lib.grid_plan(lengths, algo, symmetric, world=ws)
        stride = int(max(1, plan["floats_per_rank"].max()))
        # (torch.empty launches nothing: libacx works on its own stream and zeroes what it owns)
        local = torch.empty(stride, dtype=torch.float32, device=ctx.torch_device())
        ctx.grid_run(plan["spec"], params, rank, local.data_ptr())
        gathered = _dist.gather_tiles(local, stride)
        if rank == 0:
            _lib.grid_scatter(lengths, plan["spec"], gathered, stride, planes, mirror=symmetric)

    # ------------------------------------------------------------------ queries against the collection
    # What a device-backed class tells identify() / query_rows() about the sequence coverid.benchmark() runs for it:
    # the similarity types the device computes (the planes of _grid(), in plane order), the types that only exist as a
    # fusion of whole matrices, and the orientation all_pairwise is called with there.
    _identify_planes = ("main",)
    _identify_fused = ()
    _identify_symmetric = True
    # what rerank_fused() needs of a class with fused types: per fused type the device planes do_late_fusion hands to the
    # fusion, in ITS order (the sweep's in-place aliasing makes the order matter), and the transform from score to distance
    # (_lib.FUSED_*)
    _fused_planes = {}
    _fused_transform = None

    # the open appended() session (an AppendedSession), None outside one
    _session = None

    def _n_tracks(self):
        """How many tracks may an index name right now: N, and N + Q inside an appended() session.  Every index check of
        the read-only methods takes its bound from here; `self.N` is the collection's count throughout."""
        return self.N if self._session is None else self._session.total

    def _identify_norm(self):
        """(col_mode, col) of the class's normalize_by_length as acx_query_spec states it (include/acx.h): (0, None) for
        a class without one.  col holds the collection's N values; _query_call adds a session's tail."""
        return 0, None

    def _query_setup(self, who, queries, similarity_types):
        """Argument checks of identify() / query_rows(), all before the first library call (no pool is uploaded, no GPU
        is touched, for a call that cannot run): -> (queries int32 (Q,), the similarity types asked for)."""
        if not hasattr(self, "_grid"):
            raise NotImplementedError("%s: %s has no device path (_grid()); a class that brings its own CPU similarity() "
                                      "answers queries through similarity(idxs) and top_matches()" % (who, type(self).__name__))
        types = list(self._identify_planes) if similarity_types is None else list(similarity_types)
        for t in types:
            if t in self._identify_fused:
                raise NotImplementedError("%s: '%s' is a fusion of whole N x N matrices (do_late_fusion) and cannot be "
                                          "computed for a band of query rows; rerank_fused() fuses it within a query's shortlist" % (who, t))
            if t not in self._identify_planes:
                raise ValueError("%s: unknown similarity type '%s' (available: %s)" % (who, t, list(self._identify_planes)))
        q = np.asarray(queries)
        if q.size and not np.issubdtype(q.dtype, np.integer):
            raise ValueError("%s: queries must be integer track indices" % who)
        q = q.reshape(-1).astype(np.int64)
        if q.size and (q.min() < 0 or q.max() >= self._n_tracks()):
            raise ValueError("%s: queries must be track indices in [0, %d)" % (who, self._n_tracks()))
        return q.astype(np.int32), types

    def _check_candidates(self, who, candidates, what):
        """The candidates of identify() / identify_tracks(): None, or strictly ascending track indices in [0, N) as int32."""
        if candidates is None:
            return None
        cands = np.asarray(candidates)
        if cands.size and not np.issubdtype(cands.dtype, np.integer):
            raise ValueError("%s: candidates must be integer track indices" % who)
        cands = cands.reshape(-1).astype(np.int64)
        if cands.size and (cands.min() < 0 or cands.max() >= self._n_tracks()):
            raise ValueError("%s: candidates must be %s in [0, %d)" % (who, what, self._n_tracks()))
        if np.any(np.diff(cands) <= 0):
            raise ValueError("%s: candidates must be strictly ascending" % who)
        return cands.astype(np.int32)

    def _query_call(self):
        ctx, algo, params, keys = self._grid()
        if tuple(keys) != tuple(self._identify_planes):
            raise RuntimeError("%s: _grid() planes %s differ from _identify_planes %s" % (type(self).__name__, keys, self._identify_planes))
        mode, col = self._identify_norm()
        if col is not None and self._session is not None:
            col = np.concatenate([np.asarray(col, np.float64).reshape(-1), np.asarray(self._session.col_tail, np.float64).reshape(-1)])
        return ctx, algo, params, mode, col

    def identify(self, queries, k=10, candidates=None, similarity_types=None):
        """Which k tracks of the collection are the covers of these tracks?  queries: track indices (any order,
        duplicates allowed); candidates: the tracks that may be listed -- any integer sequence, flattened; it must then
        be strictly ascending (None: every track).  Returns {type: (idx (Q, k) int32, score (Q, k) float32)} for the
        similarity types the device computes (similarity_types: a subset, None: all): values and order are those of
        coverid.benchmark()'s sequence for the class -- all_pairwise(...), normalize_by_length() where the class has
        one (ChenFusion: with the sign flip of do_late_fusion, larger = closer), top_matches(type, k, rows=queries) --
        but only the Q rows are computed (acx_query_topk): the scores stay on the device, are normalised and ranked
        there, and `Ds` is not written.  A query never lists itself; fewer than k candidates: the tail is -1 / NaN.
        Fused types need the whole matrix: NotImplementedError.  Not a collective: under a process group every rank
        that calls it computes on its own GPU."""
        q, types = self._query_setup("identify", queries, similarity_types)
        k = self._check_k("identify", k)
        cands = self._check_candidates("identify", candidates, "track indices")
        ctx, algo, params, mode, col = self._query_call()
        idx, score = ctx.query_topk(algo, self._identify_symmetric, params, q, k, candidates=cands, col=col, col_mode=mode)
        return self._by_type(idx, score, types)

    def query_rows(self, queries, similarity_types=None):
        """The same rows in full: {type: (Q, N) float32}, the finished scores of every query against every track (its
        own cell 0), as identify() ranks them (acx_query_scores).  `Ds` is not written."""
        q, types = self._query_setup("query_rows", queries, similarity_types)
        ctx, algo, params, mode, col = self._query_call()
        rows = ctx.query_scores(algo, self._identify_symmetric, params, q, col=col, col_mode=mode)
        planes = list(self._identify_planes)
        return {t: rows[planes.index(t)] for t in types}

    # ------------------------------------------------------------------ tracks the collection does not hold
    def _check_tracks(self, who, tracks, **how):
        """Per class: the tracks of identify_tracks() / score_tracks() in the format of the class's injection method,
        checked and converted WITHOUT touching the library (ValueError for a wrong shape or dtype).  `how`: the class's
        own options of that format (Serra09: raw).  Returns what _append_tracks takes, whatever the class needs there."""
        raise NotImplementedError("%s: %s has no append path (_check_tracks / _append_tracks)" % (who, type(self).__name__))

    def _append_tracks(self, ctx, checked):
        """Per class: put what _check_tracks returned behind the uploaded pool (Context.*_append*) and return what
        _identify_norm needs for the new columns: its `col` values for them, or None for a class without a norm."""
        raise NotImplementedError

    def _tracks_setup(self, who, tracks, similarity_types, candidates, how):
        """Argument checks of identify_tracks() / score_tracks(), all before the first library call:
        -> (what _check_tracks returned, the number of tracks, the similarity types, the candidates)."""
        _, types = self._query_setup(who, [], similarity_types)
        try:
            tracks = list(tracks)
        except TypeError:
            raise ValueError("%s: tracks must be a list of tracks" % who)
        if not tracks:
            raise ValueError("%s: tracks must hold at least one track" % who)
        checked = self._check_tracks(who, tracks, **how)
        return checked, len(tracks), types, self._check_candidates(who, candidates, "tracks of the collection, indices")

    def _append_session(self, ctx, checked, s):
        """Entering a session: the one append.  A class with more per-track side data than _identify_norm's column (Serra09:
        the pooled lengths) overrides this and keeps the tail on the session object."""
        s.col_tail = self._append_tracks(ctx, checked)

    @contextlib.contextmanager
    def _appended(self, checked, Q, labels=None):
        """The session itself, for tracks that _check_tracks has passed: one append on the way in, one pool_truncate(algo, N)
        on the way out -- after the block, after an exception in it and after a library error alike."""
        if self._session is not None:
            raise RuntimeError("appended: a session is already open on this object (sessions do not nest)")
        ctx, algo = self._query_call()[:2]              # (uploads the collection's pool first where that has not happened)
        N = self.N
        s = AppendedSession(N, Q, labels)
        try:
            self._append_session(ctx, checked, s)
            self._session = s
            yield s
        finally:
            self._session = None
            ctx.pool_truncate(algo, N)

    def _session_setup(self, who, tracks, labels, how):
        """Argument checks of appended() and the one-call forms, all before the first library call:
        -> (what _check_tracks returned, the number of tracks, the labels as a list or None)."""
        if self._session is not None:
            raise RuntimeError("%s: a session is already open on this object (sessions do not nest)" % who)
        checked, Q, _, _ = self._tracks_setup(who, tracks, None, None, how)
        if labels is not None:
            try:
                labels = list(labels)
            except TypeError:
                raise ValueError("%s: labels must be a sequence of one clique label per track" % who)
            if len(labels) != Q:
                raise ValueError("%s: labels must hold one clique label per track (%d), got %d" % (who, Q, len(labels)))
        return checked, Q, labels

    def appended(self, tracks, labels=None, **how):
        """A session over tracks the collection does NOT hold: `with algo.appended(tracks) as s:` appends them behind the
        uploaded pool ONCE (tracks and `how` as identify_tracks() takes them: Serra09 / ChenFusion raw=True), keeps them
        there while the block runs, and takes them away again when it ends -- on a normal exit, on an exception raised in
        the block (it propagates) and on a library error alike.  s: an AppendedSession -- s.indices = arange(N, N + Q)
        int32, s.first == N, s.count == Q, s.total == N + Q.
        Inside the block every read-only, index-taking method of the class treats the collection as the N + Q tracks:
        identify, query_rows, rerank, evaluate, align, align_paths, align_matches, align_match_paths (with the class's
        similarity_type), Simple.profile, EarlyFusion.full_fusion / rerank_full accept indices in [0, N + Q) wherever they
        accept [0, N) outside -- queries, candidates, shortlists, pairs -- and return, bit for bit, what the same call
        returns on an object built over the N + Q tracks in one upload.  `algo.N` keeps reading N; s.total is the other
        number.  labels: Q clique labels for the new tracks, used by evaluate() only: the mates of a query are all tracks
        of the N + Q with its label; without labels evaluate() raises a ValueError.
        Refused inside the block with a RuntimeError naming the method, before any library call: what writes `Ds` or assumes
        an N x N result (similarity, all_pairwise, normalize_by_length, do_late_fusion, getEvalStatistics, top_matches),
        what changes the pool or the feature caches (set_pooled_features / set_features / set_block_features,
        identify_tracks, score_tracks, rerank_tracks, the one-call forms) and a nested appended().
        Afterwards `Ds`, N, filepaths, the cliques, the cached features, the pooled lengths and the pool are exactly as
        before.  Every argument check comes before the first library call.  Not a collective: under a process group each
        rank that opens a session works on its own GPU."""
        checked, Q, labels = self._session_setup("appended", tracks, labels, how)
        return self._appended(checked, Q, labels)

    def _with_appended(self, checked, Q, call):
        """call(ctx, algo, params, mode, col, queries) with the Q tracks behind the collection's pool as tracks N .. N + Q - 1;
        whatever happens, the pool holds the N tracks of the collection again afterwards."""
        with self._appended(checked, Q) as s:
            ctx, algo, params, mode, col = self._query_call()
            return call(ctx, algo, params, mode, col, s.indices)

    def _cliques_now(self):
        """The cliques as lists of sorted track indices: the collection's, and inside a session (opened with labels) the same
        cliques extended by them -- a new label opens a clique behind the collection's, in the order of the new tracks, as
        _register_label would over the N + Q tracks.  `self.cliques` is not touched."""
        s = self._session
        if s is None:
            return [sorted(self.cliques[c]) for c in self.cliques]
        cliques = {c: set(m) for c, m in self.cliques.items()}
        for i, label in zip(s.indices, s.labels):
            cliques.setdefault(label, set()).add(int(i))
        return [sorted(cliques[c]) for c in cliques]

    # ------------------------------------------------------------------ one-call forms: one append, one question
    # what locate_tracks() aligns by when similarity_type is None (None here: the class's first device plane), and whether the
    # listed score of identify() belongs to the pair (hit, new track) -- a symmetric class whose alignment of the transposed pair
    # can score differently (EarlyFusion)
    _locate_type = None
    _locate_hit_first = False

    def _align_kw(self, who, similarity_type):
        """Per class with align_matches(): similarity_type checked (the class's own errors, before any library call) ->
        the keywords its align methods take."""
        raise NotImplementedError("%s: %s has no alignment (align_matches)" % (who, type(self).__name__))

    def _align_tracks_setup(self, who, tracks, indices, similarity_type, how, paths):
        kw = self._align_kw(who, similarity_type)
        if paths and not hasattr(self, "align_match_paths"):
            raise NotImplementedError("%s: %s returns no alignment paths" % (who, type(self).__name__))
        checked, Q, _ = self._session_setup(who, tracks, None, how)
        _align.check_matches(who, np.arange(self.N, self.N + Q), _align.check_indices(who, indices), self.N + Q)
        return kw, checked, Q

    def align_tracks(self, tracks, indices, similarity_type=None, **how):
        """align_matches() for tracks the collection does NOT hold, in ONE append: tracks (and how: Serra09 / ChenFusion
        raw=True) as identify_tracks() takes them, indices the (Q, k) array identify_tracks() / rerank_tracks() returned
        for them (-1: an empty slot).  Row i, slot s is the alignment of the ORDERED pair (new track i, indices[i, s]):
        exactly align_matches(s.indices, indices) inside `with self.appended(tracks) as s`.  similarity_type: ChenFusion
        ('qmax', the default, or 'dmax') and EarlyFusion ('early' by default); for EarlyFusion read align_matches() on which
        pair a listed score belongs to -- locate_tracks() aligns that one."""
        kw, checked, Q = self._align_tracks_setup("align_tracks", tracks, indices, similarity_type, how, False)
        with self._appended(checked, Q) as s:
            return self.align_matches(s.indices, indices, **kw)

    def align_track_paths(self, tracks, indices, similarity_type=None, **how):
        """align_tracks() with the paths: exactly align_match_paths(s.indices, indices) inside a session."""
        kw, checked, Q = self._align_tracks_setup("align_track_paths", tracks, indices, similarity_type, how, True)
        with self._appended(checked, Q) as s:
            return self.align_match_paths(s.indices, indices, **kw)

    def locate_tracks(self, tracks, k=10, candidates=None, similarity_type=None, paths=False, **how):
        """WHICH tracks of the collection are the covers of these new tracks, and WHERE do they match -- identify_tracks()
        and align_tracks() in ONE append.  Returns (idx (Q, k) int32, score (Q, k) float32, al (Q, k) records) or, with
        paths=True, (idx, score, al, paths) for ONE similarity type: the class's first device plane by default (ChenFusion
        'qmax', Serra09 / SiMPle 'main'), EarlyFusion 'early'; a fused type has no alignment: ValueError.  candidates: as in
        identify_tracks(), [0, N) by default.  idx / score are identify_tracks(tracks, k, candidates, [similarity_type])'s;
        al (and paths) are align_tracks(tracks, idx, similarity_type)'s (align_track_paths'): row i, slot s is the ordered
        pair (new track i, idx[i, s]), an empty slot a no-match row.
        EarlyFusion alone differs: identify() of that symmetric class lists the score of the cell (min, max) of the two
        indices, and the alignment of the transposed pair may score differently, so locate_tracks() aligns the pair the
        listed score belongs to, (hit, new track) = (idx[i, s], N + i): in al and paths the QUERY side (q0, q1, q_span, path
        column 0) is the hit and the REFERENCE side the new track, and al['score'] has the bits of score."""
        who = "locate_tracks"
        k = self._check_k(who, k)
        t = (self._locate_type or self._identify_planes[0]) if similarity_type is None else similarity_type
        kw = self._align_kw(who, t)
        if paths and not hasattr(self, "align_match_paths"):
            raise NotImplementedError("%s: %s returns no alignment paths" % (who, type(self).__name__))
        checked, Q, _ = self._session_setup(who, tracks, None, how)
        self._query_setup(who, [], [t])
        cands = self._check_candidates(who, candidates, "tracks of the collection, indices")
        if cands is None:
            cands = np.arange(self.N, dtype=np.int32)
        with self._appended(checked, Q) as s:
            idx, score = self.identify(s.indices, k=k, candidates=cands, similarity_types=[t])[t]
            if not self._locate_hit_first:
                got = self.align_match_paths(s.indices, idx, **kw) if paths else (self.align_matches(s.indices, idx, **kw),)
                return (idx, score) + tuple(got)
            rows, slots = np.nonzero(idx >= 0)
            pairs = np.stack([idx[rows, slots], s.indices[rows]], axis=1)
            al = self._no_match_rows(idx.shape)
            if not paths:
                al[rows, slots] = self.align(pairs, **kw)
                return idx, score, al
            al[rows, slots], got = self.align_paths(pairs, **kw)
            return idx, score, al, _align.scatter_paths(idx, rows, slots, got)

    @refused_in_session
    def identify_tracks(self, tracks, k=10, candidates=None, similarity_types=None):
        """identify() for tracks the collection does NOT hold.  tracks: a list in the format of the class's injection
        method (Serra09 / ChenFusion: pooled (T, 12) f32 chroma, or with raw=True raw (T0, 12) chroma, pooled by
        downsample_fac on the device, on the host by pool_median above 64; SiMPle: (12, n) f64; EarlyFusion: block-feature
        dicts; FTM2D: (12 WIN,) shingles).  They are appended behind the uploaded
        pool (O(Q) work: the collection is not uploaded again), asked about as queries N .. N + Q - 1 against the
        candidates [0, N) -- or `candidates`, strictly ascending indices in [0, N) --, and taken away again: `Ds`, N,
        the cliques and the pool are as before.  Returns what identify() returns; the values are those of
        identify(queries=[N ..], candidates=range(N)) on a collection of the N + Q tracks: a symmetric class computes a
        cell as the pair (candidate, new track), SiMPle as (new track, candidate)."""
        return self._identify_tracks(tracks, k, candidates, similarity_types)

    def _identify_tracks(self, tracks, k, candidates, similarity_types, **how):
        """identify_tracks(); how: the options of the class's own track format, handed to its _check_tracks."""
        k = self._check_k("identify_tracks", k)
        checked, Q, types, cands = self._tracks_setup("identify_tracks", tracks, similarity_types, candidates, how)
        if cands is None:
            cands = np.arange(self.N, dtype=np.int32)
        idx, score = self._with_appended(checked, Q, lambda ctx, algo, params, mode, col, q: ctx.query_topk(
            algo, self._identify_symmetric, params, q, k, candidates=cands, col=col, col_mode=mode))
        return self._by_type(idx, score, types)

    @refused_in_session
    def score_tracks(self, tracks, similarity_types=None):
        """query_rows() for tracks the collection does not hold: {type: (Q, N) float32}, the finished scores of every new
        track against every track of the collection, as identify_tracks() ranks them."""
        return self._score_tracks(tracks, similarity_types)

    def _score_tracks(self, tracks, similarity_types, **how):
        checked, Q, types, _ = self._tracks_setup("score_tracks", tracks, similarity_types, None, how)
        N = self.N
        rows = self._with_appended(checked, Q, lambda ctx, algo, params, mode, col, q: ctx.query_scores(
            algo, self._identify_symmetric, params, q, col=col, col_mode=mode))
        planes = list(self._identify_planes)
        return {t: np.ascontiguousarray(rows[planes.index(t)][:, :N]) for t in types}

    # ------------------------------------------------------------------ reranking: a shortlist per query
    def _check_shortlists(self, who, shortlists, Q):
        """The shortlists of rerank() / rerank_tracks() without touching the library: a (Q, L) integer array, or a
        sequence of Q integer sequences of any lengths -- padded with -1 behind their last entry --, every entry a track
        of the collection in [0, N) or -1 (an empty slot), no track twice in a row.  -> (Q, L) int32."""
        lists = shortlists_to_array(who, shortlists)
        if lists.shape[0] != Q:
            raise ValueError("%s: shortlists must hold one row per query (%d), got %d" % (who, Q, lists.shape[0]))
        if lists.size and (lists.min() < -1 or lists.max() >= self._n_tracks()):
            raise ValueError("%s: shortlist entries must be track indices in [0, %d) or -1" % (who, self._n_tracks()))
        srt = np.sort(lists, axis=1)
        dup = (srt[:, 1:] == srt[:, :-1]) & (srt[:, 1:] >= 0)
        if dup.any():
            r, j = np.argwhere(dup)[0]
            raise ValueError("%s: shortlists row %d lists track %d twice" % (who, r, srt[r, j + 1]))
        return lists.astype(np.int32)

    @staticmethod
    def _check_k(who, k):
        k = int(k)
        if k < 1:
            raise ValueError("%s: k must be >= 1 (got %d)" % (who, k))
        return k

    def _by_type(self, idx, score, types):
        planes = list(self._identify_planes)
        return {t: (np.ascontiguousarray(idx[:, planes.index(t)]), np.ascontiguousarray(score[:, planes.index(t)])) for t in types}

    def rerank(self, queries, shortlists, k=10, similarity_types=None):
        """identify() with a shortlist PER QUERY: the second stage of a cascade, whose first stage (a cheap index) left
        every query a few hundred candidates.  shortlists: a (Q, L) integer array, or a sequence of Q integer sequences
        of any lengths (padded with -1); an entry is a track index or -1, an empty slot; the order within a row is free,
        no track twice in a row; a query's own track is skipped.  Returns what identify() returns, and row i holds
        exactly identify([queries[i]], k, candidates=sorted(valid entries of shortlists[i])): only the Q x L listed cells
        are computed (acx_query_topk_lists), in bands that are not limited to 128 rows.  `Ds` is not written.  Not a
        collective."""
        q, types = self._query_setup("rerank", queries, similarity_types)
        k = self._check_k("rerank", k)
        lists = self._check_shortlists("rerank", shortlists, len(q))
        ctx, algo, params, mode, col = self._query_call()
        idx, score = ctx.query_topk_lists(algo, self._identify_symmetric, params, q, lists, k, col=col, col_mode=mode)
        return self._by_type(idx, score, types)

    # ------------------------------------------------------------------ fused scores within a query's shortlist
    def _fused_setup(self, who, similarity_types, K, niters):
        """The fused types, K and niters of rerank_fused() and its relatives, checked without touching the library."""
        if not self._identify_fused:
            raise NotImplementedError("%s: %s has no fused similarity type (no do_late_fusion)" % (who, type(self).__name__))
        types = list(self._identify_fused) if similarity_types is None else list(similarity_types)
        if not types:
            raise ValueError("%s: similarity_types must name at least one fused type of %s" % (who, list(self._identify_fused)))
        for t in types:
            if t in self._identify_planes:
                raise ValueError("%s: '%s' is not a fused type (rerank() lists it); fused types: %s" % (who, t, list(self._identify_fused)))
            if t not in self._identify_fused:
                raise ValueError("%s: unknown similarity type '%s' (fused types: %s)" % (who, t, list(self._identify_fused)))
        if len(set(types)) != len(types):
            raise ValueError("%s: similarity_types names a fused type twice" % who)
        K, niters = int(K), int(niters)
        if K < 1:
            raise ValueError("%s: K must be >= 1 (got %d)" % (who, K))
        if K > 64:
            raise NotImplementedError("%s: more than 64 neighbours are not supported on the device (K = %d)" % (who, K))
        if niters < 1:
            raise ValueError("%s: niters must be >= 1 (got %d)" % (who, niters))
        return types, K, niters

    @staticmethod
    def _check_fused_lists(who, q, lists, K):
        """Every neighbourhood -- the query and the valid entries of its row -- holds at least K + 2 tracks (below that the
        K-neighbour cut of the fusion is not defined), and a row at most 1024 entries."""
        if lists.shape[1] > 1024:
            raise NotImplementedError("%s: shortlists of more than 1024 entries are not supported (got %d)" % (who, lists.shape[1]))
        n = 1 + ((lists >= 0) & (lists != np.asarray(q).reshape(-1, 1))).sum(axis=1)
        bad = np.nonzero(n < K + 2)[0]
        if len(bad):
            raise ValueError("%s: shortlists row %d gives a neighbourhood of %d tracks (the query included); the fusion needs at "
                             "least K + 2 = %d" % (who, bad[0], n[bad[0]], K + 2))

    def _fused_call(self, ctx, algo, params, mode, col, q, lists, k, types, K, niters):
        planes = list(self._identify_planes)
        spec = _lib.fused_spec([[planes.index(p) for p in self._fused_planes[t]] for t in types], self._fused_transform, K=K, niters=niters)
        idx, score, _ = ctx.query_fused_lists(algo, self._identify_symmetric, params, q, lists, k, spec, col=col, col_mode=mode)
        return {t: (np.ascontiguousarray(idx[:, i]), np.ascontiguousarray(score[:, i])) for i, t in enumerate(types)}

    def rerank_fused(self, queries, shortlists, k=10, similarity_types=None, K=20, niters=20):
        """rerank() for the class's FUSED similarity types (ChenFusion 'Late', EarlyFusion 'late' / 'early+late'; None: all
        of them): {type: (idx (Q, k) int32, score (Q, k) float32)}.  Similarity network fusion is a function of a set of
        tracks, so the fused score of a query is defined on its neighbourhood T = sorted({query} U valid shortlist entries):
        row i holds exactly what the class computes on a collection of only those tracks -- all_pairwise(symmetric=True),
        normalize_by_length() where the class has one, do_late_fusion() (K, niters: its constants by default),
        top_matches(type, k, rows=[position of the query]) -- with the indices mapped back through T (acx_query_fused_lists:
        the same bits).  shortlists as rerank() takes them.  A neighbourhood needs at least K + 2 tracks (ValueError naming
        the row).  A query costs n (n - 1) / 2 alignments, n = len(T) -- 5 050 for a shortlist of 100, 1 275 for 50 -- where
        rerank() costs len(shortlist); a pair two neighbourhoods share is computed twice.  A ChenFusion pair with raw score 0
        (an empty plot) makes the rows of the neighbourhoods that hold it NaN, as it does in the whole-collection fusion.
        `Ds` is not written.  Not a collective."""
        who = "rerank_fused"
        types, K, niters = self._fused_setup(who, similarity_types, K, niters)
        q, _ = self._query_setup(who, queries, [])
        k = self._check_k(who, k)
        lists = self._check_shortlists(who, shortlists, len(q))
        self._check_fused_lists(who, q, lists, K)
        ctx, algo, params, mode, col = self._query_call()
        return self._fused_call(ctx, algo, params, mode, col, q, lists, k, types, K, niters)

    @refused_in_session
    def rerank_tracks_fused(self, tracks, shortlists, k=10, similarity_types=None, K=20, niters=20):
        """rerank_fused() for tracks the collection does NOT hold (tracks as identify_tracks() takes them, shortlist entries
        in [0, N) or -1): exactly rerank_fused(s.indices, shortlists, ...) inside `with self.appended(tracks) as s`."""
        return self._rerank_tracks_fused(tracks, shortlists, k, similarity_types, K, niters)

    def _rerank_tracks_fused(self, tracks, shortlists, k, similarity_types, K, niters, **how):
        who = "rerank_tracks_fused"
        types, K, niters = self._fused_setup(who, similarity_types, K, niters)
        k = self._check_k(who, k)
        checked, Q, _, _ = self._tracks_setup(who, tracks, [], None, how)
        lists = self._check_shortlists(who, shortlists, Q)
        self._check_fused_lists(who, np.arange(self.N, self.N + Q), lists, K)
        return self._with_appended(checked, Q, lambda ctx, algo, params, mode, col, q: self._fused_call(
            ctx, algo, params, mode, col, q, lists, k, types, K, niters))

    def identify_cascade(self, first, queries, k=10, shortlist=200, first_type=None, similarity_types=None):
        """Two stages: `first` -- another device-backed algorithm object over the SAME collection, the cheap one (FTM2D) --
        shortlists `shortlist` (1 .. 1024) tracks per query by its similarity type `first_type` (None: its first plane),
        and this object reranks them: self.rerank(queries, first.identify(queries, k=shortlist)[first_type][0], k).
        identify_cascade_fused() is the same cascade with rerank_fused() as its second stage."""
        if getattr(first, "N", None) != self.N:
            raise ValueError("identify_cascade: first holds %s tracks, this collection %d" % (getattr(first, "N", None), self.N))
        shortlist = int(shortlist)
        if shortlist < 1 or shortlist > 1024:
            raise ValueError("identify_cascade: shortlist must be in 1..1024 (got %d)" % shortlist)
        k = self._check_k("identify_cascade", k)
        q, _ = self._query_setup("identify_cascade", queries, similarity_types)
        first_type = first._identify_planes[0] if first_type is None else first_type
        first._query_setup("identify_cascade", q, [first_type])
        lists = first.identify(q, k=shortlist, similarity_types=[first_type])[first_type][0]
        return self.rerank(q, lists, k=k, similarity_types=similarity_types)

    def identify_cascade_fused(self, first, queries, k=10, shortlist=200, first_type=None, similarity_types=None, K=20, niters=20):
        """identify_cascade() with the class's FUSED types as the second stage: `first` shortlists `shortlist` (K + 1 .. 1024)
        tracks per query and this object fuses within every query's shortlist:
        self.rerank_fused(queries, first.identify(queries, k=shortlist)[first_type][0], k, similarity_types, K, niters)."""
        who = "identify_cascade_fused"
        if getattr(first, "N", None) != self.N:
            raise ValueError("%s: first holds %s tracks, this collection %d" % (who, getattr(first, "N", None), self.N))
        shortlist = int(shortlist)
        if shortlist < 1 or shortlist > 1024:
            raise ValueError("%s: shortlist must be in 1..1024 (got %d)" % (who, shortlist))
        k = self._check_k(who, k)
        types, K, niters = self._fused_setup(who, similarity_types, K, niters)
        if min(shortlist, self._n_tracks() - 1) < K + 1:
            raise ValueError("%s: a shortlist of %d of %d tracks gives neighbourhoods below K + 2 = %d tracks"
                             % (who, shortlist, self._n_tracks(), K + 2))
        q, _ = self._query_setup(who, queries, [])
        first_type = first._identify_planes[0] if first_type is None else first_type
        first._query_setup(who, q, [first_type])
        lists = first.identify(q, k=shortlist, similarity_types=[first_type])[first_type][0]
        return self.rerank_fused(q, lists, k=k, similarity_types=types, K=K, niters=niters)

    @refused_in_session
    def rerank_tracks(self, tracks, shortlists, k=10, similarity_types=None):
        """rerank() for tracks the collection does NOT hold (tracks as identify_tracks() takes them): they are appended
        behind the uploaded pool, asked about as queries N .. N + Q - 1 with their shortlists -- entries in [0, N) or
        -1 --, and taken away again; `Ds`, N, the cliques and the pool are as identify_tracks() leaves them."""
        return self._rerank_tracks(tracks, shortlists, k, similarity_types)

    def _rerank_tracks(self, tracks, shortlists, k, similarity_types, **how):
        k = self._check_k("rerank_tracks", k)
        checked, Q, types, _ = self._tracks_setup("rerank_tracks", tracks, similarity_types, None, how)
        lists = self._check_shortlists("rerank_tracks", shortlists, Q)
        idx, score = self._with_appended(checked, Q, lambda ctx, algo, params, mode, col, q: ctx.query_topk_lists(
            algo, self._identify_symmetric, params, q, lists, k, col=col, col_mode=mode))
        return self._by_type(idx, score, types)

    def evaluate(self, queries=None, similarity_types=None, topsidx=[1, 10, 100, 1000], report=False, info=None, row_block=1024):
        """MR, MRR, MDR, MAP and Top-k of a query set against the collection without an N x N matrix:
        {type: (MR, MRR, MDR, MAP, tops)} for the similarity types the device computes (similarity_types: a subset,
        None: all).  Values and orientation are identify()'s -- coverid.benchmark()'s sequence for the class, ChenFusion
        with its sign flip --, the tie order is getEvalStatistics': the clique-contiguous layout of rank_plan.  Only the
        rows of the queries that have a clique mate are computed, in bands (acx_query_ranks): the scores stay on the
        device, are normalised there, and the positions of every query's clique mates are counted there; only those
        integers come back.  `Ds` is not written.
        queries: distinct track indices in any order (duplicates: ValueError), None: every track -- then the result is
        all_pairwise(symmetric=...) + normalize_by_length() + getEvalStatistics(type, engine="device") bit for bit.
        With a subset MR, MDR, MAP and Top-k run over the queries that have at least one clique mate and MRR divides by
        the number of queries given (the reference's division by all songs, applied to the subset).  The cliques are
        `self.cliques`: every track must be labelled.  A (query, type) whose finished row holds NaN or -inf outside its
        own cell is ranked on the host by the sorting branch from query_rows(), a block of rows at a time.
        info: a dict that receives {type: {"device_rows", "host_rows"}}.  report=True prints and appends the lines
        getEvalStatistics writes.  Fused types need the whole matrix: NotImplementedError.  Not a collective: under a
        process group every rank that calls it computes on its own GPU."""
        n = self._n_tracks()
        q, types = self._query_setup("evaluate", np.arange(n) if queries is None else queries, similarity_types)
        if len(np.unique(q)) != len(q):
            raise ValueError("evaluate: queries must be distinct track indices")
        if self._session is not None and self._session.labels is None:
            raise ValueError("evaluate: the session was opened without labels; evaluate() needs a clique label for every "
                             "appended track (appended(tracks, labels=...))")
        if not self.cliques and _dist.single():
            self.get_all_clique_ids()
        plan = evaluate_plan(self._cliques_now(), n, None if queries is None else q)
        ctx, algo, params, mode, col = self._query_call()
        pos, flag = ctx.query_ranks(algo, self._identify_symmetric, params, plan["rows"], plan["moff"], plan["mates"],
                                    posn=plan["posn"], col=col, col_mode=mode)
        planes = list(self._identify_planes)
        out = {}
        for t in types:
            e = planes.index(t)
            inf = {}
            out[t] = _statistics_from_positions(None, plan, pos[e], flag[:, e], topsidx, row_block, inf,
                                                rows_of=lambda tracks, t=t: self.query_rows(tracks, [t])[t])
            if info is not None:
                info[t] = inf
            if report:
                self._report_statistics(t, topsidx, *out[t])
        return out

    def cleanup_memmap(self):
        """Remove the memmap files behind the similarity matrices."""
        for s in list(self.Ds.keys()):
            path = self._dmat_path(s)
            if isinstance(self.Ds[s], np.memmap):
                self.Ds[s].flush()
            try:
                if os.path.exists(path):
                    os.remove(path)
            except OSError:
                print("Could not clean-up automatically.")

    # ------------------------------------------------------------------ evaluation
    def _rank_context(self):
        """The libacx context that ranks finished score rows (getEvalStatistics(engine="device"), top_matches): the
        object's own if it has one already, else one created here on the object's device -- never through _grid():
        ranking a matrix must not trigger a pool upload, and user subclasses without any device code rank too.
        No GPU: _lib.Context raises AcxError; there is no host fallback."""
        ctx = getattr(self, "_ctx", None)
        if isinstance(ctx, _lib.Context) and getattr(ctx, "_h", None):
            return ctx
        if getattr(self, "_rank_ctx", None) is None or not self._rank_ctx._h:
            dev = getattr(self, "_device", None)
            if dev is None:
                dev = getattr(self, "device", None)
            self._rank_ctx = _lib.Context(int(os.environ.get("LOCAL_RANK", "0")) if dev is None else int(dev))
        return self._rank_ctx

    @refused_in_session
    def top_matches(self, similarity_type, k=10, rows=None):
        """The k best other tracks of every track (or of `rows`) by Ds[similarity_type], best first, ties in index order:
        (idx (R, k) int32, score (R, k) float32) = np.argsort(-row, kind="stable")[:k] with the track itself removed,
        computed on the device (acx_topk_rows).  Fewer than k other tracks: the tail is index -1, score NaN."""
        return self._rank_context().topk_rows(self.Ds[similarity_type], k, rows=rows)

    @refused_in_session
    def getEvalStatistics(self, similarity_type, topsidx=[1, 10, 100, 1000], engine=None):
        """MR, MRR, MDR, MAP and Top-k of one similarity matrix; appends a row to
        results_<shortname>_<name>.csv.  Same definitions as the reference (:205-290),
        including MRR's division by ALL N songs and the %.3g CSV format.
        engine: "host" (numpy), "device" (the rows are ranked by libacx on the GPU, eval_statistics_device; no GPU raises
        AcxError) or None = the class attribute `eval_engine` ("host").
        Under torch.distributed this is a COLLECTIVE: rank 0 (the owner of the matrices) evaluates and
        writes the CSV, the tuple is broadcast and returned on every rank -- so every rank must call it
        (`if rank == 0: algo.getEvalStatistics(...)` would leave rank 0 waiting in the broadcast)."""
        rank, ws = _dist.world()
        engine = self.eval_engine if engine is None else engine
        if engine not in ("host", "device"):
            raise ValueError("getEvalStatistics: engine must be 'host' or 'device', got %r" % (engine,))

        def evaluate():
            cliques = [sorted(self.cliques[s]) for s in self.cliques]
            if engine == "device":
                return eval_statistics_device(self.Ds[similarity_type], cliques, topsidx, ctx=self._rank_context())
            D = np.array(self.Ds[similarity_type], dtype=np.float32)
            return eval_statistics(D, cliques, topsidx)
        MR, MRR, MDR, MAP, tops = _dist.on_root(evaluate)
        if rank != 0:
            return MR, MRR, MDR, MAP, tops
        self._report_statistics(similarity_type, topsidx, MR, MRR, MDR, MAP, tops)
        return MR, MRR, MDR, MAP, tops

    def _report_statistics(self, similarity_type, topsidx, MR, MRR, MDR, MAP, tops):
        """The reference's report of one tuple (:270-290): the printed block and one line appended to
        results_<shortname>_<name>.csv (the header first when the file is new)."""
        print("%s %s STATS\n-------------------------\nMR = %.3g\nMRR = %.3g\nMDR = %.3g\nMAP = %.3g"
              % (self.name, similarity_type, MR, MRR, MDR, MAP))
        for t, v in zip(topsidx, tops):
            print("Top-%i: %i" % (t, v))
        resultsfile = "results_%s_%s.csv" % (self.shortname, self.name)
        if not os.path.exists(resultsfile):
            with open(resultsfile, "w") as fout:
                fout.write("name, MR, MRR, MDR, MAP")
                for t in topsidx:
                    fout.write(",Top-%i" % t)
                fout.write("\n")
        with open(resultsfile, "a") as fout:
            fout.write("%s_%s," % (self.name, similarity_type))
            fout.write("%.3g, %.3g, %.3g, %.3g" % (MR, MRR, MDR, MAP))
            for t in tops:
                fout.write(", %.3g" % t)
            fout.write("\n")


def shortlists_to_array(who, shortlists):
    """The shortlists of rerank() as one (Q, L) int64 array: a 2-D integer array as it is; a sequence of Q integer
    sequences of any lengths with every row padded with -1 (an empty slot) to the longest, L = 0 when all are empty."""
    if isinstance(shortlists, np.ndarray):
        if shortlists.ndim != 2:
            raise ValueError("%s: a shortlist array must be (Q, L), got shape %s" % (who, shortlists.shape))
        if shortlists.size and not np.issubdtype(shortlists.dtype, np.integer):
            raise ValueError("%s: shortlists must hold integer track indices" % who)
        return shortlists.astype(np.int64)
    try:
        rows = [np.asarray(r) for r in shortlists]
    except TypeError:
        raise ValueError("%s: shortlists must be a (Q, L) array or a sequence of sequences" % who)
    for i, r in enumerate(rows):
        if r.ndim != 1:
            raise ValueError("%s: shortlists[%d] must be a flat sequence of track indices, got shape %s" % (who, i, r.shape))
        if r.size and not np.issubdtype(r.dtype, np.integer):
            raise ValueError("%s: shortlists must hold integer track indices (row %d)" % (who, i))
    out = np.full((len(rows), max([len(r) for r in rows], default=0)), -1, np.int64)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out


def _clique_order(cliques):
    """Cliques largest first (stable): (Ks sorted, idx = the tracks in that clique-contiguous order)."""
    Ks = np.array([len(c) for c in cliques])
    order = np.argsort(-Ks, kind="stable")
    Ks = Ks[order]
    cl = [list(cliques[i]) for i in order]
    idx = np.array([t for c in cl for t in c], dtype=np.int64)
    return Ks, idx


def _finish_counted(pos, Kb):
    """The tail of the counting branch for one block of rows: `pos` (rows, kmax) f64 holds the 1-based positions of every
    row's clique mates in any column order, +inf where there is none; Kb the rows' clique sizes.  Returns (rank of the
    first mate, average precision) per row.  Sorts `pos` in place."""
    kmax = pos.shape[1]
    pos.sort(axis=1)                                     # ascending; missing mates (+inf) last
    nm = (Kb - 1)[:, None]
    t = np.arange(1, kmax + 1, dtype=np.float64)[None, :]
    contrib = np.where(t <= nm, t / pos, 0.0)
    return pos[:, 0], contrib.sum(axis=1) / (Kb - 1)


def _rank_sorted(Db, row_start, row_K):
    """The sorting branch for one block of rows of the clique-ordered matrix (own cells -inf): (rank of the first mate,
    average precision) per row from a stable argsort; row_start / row_K: first column and size of every row's clique."""
    nb = Db.shape[0]
    srt = np.argsort(-Db, axis=1, kind="stable")
    member = (srt >= row_start[:, None]) & (srt < (row_start + row_K)[:, None])
    rr, kk = np.nonzero(member)              # row-major: per row, ascending rank position
    # the last member of every row is the song itself (-inf sorts last): drop it
    first = np.concatenate([[0], np.cumsum(row_K)])[:-1]
    last = first + row_K - 1
    keep = np.ones(len(rr), dtype=bool)
    keep[last] = False
    pos = (kk + 1)[keep].astype(np.float64)
    rows = rr[keep]
    within = np.arange(len(rr)) - np.repeat(first, row_K)
    num = (within + 1)[keep].astype(np.float64)
    ranks = pos[np.searchsorted(rows, np.arange(nb))]
    sums = np.bincount(rows, weights=num / pos, minlength=nb)
    return ranks, sums / (row_K - 1)


def _finish_statistics(ranks, allmap, N, n_eval, topsidx):
    """MR, MRR, MDR, MAP, Top-k from the per-row ranks / average precisions (NaN for rows that are not evaluated)."""
    if n_eval == 0:
        warnings.warn("no clique with at least two songs")
    MAP = float(np.nanmean(allmap)) if n_eval else float("nan")
    ranks = ranks[~np.isnan(ranks)]
    MR = float(np.mean(ranks)) if len(ranks) else float("nan")
    MRR = float(1.0 / N * np.sum(1.0 / ranks))
    MDR = float(np.median(ranks)) if len(ranks) else float("nan")
    tops = np.array([np.sum(ranks <= t) for t in topsidx], dtype=np.float64)
    return MR, MRR, MDR, MAP, tops


def rank_plan(cliques, N):
    """What eval_statistics_device asks the device for.  The cliques are laid out as eval_statistics does (largest first,
    stable); a track's place in that layout is its tie rank.  Returns a dict:
      idx     (N,) int64   the tracks in clique order;   Ks  clique sizes in that order;   n_eval  rows of cliques >= 2
      posn    (N,) int32   posn[track] = its place in idx (the tie order of every row)
      rows    (R,) int32   the tracks whose rows are ranked, ascending -- the evaluated tracks, or, when these cover at
                           least half of the span between the first and the last of them, the WHOLE span (a float32
                           matrix is then handed over as it lies in memory; the extra rows list no columns)
      moff    (R + 1,) int64, mates (moff[-1],) int32   the clique mates (track indices, clique order, own track left
                           out) of every row of `rows`
      where   (n_eval, 2) int64   for the e-th track of idx: first entry and number of its mates in `mates`."""
    Ks, idx = _clique_order(cliques)
    if len(idx) != N or not np.array_equal(np.sort(idx), np.arange(N)):
        raise ValueError("eval_statistics_device: the cliques must hold every track of the matrix exactly once")
    n_eval = int(np.sum(Ks[Ks >= 2]))
    posn = np.empty(N, np.int32)
    posn[idx] = np.arange(N, dtype=np.int32)
    starts = np.concatenate([[0], np.cumsum(Ks)])[:-1]
    row_start = np.repeat(starts, Ks)[:n_eval]
    row_K = np.repeat(Ks, Ks)[:n_eval]
    ev = np.sort(idx[:n_eval])
    if n_eval and 2 * n_eval >= int(ev[-1] - ev[0]) + 1:
        rows = np.arange(ev[0], ev[-1] + 1, dtype=np.int32)
    else:
        rows = ev.astype(np.int32)
    place = posn[rows].astype(np.int64)                     # a row's place in clique order (>= n_eval: lists nothing)
    ev_mask = place < n_eval
    pe = place[ev_mask]
    K = row_K[pe] if n_eval else np.zeros(0, np.int64)
    nmate = np.zeros(len(rows), np.int64)
    nmate[ev_mask] = K - 1
    moff = np.concatenate([[0], np.cumsum(nmate)]).astype(np.int64)
    # every evaluated row's clique as places in clique order, the row's own place dropped
    within = np.arange(int(K.sum())) - np.repeat(np.cumsum(K) - K, K)
    members = np.repeat(row_start[pe], K) + within if n_eval else np.zeros(0, np.int64)
    mates = idx[members[members != np.repeat(pe, K)]].astype(np.int32)
    where = np.zeros((n_eval, 2), np.int64)
    where[pe, 0] = moff[:-1][ev_mask]
    where[pe, 1] = nmate[ev_mask]
    return dict(idx=idx, Ks=Ks, n_eval=n_eval, posn=posn, rows=rows, moff=moff, mates=mates, where=where)


def evaluate_plan(cliques, N, queries=None):
    """rank_plan for a query set (CoverAlgorithm.evaluate): the same clique layout and tie order, but only the queries
    that have a clique mate are rows -- in clique order --, and no row is there only to keep a span whole.
    queries: distinct track indices, None: every track.  The dict of rank_plan, plus
      ev     (E,) int64   the places (in clique order, ascending) of the queries that are evaluated; rows = idx[ev]
      n_mrr  the number MRR divides by: the queries given (N for None)
    `where` stays indexed by place: rows outside `ev` list nothing."""
    base = rank_plan(cliques, N)
    idx, Ks, n_eval, posn = base["idx"], base["Ks"], base["n_eval"], base["posn"]
    if queries is None:
        ev = np.arange(n_eval, dtype=np.int64)
        n_mrr = N
    else:
        queries = np.asarray(queries, dtype=np.int64).reshape(-1)
        if len(np.unique(queries)) != len(queries):
            raise ValueError("evaluate: queries must be distinct track indices")
        if len(queries) and (queries.min() < 0 or queries.max() >= N):
            raise ValueError("evaluate: queries must be track indices in [0, %d)" % N)
        place = np.sort(posn[queries].astype(np.int64))
        ev = place[place < n_eval]
        n_mrr = len(queries)
    starts = np.concatenate([[0], np.cumsum(Ks)])[:-1]
    row_start = np.repeat(starts, Ks)[ev]
    K = np.repeat(Ks, Ks)[ev]
    nmate = K - 1
    moff = np.concatenate([[0], np.cumsum(nmate)]).astype(np.int64)
    within = np.arange(int(K.sum())) - np.repeat(np.cumsum(K) - K, K)
    members = np.repeat(row_start, K) + within
    mates = idx[members[members != np.repeat(ev, K)]].astype(np.int32)
    where = np.zeros((n_eval, 2), np.int64)
    where[ev, 0] = moff[:-1]
    where[ev, 1] = nmate
    return dict(idx=idx, Ks=Ks, n_eval=n_eval, posn=posn, rows=idx[ev].astype(np.int32), moff=moff, mates=mates, where=where,
                ev=ev, n_mrr=int(n_mrr))


def _statistics_from_positions(D, plan, pos, flag, topsidx, row_block, info=None, rows_of=None):
    """The statistics from the integer positions acx_rank_columns / acx_query_ranks returned for `plan` (rank_plan,
    evaluate_plan): block by block in clique order, exactly the host's counting branch with the production of `pos`
    replaced (same blocks, same padded width, same tail: numpy's row sums group their terms by that width).  Rows the
    device flagged (NaN / -inf) are ranked here by the sorting branch -- the reference's reading of such a row; their
    score rows come from rows_of(tracks) -> (len(tracks), N) (None: the rows of the matrix D).
    A plan with "ev" evaluates those places only (ascending, in clique order) and MRR divides by its "n_mrr"."""
    idx, Ks, n_eval, where = plan["idx"], plan["Ks"], plan["n_eval"], plan["where"]
    N = len(idx)
    ev = plan["ev"] if "ev" in plan else np.arange(n_eval)
    if rows_of is None:
        def rows_of(tracks):
            return np.asarray(D)[tracks]
    starts = np.concatenate([[0], np.cumsum(Ks)])[:-1]
    row_start = np.repeat(starts, Ks)
    row_K = np.repeat(Ks, Ks)
    ranks = np.full(N, np.nan)
    allmap = np.full(N, np.nan)
    flag_of_track = np.zeros(N, bool)
    flag_of_track[plan["rows"]] = flag.astype(bool)
    flagged = flag_of_track[idx[ev]]                        # in clique order
    for r0 in range(0, len(ev), row_block):
        pl = ev[r0:r0 + row_block]
        Kb = row_K[pl]
        kmax = int(Kb.max())
        P = np.full((len(pl), kmax), np.inf)
        cols = np.arange(kmax - 1)[None, :]
        have = cols < where[pl, 1][:, None]
        src = where[pl, 0][:, None] + cols
        P[:, :kmax - 1][have] = pos[src[have]]
        P[flagged[r0:r0 + row_block]] = np.inf
        ranks[pl], allmap[pl] = _finish_counted(P, Kb)
    host_rows = ev[flagged]
    for a in range(0, len(host_rows), row_block):
        hr = host_rows[a:a + row_block]
        Db = np.array(np.asarray(rows_of(idx[hr]))[:, idx], dtype=np.float32)
        Db[np.arange(len(hr)), hr] = -np.inf
        ranks[hr], allmap[hr] = _rank_sorted(Db, row_start[hr], row_K[hr])
    if info is not None:
        info["device_rows"] = int(len(ev) - len(host_rows))
        info["host_rows"] = int(len(host_rows))
    return _finish_statistics(ranks, allmap, plan.get("n_mrr", N), len(ev), topsidx)


def eval_statistics_device(D, cliques, topsidx=(1, 10, 100, 1000), ctx=None, info=None, row_block=1024):
    """eval_statistics with the rows ranked on the GPU: libacx counts the 1-based positions of every evaluated track's
    clique mates in the stable descending order of its score row (acx_rank_columns; tie order = the clique-contiguous
    layout eval_statistics uses, own cell ignored) and the host turns those integers into MR, MRR, MDR, MAP and Top-k
    with the code that finishes eval_statistics' counting branch -- the same numbers as
    eval_statistics(D, cliques, topsidx, count_max_clique=<huge>), bit for bit, on finite matrices.  Rows that hold NaN
    or -inf outside their own cell are flagged by the device and ranked here by the sorting branch.
    D: (N, N) scores, any dtype or strides (float32 rows are passed as they lie, a memmap included; anything else is
    converted a slab of rows at a time); ctx: a _lib.Context (None: one on device 0 for this call); info: a dict that
    receives {"device_rows", "host_rows"}.  No GPU: AcxError -- there is no host fallback."""
    N = int(D.shape[0])
    if len(D.shape) != 2 or D.shape[1] != N:
        raise ValueError("eval_statistics_device: D must be square")
    plan = rank_plan(cliques, N)
    own = ctx is None
    if own:
        ctx = _lib.Context(0)
    try:
        pos, flag = ctx.rank_columns(D, plan["rows"], plan["moff"], plan["mates"], posn=plan["posn"])
    finally:
        if own:
            ctx.close()
    return _statistics_from_positions(D, plan, pos, flag, topsidx, row_block, info)


def eval_statistics(D, cliques, topsidx=(1, 10, 100, 1000), row_block=1024, count_max_clique=24):
    """Vectorised evaluation.  `cliques`: list of lists of track indices (dict insertion
    order).  Rows are reordered so that cliques are contiguous, largest first; the
    diagonal is -inf; every row is ranked by descending score in STABLE order (ties: the lower
    index first); for every song of a clique of size >= 2 the 1-based ranks of its clique mates are
    collected -- by counting for cliques of up to `count_max_clique` songs, by a stable argsort
    otherwise (and for rows that hold NaN); both give the same numbers."""
    D = np.array(D, dtype=np.float32)
    N = D.shape[0]
    Ks, idx = _clique_order(cliques)
    D = D[idx, :][:, idx]
    np.fill_diagonal(D, -np.inf)
    starts = np.concatenate([[0], np.cumsum(Ks)])[:-1]
    row_start = np.repeat(starts, Ks)            # first column of the row's own clique
    row_K = np.repeat(Ks, Ks)
    n_eval = int(np.sum(Ks[Ks >= 2]))            # cliques are sorted: evaluated rows come first
    ranks = np.full(N, np.nan)
    allmap = np.full(N, np.nan)
    col = np.arange(N, dtype=np.int64)
    for r0 in range(0, n_eval, row_block):
        r1 = min(n_eval, r0 + row_block)
        Db = D[r0:r1]
        Kb = row_K[r0:r1]
        kmax = int(Kb.max())
        if kmax <= count_max_clique and not np.isnan(Db).any():
            # Ranks by COUNTING instead of sorting: only the positions of a row's clique mates are needed, and the
            # position of column c in the stable descending order is 1 + #(cells above D[i, c]) + #(equal cells left of
            # c).  2 (K - 1) passes over the block instead of an N log N sort per row (6 x faster at N = 15 000, K = 5).
            rows_i = np.arange(r0, r1)
            pos = np.full((r1 - r0, kmax), np.inf)
            for m in range(kmax):
                c = row_start[r0:r1] + m
                ok = (m < Kb) & (c != rows_i)
                if not ok.any():
                    continue
                cc = np.where(ok, c, 0)
                v = Db[np.arange(r1 - r0), cc][:, None]
                p = 1.0 + np.count_nonzero(Db > v, axis=1)
                eq = Db == v
                if np.count_nonzero(eq) > r1 - r0:               # ties beyond the cell itself: the left ones come first
                    p = p + np.count_nonzero(eq & (col[None, :] < cc[:, None]), axis=1)
                pos[ok, m] = p[ok]
            ranks[r0:r1], allmap[r0:r1] = _finish_counted(pos, Kb)
            continue
        ranks[r0:r1], allmap[r0:r1] = _rank_sorted(Db, row_start[r0:r1], row_K[r0:r1])
    return _finish_statistics(ranks, allmap, N, n_eval, topsidx)
