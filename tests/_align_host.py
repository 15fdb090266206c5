"""
What tests/test_align_classes_host.py shares: a temporary collection for Serra09 / ChenFusion / EarlyFusion, and a stand-in for the
class's libacx context that RECORDS every alignment call (its name and its arguments by name, whatever way they were passed) and
answers with canned records, paths and sections.  No library is loaded and no GPU is touched.
"""
import numpy as np

from acoss_amd import _lib

N, Q = 5, 2                                   # tracks of the collection, tracks a session appends
SERRA = ("Serra09", "ChenFusion")

NO_MATCH = (0.0, -1, -1, -1, -1)
# (score, q0, r0, q1, r1): HITS[1] ends beyond every track of the collection (its Serra09 span is clipped whatever tau and m),
# HITS[2] ends early (never clipped)
HITS = [(3.5, 2, 1, 20, 25), (7.25, 0, 5, 60, 70), (2.0, 4, 4, 6, 9)]
CYCLE = [HITS[0], NO_MATCH, HITS[1], HITS[2]]


def canned_records(K):
    """Pair k of a list call gets CYCLE[k % 4]: the second pair of every list has no match."""
    return np.array([CYCLE[k % 4] for k in range(K)], _lib.ALIGNMENT_DTYPE).reshape(K)


def canned_paths(al):
    """-> (offsets, cells): pair k's path has k + 1 cells from its start on, a pair without a match none."""
    paths = [np.stack([r["q0"] + np.arange(k + 1), r["r0"] + np.arange(k + 1)], axis=1) if r["q0"] >= 0 else np.zeros((0, 2), np.int64)
             for k, r in enumerate(al)]
    off = np.concatenate([[0], np.cumsum([len(p) for p in paths])]).astype(np.int64)
    return off, np.concatenate(paths + [np.zeros((0, 2), np.int64)], axis=0).astype(np.int32)


def canned_sections(K, S):
    """-> (records (K, S), counts (K,), offsets (K S + 1,), cells): pair k has min(S, k % 3) sections -- the first pair none --,
    section s of it is HITS[(k + s) % 3] with a path of s + 1 cells."""
    n = np.array([min(S, k % 3) for k in range(K)], np.int32)
    al = np.array([[HITS[(k + s) % 3] if s < n[k] else NO_MATCH for s in range(S)] for k in range(K)], _lib.ALIGNMENT_DTYPE).reshape(K, S)
    paths = [np.stack([al[k, s]["q0"] + np.arange(s + 1), al[k, s]["r0"] + np.arange(s + 1)], axis=1) if s < n[k] else np.zeros((0, 2), np.int64)
             for k in range(K) for s in range(S)]
    off = np.concatenate([[0], np.cumsum([len(p) for p in paths])]).astype(np.int64)
    return al, n, off, np.concatenate(paths + [np.zeros((0, 2), np.int64)], axis=0).astype(np.int32)


def _params(p):
    return dict(m=p.m, tau=p.tau, kappa=p.kappa, oti=p.oti, dmax=p.dmax)


def _opts(o):
    return dict(max_sections=o.max_sections, pad=o.pad, min_score=o.min_score, min_ratio=o.min_ratio)


class RecordingCtx(object):
    """Stands where the class's libacx context would be.  calls: [(method, {argument: value})] of the alignment methods, in order;
    session: ("append", n_new) / ("truncate", n_tracks); asked: how often ef_has_long_track was consulted (no library call).
    blocks: what Context.ef_blocks would hold (None: a pool this object did not see); long: ef_has_long_track's answer.
    The signatures are those of acoss_amd._lib.Context."""

    def __init__(self, blocks=None, long=False):
        self.calls, self.session, self.asked = [], [], 0
        self.ef_blocks, self.long = blocks, long

    def _note(self, name, pairs, **args):
        assert isinstance(pairs, np.ndarray) and pairs.dtype == np.int32 and pairs.ndim == 2 and pairs.shape[1] == 2 and pairs.flags.c_contiguous
        assert args.pop("cap", None) is None
        self.calls.append((name, dict(args, pairs=pairs.tolist())))
        return len(pairs)

    def _answer(self, K, paths):
        al = canned_records(K)
        return (al,) + canned_paths(al) if paths else al

    # ---- Serra09 / ChenFusion
    def serra09_align(self, pairs, params=None):
        return self._answer(self._note("serra09_align", pairs, params=_params(params)), False)

    def serra09_align_paths(self, pairs, params=None, cap=None):
        return self._answer(self._note("serra09_align_paths", pairs, params=_params(params), cap=cap), True)

    def chenfusion_align(self, pairs, params=None, plane=0):
        return self._answer(self._note("chenfusion_align", pairs, params=_params(params), plane=plane), False)

    def chenfusion_align_paths(self, pairs, params=None, plane=0, cap=None):
        return self._answer(self._note("chenfusion_align_paths", pairs, params=_params(params), plane=plane, cap=cap), True)

    def serra09_align_sections(self, pairs, params=None, opts=None, paths=False, cap=None):
        assert paths is True or paths is False
        K = self._note("serra09_align_sections", pairs, params=_params(params), opts=_opts(opts), paths=paths, cap=cap)
        return canned_sections(K, opts.max_sections)[:4 if paths else 2]

    # ---- EarlyFusion
    def ef_has_long_track(self, pairs):
        self.asked += 1
        return self.long

    def ef_align(self, pairs, kappa=0.1, K=10, plane=3, paths=False, cap=None):
        assert paths is True or paths is False
        return self._answer(self._note("ef_align", pairs, kappa=kappa, K=K, plane=plane, paths=paths, cap=cap), paths)

    def ef_align_long(self, pairs, kappa=0.1, K=10, plane=3, paths=False, cap=None):
        assert paths is True or paths is False
        return self._answer(self._note("ef_align_long", pairs, kappa=kappa, K=K, plane=plane, paths=paths, cap=cap), paths)

    def ef_align_sections(self, pairs, kappa=0.1, K=10, plane=3, opts=None, paths=False, cap=None):
        assert paths is True or paths is False
        P = self._note("ef_align_sections", pairs, kappa=kappa, K=K, plane=plane, opts=_opts(opts), paths=paths, cap=cap)
        return canned_sections(P, opts.max_sections)[:4 if paths else 2]

    # ---- sessions
    def pool_append(self, frames, offsets):
        self.session.append(("append", len(offsets) - 1))

    def ef_pool_append(self, tracks):
        self.session.append(("append", len(tracks)))

    def pool_truncate(self, algo, n_tracks):
        self.session.append(("truncate", int(n_tracks)))


def csv(tmp_path, n):
    path = tmp_path / "ds.csv"
    with open(path, "w") as f:
        f.write("work_id,track_id\n")
        for i in range(n):
            f.write("w%d,t%d\n" % (i // 2, i))
    return str(path)


def tracks(cls_name, n):
    """Serra09 / ChenFusion: pooled lengths 40, 43, 46, ...; EarlyFusion: 5, 6, 7, ... blocks."""
    if cls_name in SERRA:
        return [np.zeros((40 + 3 * i, 12), np.float32) for i in range(n)]
    return [dict(mfccs=np.zeros((5 + i, 650), np.float32), ssms=np.zeros((5 + i, 1225), np.float32),
                 chromas=np.zeros((5 + i, 480), np.float32), chroma_med=np.zeros(12)) for i in range(n)]


def lengths(n):
    return np.array([40 + 3 * i for i in range(n)], np.int64)
