"""
Shape sets for the Serra09 band and sweep kernels (tests/test_gpu_serra09_shapes.py) and for the streaming class
(tests/test_gpu_serra09_streaming.py); their design is checked on the CPU by tests/test_serra09_shapes_design.py.  Importable without a GPU: numpy, acoss_amd.synth, the CPU oracle and libacx's device-free
plan report.

The product path (run_serra09_impl, acoss_amd/csrc/acx.hip) sorts a batch by the size classes of a pair's two sides and picks a
band kernel and a sweep kernel per class.  The class limits and the kernel per class live in ONE place, the table of
acoss_amd/csrc/serra09_plan.hpp; `cls`, `key` and `family` below do not restate it: they ask the library (acx_serra09_plan, the
functions the run itself calls), so the design test reads the table the library was compiled with and `describe` names the kernel
it would launch.  The sets put tracks on both sides of every class edge and of every tile count, in every (reference class, query
class) combination; UPPER and LOWER are the literals they are built from.
"""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np

BAND = 8
NC = 5
UPPER = (249, 505, 761, 1017, 2041)      # the longest row (cells) of classes 0 .. 4
LOWER = (250, 506, 762, 1018)            # the shortest row of classes 1 .. 4


@functools.lru_cache(maxsize=None)
def _plan(Mq, Mr, m):
    """The library's plan record of one pair of Mq x Mr cells at stack size m (tau = 1, embed_full = 0: T = M + m frames)."""
    from acoss_amd import _lib
    rec = _lib.serra09_plan([Mq + m, Mr + m], [[0, 1]], _lib.serra09_params(m=m))[0]
    assert (int(rec["Mq"]), int(rec["Mr"])) == (Mq, Mr)
    return rec


def cls(M, m=9):
    """Size class of a row of M cells (serra09_row_class): 0 .. 4, or 5 for the streaming kernels."""
    return int(_plan(M, M, m)["cr"])


def key(Mq, Mr, m=9):
    """(cr, cq): the row pass and the sweep run per cr (rows of Mr cells), the column pass per (cr, cq) (rows of Mq cells)."""
    rec = _plan(Mq, Mr, m)
    return int(rec["cr"]), int(rec["cq"])


def family(m, c):
    """The band kernel family a pass whose longest row is of class c launches for stack size m, by the library's name for it
    (serra09_band_family; the process's ACX_BAND2 applies, as it does to the run)."""
    from acoss_amd import _lib
    M = UPPER[c] if c < NC else UPPER[-1] + 1
    return _lib.serra09_family_name(_plan(M, M, m)["row_family"], m)


def __getattr__(name):
    if name == "FAMILIES":          # (on first use: importing this module does not load the library)
        return frozenset(family(m, c) for m in (9, 10) for c in range(NC))
    raise AttributeError(name)


def _embed_len(T, m, tau=1, embed_full=0):
    import oracle
    return oracle.serra09_embed_len(T, oracle.serra09_params(m=m, tau=tau, embed_full=embed_full))


def frames_for(M, m, tau=1):
    """The shortest pooled length T whose embedded length is M (tau = 1, embed_full = 0: T = M + m, but by the function)."""
    T = max(M, (M - 1) * tau)
    while _embed_len(T, m, tau) < M:
        T += 1
    assert _embed_len(T, m, tau) == M
    return T


def _pack(tracks, Ms, pairs, **extra):
    from acoss_amd import synth
    frames, offsets = synth.pack(tracks)
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    return dict(frames=frames, offsets=offsets, pairs=pairs, M=np.asarray(Ms, np.int64), **extra)


def _work(rng, T):
    """One long chord sequence in the style of synth.cover_set: triads held for 4-16 frames."""
    from acoss_amd import synth
    tri = synth._triads()
    chords = []
    c = int(rng.integers(0, 24))
    while len(chords) < T:
        chords += [c] * int(rng.integers(4, 17))
        c = (c + int(rng.choice([-5, -2, 2, 5, 7, 1]))) % 24
    return tri[np.array(chords[:T])]


def _version(rng, excerpt):
    from acoss_amd import synth
    x = np.roll(excerpt, int(rng.integers(0, 12)), axis=1) + 0.05 * rng.random(excerpt.shape)
    return synth._frame_max_normalise(x)


def _iid(rng, T):
    from acoss_amd import synth
    return synth._frame_max_normalise(rng.random((T, 12)))


@functools.lru_cache(maxsize=4)
def edge_set(m, seed=0):
    """Tracks at both sides of every class edge (249 | 250, 505 | 506, 761 | 762, 1017 | 1018), at 2041, 40 and 3 cells: per length one
    excerpt from the START of one long work and one from its END (rolled, noisy versions of it), so that alignments run through
    the first and the last tiles.  45 pairs, 26.8 Mcells: the 25 (query edge, reference edge) combinations of the upper edges
    (every (cr, cq) key), each lower edge against its upper neighbour in both orders, against its twin, a 40- and a 3-cell track."""
    rng = np.random.default_rng([seed, m, 1])
    lengths = list(UPPER) + list(LOWER) + [3, 40]
    W = frames_for(max(lengths), m) + 500
    work = _work(rng, W)
    tracks, Ms, start, end = [], [], {}, {}
    for M in lengths:
        T = frames_for(M, m)
        start[M] = len(tracks); tracks.append(_version(rng, work[:T])); Ms.append(M)
        end[M] = len(tracks); tracks.append(_version(rng, work[W - T:])); Ms.append(M)
    pairs = [(start[a], end[b]) for a in UPPER for b in UPPER]
    for lo, up in zip(LOWER, UPPER):
        pairs += [(start[lo], end[up]), (end[up], start[lo])]
    for lo in LOWER:
        pairs += [(start[lo], end[lo]), (start[lo], end[40]), (start[lo], end[3])]
    return _pack(tracks, Ms, pairs, start=start, end=end)


@functools.lru_cache(maxsize=2)
def tile_edge_set(m, seed=0):
    """i.i.d. tracks of 57 + 64 k (k = 0 .. 31) and 58 + 64 k (k = 0 .. 30) cells -- the last length of a tile count and the first
    of the next, for every count `ndata` takes -- each against one 300-cell track in both orders: 126 pairs."""
    rng = np.random.default_rng([seed, m, 2])
    Ms = [57 + 64 * k for k in range(32)] + [58 + 64 * k for k in range(31)] + [300]
    tracks = [_iid(rng, frames_for(M, m)) for M in Ms]
    f = len(Ms) - 1
    pairs = [(i, f) for i in range(f)] + [(f, i) for i in range(f)]
    return _pack(tracks, Ms, pairs)


@functools.lru_cache(maxsize=3)
def row_residue_set(m, seed=0):
    """Queries of 1 .. 17 and 248 .. 251 cells (every row count mod 8, the tails of four and of two rows per wave) against references of
    100, 400, 700, 1000 and 1500 cells (one per class): 105 pairs."""
    rng = np.random.default_rng([seed, m, 3])
    q = list(range(1, 18)) + [248, 249, 250, 251]
    r = [100, 400, 700, 1000, 1500]
    Ms = q + r
    tracks = [_iid(rng, frames_for(M, m)) for M in Ms]
    pairs = [(i, len(q) + j) for i in range(len(q)) for j in range(len(r))]
    return _pack(tracks, Ms, pairs)


# ---- the streaming class (cr = cq = 5: a side of more than 2041 cells, or a stack of 17 .. 33 frames) ----------------------------------
# csm_long_kernel works in 64 x 64 tiles, rowsel_long_kernel and binarise_long_kernel four rows to a workgroup, qmax_bits_long_kernel in
# strips of STRIP columns.  tests/test_gpu_serra09_streaming.py uses the sets below; tests/test_serra09_shapes_design.py shows what they reach.
TILE = 64
STRIP = 2048
STACK_SIDES = (1, 2, 3, 63, 64, 65, 127, 128, 129, 200, 449)
LONG_SIDES = (2042, 2048, 2049, 2050, 2051, 2112, 2113, 4096, 4097, 4099)
SHORT_SIDES = (1, 2, 3, 40, 65)
LONG_SQUARES = ((2042, 2049), (2050, 2042), (2049, 2113))
SEAM_QUERY_AT = (1900, 3950)             # frames of the work at which the seam set's two 300-cell queries start
SEAM_CELLS = (4300, 300)


def _two_ends(rng, lengths, m, tau, slack=500):
    """Per length one version of the START and one of the END of one long work: (tracks, Ms, start, end, work)."""
    W = frames_for(max(lengths), m, tau) + slack
    work = _work(rng, W)
    tracks, Ms, start, end = [], [], {}, {}
    for M in lengths:
        T = frames_for(M, m, tau)
        start[M] = len(tracks); tracks.append(_version(rng, work[:T])); Ms.append(M)
        end[M] = len(tracks); tracks.append(_version(rng, work[W - T:])); Ms.append(M)
    return tracks, Ms, start, end, work


@functools.lru_cache(maxsize=None)
def stack_set(m, seed=0, tau=1):
    """For stacks of 17 .. 33 frames (every pair streams).  Sides of 1, 2, 3, 63, 64, 65, 127, 128, 129, 200 and 449 cells: a last tile of
    1, 63 and 64 rows and columns, every row count mod 4, matrices of one to three rows or columns.  Two versions per length (start and
    end of one work), all 121 (start[a], end[b]) pairs: 1 515 361 cells."""
    rng = np.random.default_rng([seed, m, 4])
    tracks, Ms, start, end, _ = _two_ends(rng, STACK_SIDES, m, tau)
    pairs = [(start[a], end[b]) for a in STACK_SIDES for b in STACK_SIDES]
    return _pack(tracks, Ms, pairs, start=start, end=end)


@functools.lru_cache(maxsize=None)
def long_set(m, seed=0, tau=1):
    """For any stack size m <= 33.  Long sides of 2042 (the first length of class 5), 2048 .. 2051, 2112 | 2113, 4096 | 4097 and 4099 cells --
    both sides of one, two and three strips for dp_start 2 and for 3 (which drops a column), both sides of a tile edge -- each against short
    sides of 1, 2, 3, 40 and 65 cells in BOTH orders (long rows; long columns with few rows), alternately the two tracks' END versions (the
    alignment runs into the last strip and the last tiles) and their START versions; plus 2042 x 2049, 2050 x 2042 and 2049 x 2113.
    103 pairs, 18 639 749 cells."""
    rng = np.random.default_rng([seed, m, 5])
    tracks, Ms, start, end, _ = _two_ends(rng, LONG_SIDES + SHORT_SIDES, m, tau)
    pairs = []
    for a, L in enumerate(LONG_SIDES):
        for b, s in enumerate(SHORT_SIDES):
            one, other = (end, start) if (a + b) % 2 == 0 else (start, end)
            pairs += [(one[s], one[L]), (other[L], other[s])]
    pairs += [(start[a], end[b]) for a, b in LONG_SQUARES]
    return _pack(tracks, Ms, pairs, start=start, end=end)


def long_subset(d, sides=(2042, 2049)):
    """The pairs of a long_set whose long side is one of `sides` and whose other side is short: twenty for the default."""
    M = d["M"]
    keep = [(i, j) for i, j in d["pairs"] if (M[i] in sides and M[j] in SHORT_SIDES) or (M[j] in sides and M[i] in SHORT_SIDES)]
    return subset(d, keep)


@functools.lru_cache(maxsize=None)
def seam_set(m, seed=0):
    """One reference of 4300 cells, a version of a whole work, and two queries of 300 cells cut from the same work at frames 1900 and 3950:
    their true alignments cross reference columns 2048 and 4096, the seams between the strips of qmax_bits_long_kernel.  Both orders of each
    pair; in the swapped order the seam is crossed by rows, which is the control."""
    rng = np.random.default_rng([seed, m, 6])
    Mr, Mq = SEAM_CELLS
    work = _work(rng, frames_for(Mr, m))
    Tq = frames_for(Mq, m)
    tracks = [_version(rng, work)] + [_version(rng, work[at:at + Tq]) for at in SEAM_QUERY_AT]
    return _pack(tracks, [Mr, Mq, Mq], [(1, 0), (2, 0), (0, 1), (0, 2)])


TIE_LONG = 2100


@functools.lru_cache(maxsize=None)
def tie_set(m, seed=0):
    """The track kinds of tests/fuzz_serra09.py whose distance rows hold exact ties, at rows of 100 .. 700 cells: a constant track,
    piecewise-constant tracks (segments of 3, 7, 25 and 40 frames over 1 .. 5 prototypes, no noise), tracks that repeat an 8 / 16 / 32-frame
    pattern with 0.02 noise and a twin on the 32-frame pattern, sparse frames with exact zeros, one i.i.d. track; and one piecewise-constant
    track of 2100 cells, which streams at any m.  Every ordered pair of the eleven short tracks, self pairs included, and the long track
    against three of them in both orders: 127 pairs."""
    from acoss_amd import synth
    rng = np.random.default_rng([seed, m, 7])
    protos = synth._frame_max_normalise(rng.random((5, 12)))

    def steps(M, seg, nproto):
        T = frames_for(M, m)
        return protos[np.repeat(rng.integers(0, nproto, T // seg + 1), seg)[:T]].astype(np.float32)

    def periodic(M, period, base=None):
        T = frames_for(M, m)
        base = synth._frame_max_normalise(rng.random((period, 12))) if base is None else base
        return base, (np.tile(base, (T // period + 1, 1))[:T] + 0.02 * rng.random((T, 12))).astype(np.float32)

    def sparse(M):
        T = frames_for(M, m)
        x = rng.random((T, 12)) * (rng.random((T, 12)) < 0.4)
        x[:, 0] += 0.01
        return synth._frame_max_normalise(x)

    Ms = [120, 150, 257, 300, 700, 130, 200, 420, 400, 180, 110, TIE_LONG]
    b32, p32 = periodic(420, 32)
    tracks = [steps(120, 1, 1), steps(150, 3, 2), steps(257, 7, 5), steps(300, 25, 3), steps(700, 40, 4),
              periodic(130, 8)[1], periodic(200, 16)[1], p32, periodic(400, 32, b32)[1], sparse(180), _iid(rng, frames_for(110, m)),
              steps(TIE_LONG, 25, 5)]
    n = len(Ms) - 1
    pairs = [(i, j) for i in range(n) for j in range(n)]
    for i in (0, 3, 7):
        pairs += [(i, n), (n, i)]
    return _pack(tracks, Ms, pairs)


def relabel(d, m, tau=1, embed_full=0):
    """The same set under another embedding: d["M"] by the oracle's embedded length of every track."""
    out = dict(d)
    out["M"] = np.array([_embed_len(int(T), m, tau, embed_full) for T in np.diff(d["offsets"])], np.int64)
    return out


def subset(d, pairs):
    """The same tracks with another pair list."""
    out = dict(d)
    out["pairs"] = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    return out


def track(d, i):
    return d["frames"][d["offsets"][i]:d["offsets"][i + 1]]


def workers():
    from acoss_amd import utils
    return max(1, min(16, utils.effective_cpus()))


def pool_map(fn, items):
    """fn over items on min(16, effective CPUs) threads (the oracle's C routines run without the GIL and keep no global state)."""
    items = list(items)
    with ThreadPoolExecutor(workers()) as ex:
        return list(ex.map(fn, items))


def oracle_plots(d, **kw):
    """The oracle over the set's pairs: (scores (K,) float32, [R_k]) with the parameters kw (oracle.serra09_params)."""
    import oracle
    oracle.lib()
    p = oracle.serra09_params(**kw)
    def one(ij):
        s, it = oracle.serra09_pair(track(d, ij[0]), track(d, ij[1]), p, want_intermediates=True)
        return s, it["R"]               # (the distances are dropped here: 16 MB for a 2041 x 2041 pair)
    res = pool_map(one, d["pairs"])
    return np.array([s for s, _ in res], np.float32), [R for _, R in res]


def oracle_scores(d, **kw):
    """The full-chain oracle's scores alone."""
    import oracle
    oracle.lib()
    p = oracle.serra09_params(**kw)
    return np.array(pool_map(lambda ij: oracle.serra09_pair(track(d, ij[0]), track(d, ij[1]), p), d["pairs"]), np.float32)


def oracle_sweeps(Rs, gamma_o=0.5, gamma_e=0.5, dmax=False):
    import oracle
    oracle.lib()
    return np.array(pool_map(lambda R: oracle.qmax_binary(R, gamma_o, gamma_e, dmax), Rs), np.float32)


def describe(d, k, m):
    """The label of pair k in failure messages: m, Mq, Mr, the class key and the band kernel families of its two passes."""
    i, j = d["pairs"][k]
    Mq, Mr = int(d["M"][i]), int(d["M"][j])
    cr, cq = key(Mq, Mr, m)
    if cr == NC:        # the streaming class has one key, one family and no band classes: say what its kernels make of the shape
        tiles = lambda M: (M + TILE - 1) // TILE
        return ("m=%d pair %d (tracks %d, %d) Mq=%d Mr=%d (cr, cq)=(%d, %d) %s + binarise_long_kernel: %d x %d tiles of 64 (the last %d rows, %d "
                "columns), qmax_bits_long_kernel: %d strip(s) of 2048 columns" % (
                    m, k, i, j, Mq, Mr, cr, cq, family(m, cr), tiles(Mq), tiles(Mr), (Mq - 1) % TILE + 1, (Mr - 1) % TILE + 1,
                    (Mr + STRIP - 1) // STRIP))
    return "m=%d pair %d (tracks %d, %d) Mq=%d Mr=%d (cr, cq)=(%d, %d) row pass %s, column pass %s" % (
        m, k, i, j, Mq, Mr, cr, cq, family(m, cr), family(m, cq))


def assert_plots_equal(d, m, got, want, tag=""):
    """Bit for bit; the message names the pair, its kernels, the number of differing cells and the first of them."""
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape, "%s %s: shape %s vs %s" % (tag, describe(d, k, m), g.shape, w.shape)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            raise AssertionError("%s %s: recurrence plot differs in %d of %d cells, first at (row %d, column %d): device %d, oracle %d" % (
                tag, describe(d, k, m), len(bad), g.size, bad[0][0], bad[0][1], g[tuple(bad[0])], w[tuple(bad[0])]))


def assert_scores_equal(d, m, got, want, tag=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.nonzero((got != want).reshape(len(got), -1).any(axis=1))[0]
        raise AssertionError("%s scores differ for %d of %d pairs, first: %s: device %s, oracle %s" % (
            tag, len(bad), len(got), describe(d, int(bad[0]), m), got[bad[0]], want[bad[0]]))
