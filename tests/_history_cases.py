"""
History independence (tests/test_gpu_arena_history.py): a DIRTYING call, the PROBE calls that run inside what it left behind, and
the probes' CPU references, per kernel family.  tests/test_history_cases_design.py shows on the CPU what the cases reach.
Importable without a GPU: numpy, acoss_amd.synth, the CPU oracle, the suite's reference modules and libacx's device-free plan
reports (acx_serra09_plan, acx_ef_plan).

A context keeps its device arenas from call to call (grow-only, never cleared), and many kernels read arena words they did not
write.  The schedule of the GPU test, per fill word of WORDS and per probe:

    a new context, with the allocation fill on (acx_debug_set_alloc_fill)  ->  case.prepare(ctx)  ->  probe.dirty(ctx)
    ->  ctx.debug_fill_arenas(word)  ->  probe.run(ctx)

probe.run returns the API's outputs as a dict of numpy arrays: the same bits for all five words, and what probe.want says under
the checker of the family's own test.  Nothing here restates a reference: `want` comes from the modules the suite already has.
"""
import functools

import numpy as np

from . import _serra09_shapes as S

# 0; NaN as f32 and f64, an all-ones bitmap, -1, direction code 3 everywhere; +inf; a denormal below every cell; direction code 1
# everywhere (a traceback that does not stop on a stale word keeps walking)
WORDS = (0x00000000, 0xFFFFFFFF, 0x7F800000, 0x00000001, 0x55555555)


class Probe(object):
    """kind: which checker of tests/test_gpu_arena_history.py holds the outputs against `want`; dirty(ctx) and run(ctx) as above;
    want: a function without arguments (the references are computed on first use and kept)."""

    def __init__(self, name, kind, dirty, run, want, **info):
        self.name, self.kind, self.dirty, self.run, self._want, self.info = name, kind, dirty, run, want, info
        self._cache = None

    @property
    def want(self):
        if self._cache is None:
            self._cache = self._want()
        return self._cache


class Case(object):
    """prepare(ctx): the uploads every probe of the case needs; probes: a list of Probe."""

    def __init__(self, name, prepare, probes):
        self.name, self.prepare, self.probes = name, prepare, probes


def flat(out):
    """A probe's outputs as bytes per name: what must not move with the fill word."""
    return {k: (np.ascontiguousarray(v).tobytes(), np.asarray(v).shape, str(np.asarray(v).dtype)) for k, v in sorted(out.items())}


# ======================================================================================================================================
# Serra09: the product path and the alignments
# ======================================================================================================================================
M9, M17 = 9, 17
DENSE_KAPPA = 0.4
DENSE = ((1017, 1017), (2041, 505))                      # the dirtying list, in cells (Mq, Mr)
# ragged row bands, ragged column tiles, both sides of the first class edge
BAND_PROBES = ((3, 40), (40, 3), (57, 300), (249, 58), (250, 506))
# the streaming class: D2^T and the strip records in d_scratch
STREAM_PROBES = ((2042, 3), (3, 2042))
SEAM_PROBE = (40, 2049)                                   # the locating sweep's seam records (alignments only)
STACK17 = (63, 65)                                        # cells at m = 17; the same tracks hold 71 and 73 cells at m = 9
_SIDES = (1017, 2041, 505, 3, 40, 57, 300, 249, 58, 250, 506, 2042, 2049, STACK17[0] + M17 - M9, STACK17[1] + M17 - M9)


@functools.lru_cache(maxsize=None)
def serra09_pool():
    """Two versions (the start and the end of one work) of a track of every side the cases name: pair (Mq, Mr) = (start[Mq], end[Mr]);
    the seam probe's query is a copy of the last 40 cells of end[2049], so that its alignment runs down the diagonal into the last
    column, 2048: the one column of the second strip."""
    rng = np.random.default_rng([31, 9])
    tracks, Ms, start, end, _ = S._two_ends(rng, _SIDES, M9, 1)
    tracks.append(tracks[end[SEAM_PROBE[1]]][-S.frames_for(SEAM_PROBE[0], M9):].copy())
    Ms.append(SEAM_PROBE[0])
    return S._pack(tracks, Ms, [], start=start, end=end, seam_query=len(tracks) - 1)


def serra09_pairs(shapes, m=M9):
    d = serra09_pool()
    off = m - M9
    return np.array([(d["seam_query"] if (a, b) == SEAM_PROBE else d["start"][a + off], d["end"][b + off]) for a, b in shapes],
                    np.int32).reshape(-1, 2)


def _params(m=M9, **kw):
    from acoss_amd import _lib
    return _lib.serra09_params(m=m, **kw)


@functools.lru_cache(maxsize=None)
def probe_kw(shape):
    """What a probe sets beside m: the seam probe runs without the transposition index, which the 40-cell copy's global profile
    would turn away from its own track's."""
    return dict(oti=False) if shape == SEAM_PROBE else {}


@functools.lru_cache(maxsize=None)
def serra09_reference(shape, m=M9):
    """(score, plot) of the oracle for one probe pair at the default kappa."""
    d = S.subset(S.relabel(serra09_pool(), m), serra09_pairs([shape], m))
    scores, Rs = S.oracle_plots(d, m=m, **probe_kw(shape))
    assert Rs[0].shape == shape
    return scores[:1], Rs[0]


def _upload_serra09(ctx):
    d = serra09_pool()
    ctx.upload_pool(d["frames"], d["offsets"])


def _serra09_probe(export, shape, m):
    from . import _dmax_align_ref, _qmax_locate_ref, _qmax_path_ref, _qmax_sections_ref
    dense, pair = serra09_pairs(DENSE), serra09_pairs([shape], m)
    name = "%s %dx%d m=%d" % ((export,) + shape + (m,))

    def plot():
        return serra09_reference(shape, m)[1]

    def call(ctx, pairs, p):
        if export == "serra09_debug_bits":
            scores, Rs = ctx.serra09_debug_bits(pairs, p)
            print("%s: %d set bits outside the matrices' columns (masked by the sweeps)" % (name, ctx.outside_bits))
            return dict(scores=scores, **{"plot%d" % k: R for k, R in enumerate(Rs)})
        if export == "serra09_pairs":
            return dict(scores=ctx.serra09_pairs(pairs, p))
        if export == "chenfusion_pairs":
            return dict(scores=ctx.chenfusion_pairs(pairs, p))
        if export == "serra09_align":
            return dict(records=ctx.serra09_align(pairs, p))
        if export == "chenfusion_align":
            return dict(records=ctx.chenfusion_align(pairs, p, plane=1))
        if export in ("serra09_align_paths", "chenfusion_align_paths"):
            got = ctx.serra09_align_paths(pairs, p) if export == "serra09_align_paths" else ctx.chenfusion_align_paths(pairs, p, plane=1)
            return dict(records=got[0], offsets=got[1], cells=got[2])
        assert export == "serra09_align_sections", export
        got = ctx.serra09_align_sections(pairs, p, paths=True)
        return dict(records=got[0], counts=got[1], offsets=got[2], cells=got[3])

    def want():
        score, R = serra09_reference(shape, m)
        if export == "serra09_debug_bits":
            return dict(scores=score, plots=[R])
        if export == "serra09_pairs":
            return dict(scores=score)
        if export == "chenfusion_pairs":
            return dict(scores=np.stack([score, S.oracle_sweeps([R], dmax=True)], 1))
        if export == "serra09_align":
            return dict(record=_qmax_locate_ref.locate_forward(R, 0.5, 0.5, 2))
        if export == "serra09_align_paths":
            rec, cells, _ = _qmax_path_ref.path_full(R, 0.5, 0.5, 2)
            return dict(record=rec, cells=cells)
        if export == "serra09_align_sections":
            recs, paths = _qmax_sections_ref.sections_full(R, 0.5, 0.5, 2)
            return dict(records=recs, paths=paths)
        rec, cells, _ = _dmax_align_ref.dmax_full(R, 0.5, 0.5, 2)
        return dict(record=rec, cells=cells) if export == "chenfusion_align_paths" else dict(record=rec)

    return Probe(name, export, lambda ctx: call(ctx, dense, _params(kappa=DENSE_KAPPA)), lambda ctx: call(ctx, pair, _params(m, **probe_kw(shape))), want,
                 shape=shape, m=m, pairs=pair, dense=dense, plot=plot)


PRODUCT_EXPORTS = ("serra09_debug_bits", "serra09_pairs", "chenfusion_pairs")
ALIGN_EXPORTS = ("serra09_align", "serra09_align_paths", "serra09_align_sections", "chenfusion_align", "chenfusion_align_paths")
PRODUCT_SHAPES = tuple((s, M9) for s in BAND_PROBES + STREAM_PROBES) + ((STACK17, M17),)
ALIGN_SHAPES = PRODUCT_SHAPES + ((SEAM_PROBE, M9),)


def serra09_product_case():
    return Case("serra09 product path", _upload_serra09, [_serra09_probe(e, s, m) for s, m in PRODUCT_SHAPES for e in PRODUCT_EXPORTS])


def serra09_align_case():
    return Case("serra09 alignments", _upload_serra09, [_serra09_probe(e, s, m) for s, m in ALIGN_SHAPES for e in ALIGN_EXPORTS])


# ---- the same probes behind the dense pairs inside ONE list, in a later batch ------------------------------------------------------------
# Two lists: a streaming pair takes more scratch than both dense pairs together, so no limit that admits it sends a band probe to a
# later batch.  Under the smallest limit the plan accepts, the first dense pair fills batch 0 and every probe runs in batch 1 or later
# (tests/test_history_cases_design.py holds that from the plan's report).
ONE_LISTS = (("band probes", BAND_PROBES), ("streaming probes", STREAM_PROBES))


def one_list_pairs(shapes):
    return np.concatenate([serra09_pairs(DENSE), serra09_pairs(shapes)])


@functools.lru_cache(maxsize=None)
def one_list_limit(shapes):
    """The smallest scratch limit (bytes, a multiple of 1 KiB) under which the plan accepts the list."""
    from acoss_amd import _lib
    lens = np.diff(serra09_pool()["offsets"])
    for kib in range(1, 1 << 16):
        try:
            _lib.serra09_plan(lens, one_list_pairs(shapes), _params(kappa=DENSE_KAPPA), scratch_limit=kib << 10)
        except _lib.AcxError:
            continue
        return kib << 10
    raise AssertionError("no scratch limit below 64 MiB takes the list")


@functools.lru_cache(maxsize=None)
def one_list_reference(shapes):
    """(scores, plots) of the oracle for the whole list at the dense kappa."""
    return S.oracle_plots(S.subset(serra09_pool(), one_list_pairs(shapes)), m=M9, kappa=DENSE_KAPPA)


def _one_list_probe(export, label, shapes):
    pairs, dense = one_list_pairs(shapes), serra09_pairs(DENSE)
    p = lambda: _params(kappa=DENSE_KAPPA)
    fn = lambda ctx, pr: dict(scores=getattr(ctx, export)(pr, p()))

    def run(ctx):
        ctx.set_scratch_limit(one_list_limit(shapes))
        try:
            return fn(ctx, pairs)
        finally:
            ctx.set_scratch_limit(0)

    def want():
        scores, Rs = one_list_reference(shapes)
        return dict(scores=scores if export == "serra09_pairs" else np.stack([scores, S.oracle_sweeps(Rs, dmax=True)], 1))

    return Probe("%s one list, %s" % (export, label), export, lambda ctx: fn(ctx, dense), run, want, pairs=pairs, dense=dense, shapes=shapes)


def serra09_one_list_case():
    return Case("serra09 one list, later batch", _upload_serra09,
                [_one_list_probe(e, label, shapes) for label, shapes in ONE_LISTS for e in ("serra09_pairs", "chenfusion_pairs")])


# ---- the stand-alone exports on planted plots ------------------------------------------------------------------------------------------------
PLOT_EXPORTS = ("qmax_binary", "qmax_locate_binary", "qmax_path_binary", "qmax_sections_binary", "dmax_locate_binary", "dmax_path_binary")
ONES_PLOT = (64, 2112)
PLOT_PROBES = ((40, 2049, 0.05), (33, 65, 0.05))


@functools.lru_cache(maxsize=None)
def planted_plot(M, N, density):
    return (np.random.default_rng([M, N, 5]).random((M, N)) < density).astype(np.uint8)


def _plot_probe(export, M, N, density):
    from . import _dmax_align_ref, _qmax_locate_ref, _qmax_path_ref, _qmax_sections_ref
    R, ones = planted_plot(M, N, density), np.ones(ONES_PLOT, np.uint8)

    def call(ctx, P):
        got = getattr(ctx, export)(P)
        if export == "qmax_binary":
            return dict(score=np.float32(got))
        if export.endswith("locate_binary"):
            return dict(records=got)
        if export.endswith("path_binary"):
            return dict(records=got[0], cells=got[1])
        return dict(records=got[0], counts=np.int32(got[1]), offsets=got[2], cells=got[3])

    def want():
        import oracle
        if export == "qmax_binary":
            return dict(score=np.float32(oracle.qmax_binary(R, 0.5, 0.5, False)))
        if export == "qmax_locate_binary":
            return dict(record=_qmax_locate_ref.locate_forward(R, 0.5, 0.5, 2))
        if export == "qmax_path_binary":
            rec, cells, _ = _qmax_path_ref.path_full(R, 0.5, 0.5, 2)
            return dict(record=rec, cells=cells)
        if export == "qmax_sections_binary":
            recs, paths = _qmax_sections_ref.sections_full(R, 0.5, 0.5, 2)
            return dict(records=recs, paths=paths)
        rec, cells, _ = _dmax_align_ref.dmax_full(R, 0.5, 0.5, 2)
        return dict(record=rec, cells=cells) if export == "dmax_path_binary" else dict(record=rec)

    return Probe("%s %dx%d" % (export, M, N), export, lambda ctx: call(ctx, ones), lambda ctx: call(ctx, R), want, plot=lambda: R)


def serra09_plots_case():
    return Case("serra09 stand-alone plots", lambda ctx: None, [_plot_probe(e, *s) for s in PLOT_PROBES for e in PLOT_EXPORTS])


# ======================================================================================================================================
# EarlyFusion: the stand-alone exports
# ======================================================================================================================================
EF_KAPPA, EF_K = 0.1, 10
CSM_DIRT = (9, 1088)                                       # matrices of -1e30 and of +1e30: below and above every cell
CSM_PROBES = ((9, 1025), (12, 513), (12, 65))              # the long kernels, the wide and the narrow register class
SW_ONES = (64, 1024)
SW_PROBES = ((33, 65), (5, 1023))
XSEL_DIRT = (8, 1024)
XSEL_PROBES = ((65, 0.1), (5, 0.5))                        # (N, kappa) of the crafted rows


@functools.lru_cache(maxsize=None)
def csm_matrix(M, N):
    return np.random.default_rng([M, N, 6]).random((M, N)).astype(np.float32)


def _csm_probe(export, M, N):
    from . import _ef_backend_ref as backend
    C = csm_matrix(M, N)

    def call(ctx, D):
        if export == "csm_binary_sw":
            return dict(score=np.float32(ctx.csm_binary_sw(D, EF_KAPPA)))
        d = ctx.csm_debug_bits(D, EF_KAPPA, EF_K)
        out = dict(t=d["t"], jcut=d["jcut"], r=d["r"], score=np.float32(d["score"]))
        if d["bits"] is not None:
            out["bits"] = d["bits"]
        return out

    def dirty(ctx):
        call(ctx, np.full(CSM_DIRT, -1e30, np.float32))
        call(ctx, np.full(CSM_DIRT, 1e30, np.float32))

    def want():
        import oracle
        kb = oracle.binary_k(EF_KAPPA, N)
        t, jcut = backend.thresholds(C, kb)
        B = backend.binarise(C, t, jcut)
        return dict(kb=kb, t=t, jcut=jcut, plot=B, tenths=backend.sw_tenths(B), bits=backend.pack_bits(B) if max(M, N) <= 1024 else None)

    return Probe("%s %dx%d" % (export, M, N), export, dirty, lambda ctx: call(ctx, C), want, matrix=C)


@functools.lru_cache(maxsize=None)
def sw_plot(M, N):
    from . import _sw_align_ref
    return _sw_align_ref.random_plot(np.random.default_rng([M, N, 7]), M, N, 0.05)


SW_EXPORTS = ("sw_binary", "sw_bits_binary", "sw_align_binary", "sw_sections_binary")


def _sw_probe(export, M, N):
    from . import _ef_backend_ref as backend
    from . import _sw_align_ref, _sw_sections_ref
    B, ones = sw_plot(M, N), np.ones(SW_ONES, np.uint8)

    def call(ctx, P):
        got = getattr(ctx, export)(P)
        if export in ("sw_binary", "sw_bits_binary"):
            return dict(score=np.float32(got))
        if export == "sw_align_binary":
            return dict(records=got[0], cells=got[1])
        return dict(records=got[0], counts=np.int32(got[1]), offsets=got[2], cells=got[3])

    def want():
        if export in ("sw_binary", "sw_bits_binary"):
            return dict(tenths=backend.sw_tenths(B))
        if export == "sw_align_binary":
            rec, cells = _sw_align_ref.align_forward(B)
            return dict(record=rec, cells=cells)
        recs, paths = _sw_sections_ref.sections_full(B)
        return dict(records=recs, paths=paths)

    return Probe("%s %dx%d" % (export, M, N), export, lambda ctx: call(ctx, ones), lambda ctx: call(ctx, B), want, plot=lambda: B)


@functools.lru_cache(maxsize=None)
def xsel_rows(N, kappa):
    """The crafted rows of tests/test_gpu_crossfusion.py (one per way the selection can exit) at N columns."""
    from . import _crossfusion_ref
    from .test_gpu_crossfusion import _crafted_rows
    return _crafted_rows(N, _crossfusion_ref.binary_k(kappa, N), np.random.default_rng(100 + N))[0]


def _xsel_probe(N, kappa):
    from . import _crossfusion_ref
    X = xsel_rows(N, kappa)

    def call(ctx, Y, kap):
        bits, score = ctx.xsel_binary_sw(Y, kappa=kap)
        return dict(bits=bits, score=np.float32(score))

    def want():
        import oracle
        B = _crossfusion_ref.select(X, _crossfusion_ref.binary_k(kappa, N))
        return dict(bits=_crossfusion_ref.pack_bits(B), plot=B, score=oracle.sw_constrained(B))

    return Probe("xsel_binary_sw N=%d" % N, "xsel_binary_sw", lambda ctx: call(ctx, np.ones(XSEL_DIRT), 0.1), lambda ctx: call(ctx, X, kappa), want,
                 rows=X, kappa=kappa)


def ef_stand_alone_case():
    probes = [_csm_probe(e, M, N) for M, N in CSM_PROBES for e in ("csm_debug_bits", "csm_binary_sw")]
    probes += [_sw_probe(e, M, N) for M, N in SW_PROBES for e in SW_EXPORTS]
    probes += [_xsel_probe(N, kappa) for N, kappa in XSEL_PROBES]
    return Case("earlyfusion stand-alone", lambda ctx: None, probes)


# ======================================================================================================================================
# EarlyFusion: the product path.  The reference of a probe is the specification applied to the DEVICE's own matrices (acx_ef_debug_pairs
# on a context nobody filled), as in tests/test_gpu_ef_backend.py and tests/test_gpu_sw_align.py: ef_want() below says how.
# ======================================================================================================================================
EF_BLOCKS = (5, 12, 64, 65, 140, 513, 1025, 513)          # (a second track of 513 blocks: the dirtying pair (513, 513))
EF_DIRTY = ((5, 7), (4, 5))                                # track indices: (513, 513) and (140, 513), at K = 17 (keeps C^T)
EF_DIRTY_K = 17
EF_BIT_PROBES = ((5, 12), (12, 5), (64, 65), (65, 64), (12, 140))          # in blocks
EF_FLOAT_LIST = ((1025, 12), (12, 1025), (5, 65))                           # one list with the 1025-block track: the float path
EF_KS = (10, 17)
EF_PLANES = (0, 3)                                         # mfccs and early


@functools.lru_cache(maxsize=None)
def ef_pool():
    """Random tracks in the style of tests/test_gpu_ef_backend.py, with shared excerpts (alignments longer than noise gives) between
    the tracks of 64 and 65 blocks, of 12 and 140, and of 513 and 1025."""
    from .test_gpu_ef_backend import _track
    tracks = [_track(nb, 83000 + k) for k, nb in enumerate(EF_BLOCKS)]
    rng = np.random.default_rng(83999)
    for a, b, at_a, at_b, m in ((2, 3, 5, 20, 40), (1, 4, 2, 100, 9), (5, 6, 100, 600, 60)):
        for key in ("mfccs", "ssms", "chromas"):
            tracks[b][key][at_b:at_b + m] = tracks[a][key][at_a:at_a + m] + 0.02 * rng.standard_normal((m, tracks[a][key].shape[1])).astype(np.float32)
    return tracks


def ef_pairs(shapes):
    """(M, N) in blocks -> sorted (first, second) track indices, and the position of every shape in the sorted list."""
    idx = [(EF_BLOCKS.index(m), EF_BLOCKS.index(n)) for m, n in shapes]
    order = sorted(range(len(idx)), key=lambda k: idx[k])
    pairs = np.array([idx[k] for k in order], np.int32).reshape(-1, 2)
    return pairs, {shapes[k]: order.index(k) for k in range(len(idx))}


def _ef_probe(export, shapes, which, K, plane):
    pairs, where = ef_pairs(shapes)
    k = where[which]
    dense = np.array(sorted(EF_DIRTY), np.int32)

    def call(ctx, pr, K_, kk):
        if export == "earlyfusion_pairs":
            return dict(scores=ctx.earlyfusion_pairs(pr, EF_KAPPA, K_))
        if export == "ef_debug_bits":
            d = ctx.ef_debug_bits(pr, kk, EF_KAPPA, K_)
            return {key: v for key, v in d.items() if v is not None}
        if export in ("ef_align", "ef_align_long"):
            got = getattr(ctx, export)(pr, EF_KAPPA, K_, plane=plane, paths=True)
            return dict(records=got[0], offsets=got[1], cells=got[2])
        assert export == "ef_align_sections", export
        got = ctx.ef_align_sections(pr, EF_KAPPA, K_, plane=plane, paths=True)
        return dict(records=got[0], counts=got[1], offsets=got[2], cells=got[3])

    name = "%s %s K=%d" % (export, "%dx%d" % which if len(shapes) == 1 else "list:%dx%d" % which, K)
    if export not in ("earlyfusion_pairs", "ef_debug_bits"):
        name += " plane %d" % plane
    return Probe(name, export, lambda ctx: call(ctx, dense, EF_DIRTY_K, 0), lambda ctx: call(ctx, pairs, K, k), lambda: None,
                 pairs=pairs, which=k, K=K, plane=plane, shape=which, dense=dense)


def ef_product_case():
    probes = []
    for K in EF_KS:
        for shape in EF_BIT_PROBES:
            probes += [_ef_probe("earlyfusion_pairs", (shape,), shape, K, 3), _ef_probe("ef_debug_bits", (shape,), shape, K, 3)]
            probes += [_ef_probe("ef_align", (shape,), shape, K, pl) for pl in EF_PLANES]
            probes += [_ef_probe("ef_align_sections", (shape,), shape, K, 3), _ef_probe("ef_align_long", (shape,), shape, K, 3)]
        probes.append(_ef_probe("earlyfusion_pairs", EF_FLOAT_LIST, EF_FLOAT_LIST[0], K, 3))
        probes += [_ef_probe("ef_debug_bits", EF_FLOAT_LIST, shape, K, 3) for shape in EF_FLOAT_LIST]
        probes += [_ef_probe("ef_align_long", EF_FLOAT_LIST, EF_FLOAT_LIST[0], K, pl) for pl in EF_PLANES]
    return Case("earlyfusion product path", lambda ctx: ctx.ef_upload_pool(ef_pool()), probes)


def ef_plots(mats, kappa=EF_KAPPA):
    """The four plots of a pair by the specification on its four matrices (three CSMs and the fused matrix): (t, jcut, plot) each."""
    import oracle
    from . import _ef_backend_ref as backend
    out = []
    for C in mats:
        t, jcut = backend.thresholds(C, oracle.binary_k(kappa, C.shape[1]))
        out.append((t, jcut, backend.binarise(C, t, jcut)))
    return out


def ef_want(export, plot):
    """What an alignment export returns for one plot, by the reference modules."""
    from . import _sw_align_ref, _sw_sections_ref
    if export == "ef_align_sections":
        recs, paths = _sw_sections_ref.sections_full(plot)
        return dict(records=recs, paths=paths)
    rec, cells = _sw_align_ref.align_forward(plot)
    return dict(record=rec, cells=cells)


# ======================================================================================================================================
# Rank, query, SiMPle and the entry points that allocate per call
# ======================================================================================================================================
RANK_SMALL, RANK_LARGE = 63, 4097


@functools.lru_cache(maxsize=None)
def rank_input(n):
    """Heavily tied score rows (eighths), a row per track up to 24, up to 12 mates a row, a tie order: tests/test_gpu_rank.py's recipe."""
    rng = np.random.default_rng(n)
    R = min(n, 24)
    D = (np.round(rng.random((R, n)) * 8) / 8).astype(np.float32)
    rows = np.arange(R, dtype=np.int32)
    moff, mates = [0], []
    for t in rows:
        cand = rng.choice(n - 1, size=min(int(rng.integers(1, 13)), n - 1), replace=False)
        mates += [int(c) + (1 if c >= t else 0) for c in cand]
        moff.append(len(mates))
    return D, rows, np.array(moff, np.int64), np.array(mates, np.int32), rng.permutation(n).astype(np.int32)


def _rank_probe(export):
    from . import _rank_ref

    def call(ctx, n):
        D, rows, moff, mates, posn = rank_input(n)
        if export == "rank_columns":
            pos, flag = ctx.rank_columns(D, rows, moff, mates, posn=posn)
            return dict(pos=pos, flag=flag)
        idx, score = ctx.topk_rows(D, 10, rows=rows, posn=posn)
        return dict(idx=idx, score=score)

    def want():
        D, rows, moff, mates, posn = rank_input(RANK_SMALL)
        if export == "rank_columns":
            pos, flag = _rank_ref.rank_columns(D, rows, moff, mates, posn)
            return dict(pos=pos, flag=flag)
        idx, score = _rank_ref.topk_rows(D, 10, rows=rows, posn=posn)
        return dict(idx=idx, score=score)

    return Probe("%s n=%d" % (export, RANK_SMALL), export, lambda ctx: call(ctx, RANK_LARGE), lambda ctx: call(ctx, RANK_SMALL), want)


def rank_case():
    return Case("rank", lambda ctx: None, [_rank_probe("rank_columns"), _rank_probe("topk_rows")])


# ---- queries: Serra09 on the small pool of tests/test_gpu_query.py, whose pair scores the oracle gives bit for bit ------------------------------
QUERIES = (7, 2, 9, 2, 5)
QUERY_K = 10
QUERY_DIRT_N = 20000                                       # FTM2D shingles: rows beyond the LDS budget, the largest the query tests run


@functools.lru_cache(maxsize=None)
def query_pool():
    from acoss_amd import synth
    return synth.cover_set(clique_sizes=[2] * 9 + [3, 1], seed=31, t_range=(60, 420))


@functools.lru_cache(maxsize=None)
def query_rows():
    """(Q, N) raw Serra09 scores of QUERIES against every track by the oracle: cell (q, c) is the pair (min, max); the own cell 0."""
    import oracle
    d = query_pool()
    n = len(d["offsets"]) - 1
    pairs = np.array([(min(q, c), max(q, c)) for q in QUERIES for c in range(n) if c != q], np.int32)
    sc = oracle.serra09_pairs(d["frames"], d["offsets"], pairs)
    rows = np.zeros((len(QUERIES), n), np.float32)
    k = 0
    for i, q in enumerate(QUERIES):
        for c in range(n):
            if c != q:
                rows[i, c] = sc[k]
                k += 1
    return rows


@functools.lru_cache(maxsize=None)
def query_args():
    d = query_pool()
    n = len(d["offsets"]) - 1
    rng = np.random.default_rng(n)
    col = np.sqrt(np.diff(d["offsets"]).astype(np.float64))
    lists = np.stack([rng.permutation(np.delete(np.arange(n), q))[:8] for q in QUERIES]).astype(np.int32)
    lists[0, 2] = -1
    lists[-1, 0] = QUERIES[-1]                             # the own track
    moff = 2 * np.arange(len(QUERIES) + 1)
    mates = np.array([[(q + 1) % n, (q + 5) % n] for q in QUERIES], np.int32).reshape(-1)
    return dict(n=n, col=col, lists=lists, moff=moff, mates=mates)


def _query_prepare(ctx):
    d = query_pool()
    ctx.upload_pool(d["frames"], d["offsets"])
    ctx.ftm2d_upload_shingles(0.25 * np.random.default_rng(21).standard_normal((QUERY_DIRT_N, 8)))


def _query_probe(export):
    from acoss_amd import _lib
    from . import _query_lists_ref, _query_ref
    a = query_args()
    q = list(QUERIES)

    def run(ctx):
        p = _lib.serra09_params()
        if export == "query_topk":
            idx, score = ctx.query_topk(_lib.ALGO_SERRA09, True, p, q, QUERY_K, col=a["col"], col_mode=1)
            return dict(idx=idx, score=score)
        if export == "query_topk_lists":
            idx, score = ctx.query_topk_lists(_lib.ALGO_SERRA09, True, p, q, a["lists"], 4, col=a["col"], col_mode=1)
            return dict(idx=idx, score=score)
        pos, flag = ctx.query_ranks(_lib.ALGO_SERRA09, True, p, q, a["moff"], a["mates"], col=a["col"], col_mode=1)
        return dict(pos=pos, flag=flag)

    def dirty(ctx):
        big = [QUERY_DIRT_N - 1, 120, 7]
        if export == "query_topk":
            ctx.query_topk(_lib.ALGO_FTM2D, True, None, big, 1024)
        elif export == "query_topk_lists":
            lists = np.random.default_rng(3).permutation(QUERY_DIRT_N - 1)[:3 * 4000].reshape(3, 4000).astype(np.int32)
            ctx.query_topk_lists(_lib.ALGO_FTM2D, True, None, big, lists, 1024)
        else:
            ctx.query_ranks(_lib.ALGO_FTM2D, True, None, big, 2 * np.arange(4), np.array([1, 2, 3, 4, 5, 6], np.int32))

    def want():
        rows = query_rows()
        if export == "query_topk":
            idx, score = _query_ref.topk(rows, q, QUERY_K, col=a["col"], col_mode=1)
            return dict(idx=idx, score=score)
        if export == "query_topk_lists":
            idx, score = _query_lists_ref.topk_lists(rows, q, a["lists"], 4, col=a["col"], col_mode=1)
            return dict(idx=idx, score=score)
        full, fs = _query_ref.topk(rows, q, a["n"] - 1, col=a["col"], col_mode=1)
        assert np.all(fs[:, 1:] != fs[:, :-1]), "the rows hold no tie: a position is the place in the full ranking"
        pos = [1 + list(full[i]).index(m) for i in range(len(q)) for m in a["mates"][a["moff"][i]:a["moff"][i + 1]]]
        return dict(pos=np.array([pos], np.int32), flag=np.zeros((len(q), 1), np.uint8))

    return Probe(export, export, dirty, run, want)


def query_case():
    return Case("query", _query_prepare, [_query_probe(e) for e in ("query_topk", "query_ranks", "query_topk_lists")])


# ---- fused scores of query shortlists: the yardstick is the composition of the exports it is made of, on a context nobody filled, as in
# tests/test_gpu_fused.py (pair scores, acx_snf_fuse_dists, acx_topk_rows); the arena of a call is one block allocated per call
def fused_case():
    from acoss_amd import _lib, synth
    from .test_gpu_fused import N_CHEN, NS, _chen_tracks, _ragged

    def lists_of(which):
        if which == "small":                                # K = 2: neighbourhoods of n = K + 2 and one more, the smallest the export takes
            return _ragged(np.random.default_rng(5), N_CHEN, [4, 5, 5, 4], 6, own_rows=(1,)) + (dict(K=2, niters=2), 6)
        rng = np.random.default_rng(17)                     # K = 20: every size up to n = 257 in one call
        return _ragged(rng, N_CHEN, NS, 260, own_rows=(2, 4, 7), queries=rng.integers(0, N_CHEN, len(NS))) + (dict(K=20, niters=20), 10)

    def call(ctx, which):
        q, lists, kw, k = lists_of(which)
        frames_offsets = fused_pool()
        spec = _lib.fused_spec([(0, 1)], _lib.FUSED_SQRTLEN, **kw)
        col = np.sqrt(np.diff(frames_offsets[1]).astype(np.float64))
        idx, score, flag = ctx.query_fused_lists(_lib.ALGO_CHENFUSION, True, _lib.serra09_params(pct_mode=1), q, lists, k, spec, col=col, col_mode=2)
        return dict(idx=idx, score=score, flag=flag)

    probe = Probe("query_fused_lists K=2", "query_fused_lists", lambda ctx: call(ctx, "large"), lambda ctx: call(ctx, "small"), lambda: None,
                  args=lambda: lists_of("small"))
    return Case("query fused lists", lambda ctx: ctx.upload_pool(*fused_pool()), [probe])


@functools.lru_cache(maxsize=None)
def fused_pool():
    from acoss_amd import synth
    from .test_gpu_fused import _chen_tracks
    return synth.pack(_chen_tracks())


# ---- SiMPle -----------------------------------------------------------------------------------------------------------------------------------------
SIMPLE_L = 10
SIMPLE_SMALL, SIMPLE_LARGE = (11, 12, 25), (400, 400, 400, 400)


@functools.lru_cache(maxsize=None)
def simple_tracks():
    from . import _simple_ref
    rng = np.random.default_rng(10)
    return [_simple_ref.frames(rng, n, peak=0.3 * (k % 3)) for k, n in enumerate(SIMPLE_SMALL + SIMPLE_LARGE)]


def _ordered(first, count):
    return np.array([(i, j) for i in range(first, first + count) for j in range(first, first + count) if i != j], np.int32)


def _simple_probe(export):
    from . import _simple_profile_ref, _simple_ref
    small, large = _ordered(0, len(SIMPLE_SMALL)), _ordered(len(SIMPLE_SMALL), len(SIMPLE_LARGE))

    def call(ctx, pairs):
        if export == "simple_pairs":
            return dict(scores=ctx.simple_pairs(pairs, SIMPLE_L, oti=True))
        al, off, mp, mpi = ctx.simple_profile(pairs, SIMPLE_L, oti=True, profiles=True)
        return dict(records=al, offsets=off, mp=mp, mpi=mpi)

    def want():
        T = simple_tracks()
        if export == "simple_pairs":
            ref = [_simple_ref.score_exact(T[i], T[j], SIMPLE_L, True) for i, j in small]
            return dict(scores=np.array([r[0] for r in ref]), tol=np.array([_simple_ref.score_tol(T[i], T[j], SIMPLE_L, r[0]) for (i, j), r in zip(small, ref)]))
        return dict(refs=[_simple_profile_ref.reference(T[i], T[j], SIMPLE_L, True) for i, j in small])

    return Probe("%s L=%d" % (export, SIMPLE_L), export, lambda ctx: call(ctx, large), lambda ctx: call(ctx, small), want, pairs=small)


def simple_case():
    from . import _simple_ref
    return Case("simple", lambda ctx: ctx.upload_pool_f64(*_simple_ref.pool_of(simple_tracks())), [_simple_probe("simple_pairs"), _simple_probe("simple_profile")])


# ---- entry points that allocate their work buffers per call: the allocation fill does the work ---------------------------------------------------
FTM_DIRT = (75, 160)                                       # (win, beats)
FTM_PROBES = ((16, 17), (2, 2))
SNF_SMALL, SNF_LARGE = 65, 257
XF_SMALL, XF_LARGE = (12, 30), (64, 65)
GRID_FTM = (129, 257)
GRID_SERRA09 = (5, 12)


@functools.lru_cache(maxsize=None)
def ftm_track(win, nbeats):
    from .test_gpu_ftm2d import _track
    return _track(np.random.default_rng(1000 * win + nbeats), nbeats)


def _ftm_probe(win, nbeats):
    from . import _ftm2d_ref
    pwr, C = 1.96, 5.0
    call = lambda ctx, w, nb: ctx.ftm2d_debug_track(*ftm_track(w, nb), pwr, w, C)
    X, on = ftm_track(win, nbeats)
    return Probe("ftm2d_debug_track win=%d beats=%d" % (win, nbeats), "ftm2d_debug_track", lambda ctx: call(ctx, *FTM_DIRT),
                 lambda ctx: call(ctx, win, nbeats), lambda: _ftm2d_ref.stages(X, on, pwr, win, C), args=(X, on, pwr, win, C, nbeats))


@functools.lru_cache(maxsize=None)
def snf_dists(n):
    rng = np.random.default_rng(n + 3)
    out = []
    for _ in range(3):
        D = rng.random((n, n)) * 3
        lab = rng.integers(0, max(2, n // 5), n)
        D[lab[:, None] == lab[None, :]] *= 0.3             # clique structure
        out.append(D)
    return out


def _snf_probe():
    def call(ctx, n):
        Ws, fused = ctx.snf_fuse_dists(snf_dists(n), K=20, niters=5, reg_diag=1.0, want_ws=True)
        return dict(fused=fused, **{"W%d" % k: W for k, W in enumerate(Ws)})

    def want():
        import oracle
        Ws, fused = oracle.snf_fuse(snf_dists(SNF_SMALL), K=20, niters=5, reg_diag=1)        # (tests/_snf_ref.py restates it per stage)
        return dict(Ws=Ws, fused=fused)

    return Probe("snf_fuse_dists n=%d" % SNF_SMALL, "snf_fuse_dists", lambda ctx: call(ctx, SNF_LARGE), lambda ctx: call(ctx, SNF_SMALL), want)


@functools.lru_cache(maxsize=None)
def xf_triple(M, N):
    from .test_gpu_crossfusion import _triple
    return _triple(M, N)


XF_ARGS = dict(kappa=0.1, K=10, niters=5, reg_diag=1.0)


def _xf_probe():
    from . import _crossfusion_ref
    call = lambda ctx, shape: ctx.crossfusion_matrices(*xf_triple(*shape), **XF_ARGS)

    def want():
        SA, SB, C = xf_triple(*XF_SMALL)
        return _crossfusion_ref.chain(SA, SB, C, XF_ARGS["K"], XF_ARGS["niters"], XF_ARGS["reg_diag"], XF_ARGS["kappa"])

    return Probe("crossfusion_matrices %dx%d" % XF_SMALL, "crossfusion_matrices", lambda ctx: call(ctx, XF_LARGE), lambda ctx: call(ctx, XF_SMALL), want)


@functools.lru_cache(maxsize=None)
def grid_shingles(n):
    rng = np.random.default_rng(n)
    S = rng.random((n, 900)) ** 4
    S = S / np.linalg.norm(S, axis=1, keepdims=True) * rng.uniform(0.9, 1.1, (n, 1))
    S[n // 2] *= 0.2                                        # spread the scores
    return S


@functools.lru_cache(maxsize=None)
def grid_serra09_pool():
    from acoss_amd import synth
    return synth.cover_set(clique_sizes=[2] * 6, seed=12, t_range=(60, 200))


def _grid_probe(algo):
    from acoss_amd import _lib
    from . import _ftm2d_ref

    def upload(ctx, n):
        if algo == "ftm2d":
            ctx.ftm2d_upload_shingles(grid_shingles(n))
        else:
            d = grid_serra09_pool()
            ctx.upload_pool(d["frames"][:d["offsets"][n]], d["offsets"][:n + 1])

    def call(ctx, n):
        upload(ctx, n)
        D = np.zeros((n, n), np.float32)
        ctx.pair_grid(_lib.ALGO_FTM2D if algo == "ftm2d" else _lib.ALGO_SERRA09, True, None if algo == "ftm2d" else _lib.serra09_params(), [D],
                      mirror=True)
        return dict(D=D)

    small, large = GRID_FTM if algo == "ftm2d" else GRID_SERRA09

    def want():
        """The WHOLE matrix: the mirrored scores of the pairs i < j, and 0 in the cells no pair writes (the diagonal)."""
        import oracle
        i, j = np.triu_indices(small, 1)
        pairs = np.stack([i, j], 1).astype(np.int32)
        if algo == "ftm2d":
            sc = _ftm2d_ref.pair_scores(grid_shingles(small), pairs).astype(np.float32)
        else:
            d = grid_serra09_pool()
            sc = oracle.serra09_pairs(d["frames"][:d["offsets"][small]], d["offsets"][:small + 1], pairs)
        D = np.zeros((small, small), np.float32)
        D[i, j] = sc
        D[j, i] = sc
        return dict(D=D)

    return Probe("pair_grid %s n=%d" % (algo, small), "pair_grid_" + algo, lambda ctx: call(ctx, large), lambda ctx: call(ctx, small), want)


def per_call_case():
    return Case("per-call buffers", lambda ctx: None,
                [_ftm_probe(*s) for s in FTM_PROBES] + [_snf_probe(), _xf_probe(), _grid_probe("ftm2d"), _grid_probe("serra09")])


def cpu_cases():
    """The cases whose references the CPU gives (every one but the EarlyFusion product path)."""
    return [serra09_product_case(), serra09_one_list_case(), serra09_align_case(), serra09_plots_case(), ef_stand_alone_case(), rank_case(),
            query_case(), simple_case(), per_call_case()]
