"""
Host-side checks of the sixteen alignment wrappers of acoss_amd._lib.Context (ef_align, ef_align_long, sw_align_binary,
sw_align_long_binary, qmax_locate_binary, dmax_locate_binary, qmax_path_binary, dmax_path_binary, serra09_align,
serra09_align_paths, chenfusion_align, chenfusion_align_paths, serra09_align_sections, ef_align_sections, qmax_sections_binary,
sw_sections_binary): which export each reaches, with which arguments, and what it hands back.  No library is loaded and no
GPU is touched: a stand-in for Context._L records every call and fills plausible outputs.
"""
import ctypes

import numpy as np
import pytest

from acoss_amd import _lib

REC = (2.5, 2, 3, 4, 5)          # the record the stand-in writes into every element of `out`
NO_MATCH = (0.0, -1, -1, -1, -1)  # ... and behind the sections of a pair


def _write(addr, ctype, values):
    arr = (ctype * len(values)).from_address(addr)
    for k, v in enumerate(values):
        arr[k] = v


class FakeLib(object):
    """Every attribute is an export: the call is recorded as (name, args) and the outputs are filled from the arguments' layout."""
    LIST = {"acx_ef_align": 5, "acx_ef_align_long": 5, "acx_chenfusion_align_paths": 5, "acx_serra09_align_paths": 4}    # index of `out`
    PLOT_N_LAST = ("acx_sw_align_binary", "acx_sw_align_long_binary")          # (.., out, cells, cap, n_cells)
    PLOT_N_FIRST = ("acx_qmax_path_binary", "acx_dmax_path_binary")            # (.., params, out, n_cells, cells, cap)
    LOCATE = ("acx_qmax_locate_binary", "acx_dmax_locate_binary")              # (.., params, out)
    RECORDS = {"acx_serra09_align": 4, "acx_chenfusion_align": 5}              # (ctx, pairs, K, .., out): index of `out`
    # (.., opts, out, counts, path_off, cells, cap): index of `opts`; the list forms over args[2] pairs, the plot forms over one
    SECTIONS = {"acx_serra09_align_sections": 4, "acx_ef_align_sections": 5, "acx_qmax_sections_binary": 5, "acx_sw_sections_binary": 4}

    def __init__(self):
        self.calls = []

    def acx_last_error(self, h):
        return b"stand-in"

    def acx_serra09_embed_len(self, T, pref):
        p = pref._obj
        return int(T) - (p.m - 1) * p.tau

    def __getattr__(self, name):
        if not name.startswith("acx_"):
            raise AttributeError(name)

        def export(*args):
            self.calls.append((name, args))
            if name in self.RECORDS:
                assert len(args) == self.RECORDS[name] + 1, name
                rec = np.array([REC] * args[2], _lib.ALIGNMENT_DTYPE)
                ctypes.memmove(args[-1], rec.ctypes.data, rec.nbytes)
            elif name in self.SECTIONS:
                # pair k has min(S, k + 1) sections of one cell each while the buffer lasts
                K, o = (1 if name.endswith("_binary") else args[2]), self.SECTIONS[name]
                assert len(args) == o + 6, name
                S = args[o]._obj.max_sections
                out, cnt, off, cells, cap = args[o + 1:o + 6]
                n = [min(S, k + 1) for k in range(K)]
                rec = np.array([[REC if s < n[k] else NO_MATCH for s in range(S)] for k in range(K)], _lib.ALIGNMENT_DTYPE).reshape(K, S)
                ctypes.memmove(out, rec.ctypes.data, rec.nbytes)
                _write(cnt, ctypes.c_int32, n)
                if off is not None:
                    offs, used = [0], 0
                    for k in range(K):
                        for s in range(S):
                            used += 1 if s < n[k] and used < cap else 0
                            offs.append(used)
                    _write(off, ctypes.c_int64, offs)
                    _write(cells, ctypes.c_int32, [7 + k for k in range(2 * used)])
            elif name in self.LIST:
                K, o = args[2], self.LIST[name]
                out, off, cells, cap = args[o:o + 4]
                _write(out, ctypes.c_int32, [0] * (5 * K))
                rec = np.array([REC] * K, _lib.ALIGNMENT_DTYPE)
                ctypes.memmove(out, rec.ctypes.data, rec.nbytes)
                if off is not None:                     # one cell per pair while the buffer lasts
                    n = min(K, cap)
                    _write(off, ctypes.c_int64, [min(k, n) for k in range(K + 1)])
                    _write(cells, ctypes.c_int32, [7 + k for k in range(2 * n)])
            else:
                if name in self.PLOT_N_LAST:
                    out, cells, cap, nref = args[4:8]
                elif name in self.PLOT_N_FIRST:
                    out, nref, cells, cap = args[5:9]
                else:
                    assert name in self.LOCATE, name
                    out, cells, cap, nref = args[5], None, 0, None
                rec = np.array([REC], _lib.ALIGNMENT_DTYPE)
                ctypes.memmove(out, rec.ctypes.data, rec.nbytes)
                if cells is not None:
                    n = min(2, cap)
                    _write(cells, ctypes.c_int32, [7 + k for k in range(2 * n)])
                    nref._obj.value = n
            return _lib.ACX_OK
        return export


def _ctx(ef_blocks=None, lengths=None):
    c = _lib.Context.__new__(_lib.Context)        # no acx_create: no library, no device
    c._L = FakeLib()
    c._h = 1234
    c.lengths = lengths
    if ef_blocks is not None:
        c.ef_blocks = ef_blocks
    return c


def _last(c):
    assert len(c._L.calls) == 1
    return c._L.calls[0]


def _check_records(out, K):
    assert out.dtype == _lib.ALIGNMENT_DTYPE and out.shape == (K,)
    assert all(tuple(r) == REC for r in out)


PAIRS = [(0, 1), (2, 0), (1, 1)]
BLOCKS = np.array([5, 9, 3])                      # min(M, N) over PAIRS: 5 + 3 + 9 = 17


@pytest.mark.parametrize("method,export", [("ef_align", "acx_ef_align"), ("ef_align_long", "acx_ef_align_long")])
def test_ef_list_wrappers(method, export):
    # the records alone: NULL path pointers, cap 0
    c = _ctx(BLOCKS)
    out = getattr(c, method)(PAIRS, kappa=0.25, K=7, plane=2)
    name, a = _last(c)
    assert name == export and len(a) == 9 and a[0] == 1234
    assert [a[1][k] for k in range(6)] == [0, 1, 2, 0, 1, 1] and a[2] == 3
    assert a[3]._obj.kappa == 0.25 and a[3]._obj.K == 7 and a[4] == 2
    assert a[6] is None and a[7] is None and a[8] == 0
    _check_records(out, 3)
    # the defaults
    c = _ctx(BLOCKS)
    getattr(c, method)(PAIRS)
    a = _last(c)[1]
    assert abs(a[3]._obj.kappa - 0.1) < 1e-12 and a[3]._obj.K == 10 and a[4] == 3 and a[6] is None
    # the paths, a pool this object saw: the sum of min(M, N); an index out of range counts nothing (the library refuses the list)
    c = _ctx(BLOCKS)
    out, off, cells = getattr(c, method)(PAIRS + [(0, 3)], paths=True)
    name, a = _last(c)
    assert name == export and a[2] == 4 and a[6] is not None and a[7] is not None and a[8] == 17
    _check_records(out, 4)
    assert off.dtype == np.int64 and off.tolist() == [0, 1, 2, 3, 4]
    assert cells.dtype == np.int32 and cells.shape == (4, 2) and cells.ravel().tolist() == list(range(7, 15))
    # a given cap goes through as it is, whatever the pool
    for blocks in (BLOCKS, None):
        c = _ctx(blocks)
        out, off, cells = getattr(c, method)(PAIRS, paths=True, cap=2)
        a = _last(c)[1]
        assert a[8] == 2 and off.tolist() == [0, 1, 2, 2] and cells.shape == (2, 2)
    # an empty list
    c = _ctx(BLOCKS)
    out, off, cells = getattr(c, method)(np.zeros((0, 2), np.int32), paths=True)
    a = _last(c)[1]
    assert a[2] == 0 and a[8] == 0 and out.shape == (0,) and off.tolist() == [0] and cells.shape == (0, 2)


def test_ef_cap_rules_for_an_unseen_pool():
    # ef_align: 1024 cells a pair, the bound of any list the bit path accepts
    c = _ctx(None)
    out, off, cells = c.ef_align(PAIRS, paths=True)
    name, a = _last(c)
    assert name == "acx_ef_align" and a[8] == 1024 * 3
    assert off.tolist() == [0, 1, 2, 3] and cells.shape == (3, 2)
    # ef_align_long: no bound without the block counts, and no call
    c = _ctx(None)
    with pytest.raises(ValueError, match="ef_align_long: .*cap must be given"):
        c.ef_align_long(PAIRS, paths=True)
    assert c._L.calls == []
    # ... the records alone need none
    _check_records(c.ef_align_long(PAIRS), 3)
    assert _last(c)[0] == "acx_ef_align_long"


LENGTHS = [30, 50, 20]


@pytest.mark.parametrize("method,export,plane", [("serra09_align_paths", "acx_serra09_align_paths", None),
                                                 ("chenfusion_align_paths", "acx_chenfusion_align_paths", 0),
                                                 ("chenfusion_align_paths", "acx_chenfusion_align_paths", 1)])
def test_serra09_list_wrappers(method, export, plane):
    p = _lib.serra09_params(m=4, tau=2)           # embedded lengths: T - 6 = 24, 44, 14
    kw = {} if plane is None else {"plane": plane}
    o = 4 if plane is None else 5
    c = _ctx(lengths=LENGTHS)
    out, off, cells = getattr(c, method)(PAIRS + [(3, 0)], params=p, **kw)
    name, a = _last(c)
    assert name == export and len(a) == o + 4 and a[0] == 1234
    assert [a[1][k] for k in range(8)] == [0, 1, 2, 0, 1, 1, 3, 0] and a[2] == 4
    assert a[3]._obj is p
    if plane is not None:
        assert a[4] == plane
    assert a[o + 1] is not None and a[o + 2] is not None and a[o + 3] == 24 + 14 + 44      # (track 3 does not exist: 0 cells)
    _check_records(out, 4)
    assert off.dtype == np.int64 and off.tolist() == [0, 1, 2, 3, 4]
    assert cells.dtype == np.int32 and cells.shape == (4, 2)
    # a given cap: nothing is worked out (no lengths are needed), the default parameters are serra09_params()
    c = _ctx(lengths=None)
    out, off, cells = getattr(c, method)(PAIRS, cap=1, **kw)
    name, a = _last(c)
    assert name == export and a[o + 3] == 1 and a[3]._obj.m == 9 and a[3]._obj.tau == 1
    assert off.tolist() == [0, 1, 1, 1] and cells.shape == (1, 2)


PLOT = np.arange(42).reshape(6, 7) % 2


@pytest.mark.parametrize("method", ["sw_align_binary", "sw_align_long_binary"])
def test_sw_plot_wrappers(method):
    export = "acx_" + method
    c = _ctx()
    out, cells = getattr(c, method)(PLOT)
    name, a = _last(c)
    assert name == export and len(a) == 8 and a[0] == 1234 and a[2] == 6 and a[3] == 7
    assert [a[1][k] for k in range(42)] == PLOT.ravel().tolist()
    assert a[5] is not None and a[6] == 6 and a[7]._obj.value == 2
    _check_records(out, 1)
    assert cells.dtype == np.int32 and cells.shape == (2, 2) and cells.ravel().tolist() == [7, 8, 9, 10]
    # the record alone
    c = _ctx()
    out = getattr(c, method)(PLOT, paths=False)
    name, a = _last(c)
    assert name == export and a[5] is None and a[6] == 0 and a[7] is None
    _check_records(out, 1)
    # a given cap
    c = _ctx()
    out, cells = getattr(c, method)(PLOT.T, cap=1)
    a = _last(c)[1]
    assert a[2] == 7 and a[3] == 6 and a[6] == 1 and cells.shape == (1, 2)
    with pytest.raises(ValueError, match=r"^%s: B must be \(M, N\), got shape \(3,\)$" % method):
        getattr(c, method)(np.zeros(3))
    assert len(c._L.calls) == 1


@pytest.mark.parametrize("method", ["qmax_locate_binary", "dmax_locate_binary"])
def test_locate_plot_wrappers(method):
    c = _ctx()
    p = _lib.serra09_params(gamma_o=0.75)
    out = getattr(c, method)(PLOT, p)
    name, a = _last(c)
    assert name == "acx_" + method and len(a) == 6 and a[0] == 1234 and a[2] == 6 and a[3] == 7 and a[4]._obj is p
    assert [a[1][k] for k in range(42)] == PLOT.ravel().tolist()
    _check_records(out, 1)
    c = _ctx()
    getattr(c, method)(PLOT)
    assert _last(c)[1][4]._obj.gamma_o == 0.5
    with pytest.raises(ValueError, match=r"^%s: R must be \(M, N\), got shape \(2, 2, 2\)$" % method):
        getattr(c, method)(np.zeros((2, 2, 2)))
    assert len(c._L.calls) == 1


@pytest.mark.parametrize("method", ["qmax_path_binary", "dmax_path_binary"])
def test_path_plot_wrappers(method):
    c = _ctx()
    p = _lib.serra09_params(gamma_e=0.25)
    out, cells = getattr(c, method)(PLOT, p)
    name, a = _last(c)
    assert name == "acx_" + method and len(a) == 9 and a[0] == 1234 and a[2] == 6 and a[3] == 7 and a[4]._obj is p
    assert [a[1][k] for k in range(42)] == PLOT.ravel().tolist()
    assert a[6]._obj.value == 2 and a[7] is not None and a[8] == 6
    _check_records(out, 1)
    assert cells.dtype == np.int32 and cells.shape == (2, 2) and cells.ravel().tolist() == [7, 8, 9, 10]
    c = _ctx()
    out, cells = getattr(c, method)(PLOT, cap=0)
    a = _last(c)[1]
    assert a[4]._obj.gamma_e == 0.5 and a[8] == 0 and cells.shape == (0, 2)
    with pytest.raises(ValueError, match=r"^%s: R must be \(M, N\), got shape \(4,\)$" % method):
        getattr(c, method)(np.zeros(4))
    assert len(c._L.calls) == 1


# ---------------------------------------------------------------------- the records-only list forms
@pytest.mark.parametrize("method,export,plane", [("serra09_align", "acx_serra09_align", None), ("chenfusion_align", "acx_chenfusion_align", 0),
                                                 ("chenfusion_align", "acx_chenfusion_align", 1)])
def test_records_only_list_wrappers(method, export, plane):
    p = _lib.serra09_params(m=4, tau=2)
    kw = {} if plane is None else {"plane": plane}
    c = _ctx(lengths=None)                                  # (no lengths are needed: there is no cap to work out)
    out = getattr(c, method)(PAIRS + [(3, 0)], params=p, **kw)
    name, a = _last(c)
    assert name == export and len(a) == (5 if plane is None else 6) and a[0] == 1234
    assert [a[1][k] for k in range(8)] == [0, 1, 2, 0, 1, 1, 3, 0] and a[2] == 4 and a[3]._obj is p
    if plane is not None:
        assert a[4] == plane
    assert a[-1] == out.ctypes.data
    _check_records(out, 4)
    # the defaults: serra09_params(), and chenfusion_align's plane 0
    c = _ctx(lengths=None)
    out = getattr(c, method)(np.array(PAIRS, np.int64))
    name, a = _last(c)
    assert name == export and a[3]._obj.m == 9 and a[3]._obj.tau == 1 and a[2] == 3
    if plane is not None:
        assert a[4] == 0
    _check_records(out, 3)
    # an empty list
    c = _ctx(lengths=None)
    out = getattr(c, method)(np.zeros((0, 2), np.int32), **kw)
    assert _last(c)[1][2] == 0 and out.shape == (0,) and out.dtype == _lib.ALIGNMENT_DTYPE


# ---------------------------------------------------------------------- the sections forms
S_PAIRS = [(0, 1), (1, 2), (1, 3), (4, 0), (2, 2)]            # (track 4 does not exist: it counts nothing)
S_M = [24, 94, 14, 5]                                         # rows / columns of the tracks' plots
S_LENGTHS = [M + 6 for M in S_M]                              # the stand-in's embedded length at m = 4, tau = 2: T - 6
S_CAP = {1: 24 + 14 + 5 + 14, 4: 24 + 56 + 20 + 14, 16: 24 + 94 + 80 + 14}      # sum of min(Mq, S min(Mq, Mr))


def _serra09_sections(c, S, **kw):
    p = _lib.serra09_params(m=4, tau=2)
    return p, c.serra09_align_sections(S_PAIRS, p, _lib.section_opts("t", S, 3.5, 0.25, 2), **kw)


def _ef_sections(c, S, **kw):
    return None, c.ef_align_sections(S_PAIRS, 0.25, 7, 2, _lib.section_opts("t", S, 3.5, 0.25, 2), **kw)


def _check_opts(oref, S):
    o = oref._obj
    assert (o.max_sections, o.pad, o.min_score, o.min_ratio) == (S, 2, 3.5, 0.25)


def _check_section_records(out, n, K, S):
    assert out.dtype == _lib.ALIGNMENT_DTYPE and out.shape == (K, S)
    assert n.dtype == np.int32 and n.tolist() == [min(S, k + 1) for k in range(K)]
    for k in range(K):
        assert [tuple(r) for r in out[k]] == [REC] * n[k] + [NO_MATCH] * (S - n[k])


@pytest.mark.parametrize("S", [1, 4, 16])
@pytest.mark.parametrize("call,export,o", [(_serra09_sections, "acx_serra09_align_sections", 4), (_ef_sections, "acx_ef_align_sections", 5)])
def test_sections_list_wrappers(call, export, o, S):
    K = len(S_PAIRS)
    # the records alone: NULL path pointers, cap 0
    c = _ctx(ef_blocks=np.array(S_M), lengths=S_LENGTHS)
    p, got = call(c, S)
    name, a = _last(c)
    assert name == export and len(a) == o + 6 and a[0] == 1234
    assert [a[1][k] for k in range(2 * K)] == [t for pr in S_PAIRS for t in pr] and a[2] == K
    if p is not None:
        assert a[3]._obj is p
    else:
        assert a[3]._obj.kappa == 0.25 and a[3]._obj.K == 7 and a[4] == 2
    _check_opts(a[o], S)
    assert a[o + 3] is None and a[o + 4] is None and a[o + 5] == 0
    assert isinstance(got, tuple) and len(got) == 2
    assert a[o + 1] == got[0].ctypes.data and a[o + 2] == got[1].ctypes.data
    _check_section_records(got[0], got[1], K, S)
    # the paths: the default cap, the offsets of all K S sections, the cells cut at the last offset
    c = _ctx(ef_blocks=np.array(S_M), lengths=S_LENGTHS)
    p, got = call(c, S, paths=True)
    name, a = _last(c)
    assert name == export and a[o + 3] is not None and a[o + 4] is not None and a[o + 5] == S_CAP[S]
    assert isinstance(got, tuple) and len(got) == 4
    out, n, off, cells = got
    _check_section_records(out, n, K, S)
    assert off.dtype == np.int64 and off.shape == (K * S + 1,) and a[o + 3] == off.ctypes.data
    total = int(n.sum())
    assert off[-1] == total and np.diff(off).tolist() == [1 if s < n[k] else 0 for k in range(K) for s in range(S)]
    assert cells.dtype == np.int32 and cells.shape == (total, 2) and cells.ravel().tolist() == list(range(7, 7 + 2 * total))
    # a given cap goes through as it is: nothing is worked out (no lengths, no block counts)
    c = _ctx()
    p, got = call(c, S, paths=True, cap=2)
    a = _last(c)[1]
    assert a[o + 5] == 2 and got[2][-1] == 2 and got[3].shape == (2, 2)
    c = _ctx()
    p, got = call(c, S, paths=True, cap=0)
    a = _last(c)[1]
    assert a[o + 5] == 0 and a[o + 4] is not None and got[2].tolist() == [0] * (K * S + 1) and got[3].shape == (0, 2)


@pytest.mark.parametrize("S", [1, 4, 16])
def test_ef_sections_cap_for_an_unseen_pool(S):
    c = _ctx(None)
    _, got = _ef_sections(c, S, paths=True)
    name, a = _last(c)
    assert name == "acx_ef_align_sections" and a[10] == 1024 * len(S_PAIRS)
    assert got[3].shape == (int(got[1].sum()), 2)


def test_sections_list_defaults_and_empty_lists():
    c = _ctx(ef_blocks=np.array(S_M), lengths=S_LENGTHS)
    out, n = c.serra09_align_sections(PAIRS)
    a = _last(c)[1]
    assert a[3]._obj.m == 9 and a[3]._obj.tau == 1
    o = a[4]._obj
    assert (o.max_sections, o.pad, o.min_score, o.min_ratio) == (4, 0, 2.0, 0.0) and out.shape == (3, 4) and a[9] == 0
    c = _ctx(ef_blocks=np.array(S_M))
    out, n = c.ef_align_sections(PAIRS)
    a = _last(c)[1]
    assert abs(a[3]._obj.kappa - 0.1) < 1e-12 and a[3]._obj.K == 10 and a[4] == 3
    o = a[5]._obj
    assert (o.max_sections, o.pad, o.min_score, o.min_ratio) == (4, 0, 2.0, 0.0) and out.shape == (3, 4) and a[10] == 0
    for method in ("serra09_align_sections", "ef_align_sections"):
        c = _ctx(ef_blocks=np.array(S_M), lengths=S_LENGTHS)
        out, n, off, cells = getattr(c, method)(np.zeros((0, 2), np.int32), paths=True)
        a = _last(c)[1]
        assert a[2] == 0 and a[-1] == 0 and out.shape == (0, 4) and n.shape == (0,) and off.tolist() == [0] and cells.shape == (0, 2)


TALL = np.arange(60).reshape(20, 3) % 2           # min(M, S min(M, N)): 3, 12, 20
WIDE = np.arange(60).reshape(3, 20) % 2           # 3 whatever S


@pytest.mark.parametrize("S", [1, 4, 16])
@pytest.mark.parametrize("method,o", [("qmax_sections_binary", 5), ("sw_sections_binary", 4)])
def test_sections_plot_wrappers(method, o, S):
    export = "acx_" + method
    opts = _lib.section_opts("t", S, 3.5, 0.25, 2)
    p = _lib.serra09_params(gamma_o=0.75)
    pre = (p,) if o == 5 else ()
    # paths=True is the default: (records (S,), count, offsets (S + 1,), cells)
    c = _ctx()
    got = getattr(c, method)(TALL, *pre, opts)
    name, a = _last(c)
    assert name == export and len(a) == o + 6 and a[0] == 1234 and a[2] == 20 and a[3] == 3
    assert [a[1][k] for k in range(60)] == TALL.ravel().tolist()
    if o == 5:
        assert a[4]._obj is p
    _check_opts(a[o], S)
    assert a[o + 3] is not None and a[o + 4] is not None and a[o + 5] == {1: 3, 4: 12, 16: 20}[S]
    assert isinstance(got, tuple) and len(got) == 4
    out, n, off, cells = got
    assert out.dtype == _lib.ALIGNMENT_DTYPE and out.shape == (S,) and [tuple(r) for r in out] == [REC] + [NO_MATCH] * (S - 1)
    assert type(n) is int and n == 1
    assert off.dtype == np.int64 and off.tolist() == [0] + [1] * S
    assert cells.dtype == np.int32 and cells.shape == (1, 2) and cells.ravel().tolist() == [7, 8]
    c = _ctx()
    getattr(c, method)(WIDE, *pre, opts)
    assert _last(c)[1][o + 5] == 3
    # the records alone
    c = _ctx()
    got = getattr(c, method)(TALL, *pre, opts, paths=False)
    name, a = _last(c)
    assert name == export and a[o + 3] is None and a[o + 4] is None and a[o + 5] == 0
    assert isinstance(got, tuple) and len(got) == 2 and got[0].shape == (S,) and tuple(got[0][0]) == REC and type(got[1]) is int and got[1] == 1
    # a given cap
    c = _ctx()
    out, n, off, cells = getattr(c, method)(TALL, *pre, opts, cap=0)
    assert _last(c)[1][o + 5] == 0 and off.tolist() == [0] * (S + 1) and cells.shape == (0, 2)


@pytest.mark.parametrize("method,what", [("qmax_sections_binary", "R"), ("sw_sections_binary", "B")])
def test_sections_plot_defaults_and_shape_errors(method, what):
    c = _ctx()
    getattr(c, method)(PLOT)
    a = _last(c)[1]
    o = a[-6]._obj
    assert (o.max_sections, o.pad, o.min_score, o.min_ratio) == (4, 0, 2.0, 0.0) and a[-1] == 6
    if what == "R":
        assert a[4]._obj.gamma_o == 0.5
    for bad, shape in ((np.zeros(3), r"\(3,\)"), (np.zeros((2, 2, 2)), r"\(2, 2, 2\)")):
        with pytest.raises(ValueError, match=r"^%s: %s must be \(M, N\), got shape %s$" % (method, what, shape)):
            getattr(c, method)(bad)
    assert len(c._L.calls) == 1
