"""
Host-side checks of the ten alignment wrappers of acoss_amd._lib.Context (ef_align, ef_align_long, sw_align_binary,
sw_align_long_binary, qmax_locate_binary, dmax_locate_binary, qmax_path_binary, dmax_path_binary, serra09_align_paths,
chenfusion_align_paths): which export each reaches, with which arguments, and what it hands back.  No library is loaded and no
GPU is touched: a stand-in for Context._L records every call and fills plausible outputs.
"""
import ctypes

import numpy as np
import pytest

from acoss_amd import _lib

REC = (2.5, 2, 3, 4, 5)          # the record the stand-in writes into every element of `out`


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
            if name in self.LIST:
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
