"""
Host-only checks of Simple.align / profile / align_matches: every argument error comes before the first library call (the
checks of acoss_amd/algorithms/_align.py), empty lists have empty answers, and an empty slot is a no-match row.
"""
import numpy as np
import pytest


class _NoDevice(object):
    """Stands where the class's libacx context would be: any use is a test failure."""
    def __getattr__(self, name):
        raise AssertionError("the library was reached (%s) before the arguments were checked" % name)


@pytest.fixture
def algo(tmp_path, monkeypatch):
    from acoss_amd.algorithms import Simple
    monkeypatch.chdir(tmp_path)
    path = tmp_path / "ds.csv"
    with open(path, "w") as f:
        f.write("work_id,track_id\n")
        for i in range(8):
            f.write("w%d,t%d\n" % (i // 2, i))
    a = Simple(str(path), "feat/", shortname="args")
    a._ctx = _NoDevice()
    monkeypatch.setattr(Simple, "_context", lambda self: (_ for _ in ()).throw(AssertionError("pool upload before the argument checks")))
    yield a
    a._ctx = None
    a.cleanup_memmap()


def test_argument_errors_come_first(algo):
    for who in ("align", "profile"):
        call = getattr(algo, who)
        with pytest.raises(ValueError, match=r"%s: idxs must be \(K, 2\)" % who):
            call([0, 1, 2])
        with pytest.raises(ValueError, match=r"%s: idxs must be \(K, 2\)" % who):
            call(np.zeros((2, 3), np.int64))
        with pytest.raises(ValueError, match=r"%s: idxs must be track indices in \[0, 8\)" % who):
            call([[0, 8]])
        with pytest.raises(ValueError, match=r"%s: idxs must be track indices in \[0, 8\)" % who):
            call([[-1, 2]])
        with pytest.raises(ValueError, match="%s: track indices must be integers" % who):
            call([[0.5, 1.0]])
    with pytest.raises(ValueError, match=r"align_matches: indices must be \(Q, k\) with one row per query \(2\)"):
        algo.align_matches([0, 1], np.zeros((3, 2), np.int32))
    with pytest.raises(ValueError, match=r"align_matches: queries must be track indices in \[0, 8\)"):
        algo.align_matches([0, 8], np.zeros((2, 2), np.int32))
    with pytest.raises(ValueError, match=r"align_matches: indices must be track indices in \[0, 8\) or -1"):
        algo.align_matches([0, 1], np.array([[1, -2], [0, 3]]))
    with pytest.raises(ValueError, match=r"align_matches: indices must be track indices in \[0, 8\) or -1"):
        algo.align_matches([0, 1], np.array([[1, 8], [0, 3]]))
    with pytest.raises(ValueError, match="align_matches: track indices must be integers"):
        algo.align_matches([0, 1], np.array([[1.0, 2.0], [0.0, 3.0]]))


def test_empty_lists_and_empty_slots_need_no_device(algo):
    from acoss_amd import _lib
    assert algo.ALIGN_DTYPE == _lib.SIMPLE_ALIGNMENT_DTYPE
    al = algo.align(np.zeros((0, 2), np.int64))
    assert al.shape == (0,) and al.dtype == algo.ALIGN_DTYPE
    al, mps, mpis = algo.profile([])
    assert al.shape == (0,) and mps == [] and mpis == []
    got = algo.align_matches([3, 5], np.full((2, 4), -1, np.int32))
    assert got.shape == (2, 4) and got.dtype == algo.ALIGN_DTYPE
    assert np.all(got["run_len"] == 0) and np.all(np.isnan(got["score"])) and np.all(np.isnan(got["best_dist"]))
    for f in ("best_q", "best_r", "q0", "r0", "q1", "r1", "q_span", "r_span"):
        assert np.all(got[f] == -1), f
    assert np.all(got["shift"] == 0)
    assert algo.align_matches([], np.zeros((0, 5), np.int32)).shape == (0, 5)
