"""The reference ranking (tests/sc_rank_ref.py) on a 12-context database whose answer is known by construction: what
tests/test_sc_rank_gpu.py holds the device against must itself be right about ties, empty contexts, the excluded recent ones and
the direction of the distance."""
import numpy as np
import pytest

import oracle
from tests import sc_rank_ref as R

DBL_MAX = R.DBL_MAX
EXCL = 2


@pytest.fixture(scope="module")
def db():
    """0: A   1: B   2: A again   3: no point   4: C   5: A turned by 3 sectors   6 .. 11: six more places"""
    a = R.make_scan(1, reach=75.0)
    clouds = [a, R.make_scan(2), a.copy(), np.zeros((0, 8), np.float32), R.make_scan(3), R.rotate_sectors(a, 3)]
    clouds += [R.make_scan(10 + i) for i in range(6)]
    orc = oracle.ScanContextOracle(num_exclude_recent=EXCL)
    for c in clouds:
        orc.add(c)
    return orc


def test_no_candidates_while_q_is_not_past_the_excluded_ones(db):
    idx, dist, shift = R.rank(db, 0, 12, 3)
    assert idx.shape == dist.shape == shift.shape == (12, 3) and idx.dtype == np.int64 and shift.dtype == np.int32
    for q in range(EXCL + 1):                                          # q <= num_exclude_recent
        assert (idx[q] == -1).all() and (dist[q] == DBL_MAX).all() and (shift[q] == 0).all()
    assert idx[3, 0] == 0 and (idx[3, 1:] == -1).all()                 # q = 3: one candidate, then the tail
    assert (idx[4, :2] >= 0).all() and idx[4, 2] == -1 and dist[4, 2] == DBL_MAX and shift[4, 2] == 0
    assert (idx[5:] >= 0).all()
    for q in range(12):
        assert (idx[q] < max(0, q - EXCL)).all()


def test_identical_contexts_tie_and_the_lower_index_comes_first(db):
    idx, dist, shift = R.rank(db, 5, 1, 3)                             # A turned: candidates 0 (A), 1 (B), 2 (A)
    assert idx[0].tolist() == [0, 2, 1]
    assert dist[0, 0] == dist[0, 1] == db.distance(5, 0)[0] and dist[0, 0] < 0.2 < dist[0, 2]
    assert shift[0, 0] == shift[0, 1] == 3
    # ... and in every later row the two copies of A stand next to each other, 0 before 2
    idx, dist, _ = R.rank(db, 6, 6, 8)
    for row in range(6):
        at = idx[row].tolist()
        assert at.index(2) == at.index(0) + 1 and dist[row, at.index(0)] == dist[row, at.index(2)]


def test_an_empty_context_is_a_candidate_at_dbl_max_and_sorts_last(db):
    assert db.distance(6, 3) == (DBL_MAX, 0)
    idx, dist, shift = R.rank(db, 6, 1, 8)                             # candidates 0 .. 3
    assert idx[0, 3] == 3 and dist[0, 3] == DBL_MAX and shift[0, 3] == 0
    assert (dist[0, :3] < 1.0).all() and (idx[0, 4:] == -1).all() and (dist[0, 4:] == DBL_MAX).all()
    idx, dist, shift = R.rank(db, 3, 1, 2)                             # the empty context as the query: its candidate counts, at DBL_MAX
    assert idx[0].tolist() == [0, -1] and (dist[0] == DBL_MAX).all() and (shift[0] == 0).all()


def test_rows_are_sorted_and_the_query_is_the_unshifted_side(db):
    idx, dist, shift = R.rank(db, 0, 12, 8)
    for q in range(12):
        n = max(0, min(8, q - EXCL))
        keys = [(dist[q, r], idx[q, r]) for r in range(n)]
        assert keys == sorted(keys)
        for r in range(n):
            assert (dist[q, r], shift[q, r]) == db.distance(q, int(idx[q, r]))
    # distance(q, i) is not distance(i, q): A turned by 3 sectors finds A at shift 3, A finds it at shift 57
    assert db.distance(5, 0)[1] == 3 and db.distance(0, 5)[1] == 57
    assert shift[5, 0] == 3
    assert any(db.distance(q, i)[0] != db.distance(i, q)[0] for q in range(6, 12) for i in range(q - EXCL))


def test_find_loops_applies_the_threshold_and_forms_the_yaw(db):
    loops = R.find_loops(db, 0, 12)
    assert [l[0] for l in loops] == list(range(12))
    for q in range(EXCL + 1):
        assert loops[q] == (q, -1, np.float32(0), None)
    q, match, yaw, d = loops[5]
    assert (match, d) == (0, db.distance(5, 0)[0]) and d <= 0.4
    assert yaw.dtype == np.float32 and yaw == np.float32(np.deg2rad(18.0))
    _, match, yaw, d = loops[3]                                        # the empty query: a candidate, but at DBL_MAX
    assert (match, yaw, d) == (-1, np.float32(0), DBL_MAX)
    for q, match, yaw, d in loops[6:]:                                 # other places: the best candidate is reported, the match refused
        assert d == min(db.distance(q, i)[0] for i in range(q - EXCL))
        assert (match >= 0) == (d <= float(db.dist_thres)) and (match >= 0 or yaw == 0)
    table = R.pair_table(db)
    assert R.find_loops(db, 4, 5, table) == loops[4:9]


def test_the_entry_point_is_exported_declared_and_its_check_program_built():
    import os
    from simpleslam_amd import pcr
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = pcr.load_library()
    header = open(os.path.join(root, "include", "pcr_hip.h")).read()
    for name in ("pcr_sc_rank_stored", "pcr_sc_shift_yaw"):
        assert name in pcr.ABI_SYMBOLS and hasattr(lib, name) and f" {name}(" in header
    assert callable(pcr.ScanContext.rankStored) and callable(pcr.ScanContext.findLoops)
    assert os.path.exists(os.path.join(root, "simpleslam_amd", "lib", "sc_loops_check")), "sc_loops_check not built (run __graft_entry__.build())"
    # host-only: the yaw helper is the reference's deg2rad<float>(6 * shift)
    for s in (0, 1, 3, 11, 59):
        assert np.float32(lib.pcr_sc_shift_yaw(s)) == R.shift_yaw(s)
    # a null handle is an error, never a crash
    assert lib.pcr_sc_rank_stored(None, 0, 0, 1, None, None, None) == 1
