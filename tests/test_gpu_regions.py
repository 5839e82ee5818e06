"""-m gpu tests of the region merge's kernels alone: al_dbg_regions_merge (the device list, the merge sort, the segmented max-scan, the head sum and
k_reg_compact) on the case lists of regions_cases.py against the plain restatement and against the host twin, per gap and merged across the gaps, appended
all at once and 64 / 1000 intervals at a time with a fold after each append (the fold between batches)."""
import ctypes as C

import numpy as np
import pytest

import regions_cases as rc

pytestmark = pytest.mark.gpu
CASES = {name: (v, names) for name, v, names in rc.cases()}
_want = {}


def _tap(fn, v, names, chunk, per_gap):
    rk, _ = rc.ranks(names)
    a = np.array([(g, rk[c], s, e) for g, c, s, e in v], dtype=np.uint32).reshape(-1, 4)
    cols = [np.ascontiguousarray(a[:, j]) for j in range(4)]
    out = [np.zeros(len(v) + 1, dtype=np.uint32) for _ in range(4)]
    n_out = C.c_uint64(0); p = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint32))
    rcode = fn(len(v), *[p(x) for x in cols], chunk, 1 if per_gap else 0, *[p(x) for x in out], C.byref(n_out))
    assert rcode == 0, rcode
    return list(zip(*[x[:n_out.value].tolist() for x in out]))


def _wanted(L, name, per_gap):
    """restatement and host twin of a case, computed once"""
    if (name, per_gap) not in _want:
        v, names = CASES[name]
        w = rc.merge(v, names, per_gap)
        assert _tap(L.al_dbg_regions_merge_host, v, names, 0, per_gap) == w
        _want[(name, per_gap)] = w
    return _want[(name, per_gap)]


@pytest.mark.parametrize("chunk", [0, 64, 1000])
@pytest.mark.parametrize("name", list(CASES))
def test_the_device_merge_equals_the_restatement_and_the_host_twin(name, chunk):
    from airlift_amd import capi
    L = capi.load()
    v, names = CASES[name]
    for per_gap in (True, False):
        assert _tap(L.al_dbg_regions_merge, v, names, chunk, per_gap) == _wanted(L, name, per_gap), (name, chunk, per_gap)


def test_the_cases_reach_what_they_are_there_for():
    m = lambda n, pg=True: rc.merge(*CASES[n], per_gap=pg)
    assert m("n0") == [] and len(m("n1")) == 1 and len(m("two_identical")) == 1
    assert [x[2:] for x in m("book_ended")] == [(10, 30)] and len(m("gap_of_one")) == 2
    assert [x[2:] for x in m("long_nested")] == [(1000, 120000), (120001, 120010)] and len(CASES["long_nested"][0]) == 5003
    assert len(m("two_groups_same_coords")) == 2 and len(m("two_groups_same_coords", False)) == 1
    assert len(m("same_start_two_contigs")) == 3
    assert [x[1] for x in m("ranks_reverse")[:3]] == [0, 1, 2] and rc.ranks(rc.NAMES)[0] == [1, 2, 0]
    assert max(x[3] for x in m("top_coordinates")) == 2 ** 31 - 2
    assert len(m("boundaries")) == len(rc.SIZES) + 1
    for n in rc.SIZES:
        assert len(m("own_%d" % n)) == n and len(m("one_%d" % n)) == 1
