"""The oracle's extension DP (o_ksw_extd2, oracle/al_oracle.c) against the reference's ksw_extd2_sse, call by call, on the directed cases of
tests/dp_cases.py: every output field and the CIGAR.  The whole-pipeline tests pin the oracle only where a difference moves a SAM line."""
import pytest

import dp_cases as D


@pytest.fixture(scope="module")
def dps():
    return D.ref_dp(), D.oracle_dp()


@pytest.fixture(scope="module")
def jobs():
    return D.cases()


def test_generator_holds_what_it_promises(jobs):
    tl = {len(j.target) for j in jobs}; ql = {len(j.query) for j in jobs}
    assert set(D.T_LENS) <= tl and set(D.Q_LENS) <= ql
    assert any(len(j.target) == 2 * len(j.query) - 1 and len(j.query) > 100 for j in jobs)
    assert {j.flag for j in jobs} == set(D.FLAGS) and {j.kind for j in jobs} == set(D.KIND_NAMES)
    assert all(len(j.target) <= D.TMAX and len(j.query) <= D.QMAX and j.target.max() <= 4 and j.query.max() <= 4 for j in jobs)
    again = D.cases()
    assert len(again) == len(jobs) and all((a.target == b.target).all() and (a.query == b.query).all() and a.flag == b.flag for a, b in zip(jobs, again))
    o = D.OPTION_SETS
    assert o["swap"].q + o["swap"].e > o["swap"].q2 + o["swap"].e2 and o["a16_gap64"].q + o["a16_gap64"].e == 63 and o["a16_gap64"].q2 + o["a16_gap64"].e2 == 64


@pytest.mark.parametrize("optname", list(D.OPTION_SETS))
def test_oracle_dp_equals_reference_dp(dps, jobs, optname):
    ref, orc = dps
    o = D.OPTION_SETS[optname]
    n = 0; bad = []
    for j in jobs:
        (rf, rc), (of, oc) = ref(o, j), orc(o, j)
        n += 1
        for k in D.FIELDS:
            if rf[k] != of[k]:
                bad.append("%s\n  %s: oracle %d, reference %d" % (D.describe(optname, j), k, of[k], rf[k]))
        if rc != oc:
            bad.append("%s\n  CIGAR: oracle %s, reference %s" % (D.describe(optname, j), D.cigar_str(oc), D.cigar_str(rc)))
        if len(bad) >= 5:
            break
    assert not bad, "\n".join(bad)
    assert n == len(jobs)
