"""-m gpu tests of the chain file's region logic on the device alone: al_dbg_chainreg (the segmented sum, k_chn_expand / k_chn_expand_m, the merge sort, the
max-scan, the head sum, k_chn_compact, k_chn_invert, k_chn_tail, k_chn_gather) on every case of chainreg_cases.py against the host twin -- rows and counts
of all three outputs, with and without merged regions.  The twin itself is held against the plain restatement by test_chain_beds_cpu.py."""
import pytest

import chainreg_cases as cc

pytestmark = pytest.mark.gpu
CASES = cc.cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_the_device_equals_the_host_twin(case):
    from airlift_amd import capi
    L = capi.load()
    name, t, R, E, M = case
    want = cc.tap(L.al_dbg_chainreg_host, t, R, E, M)
    got = cc.tap(L.al_dbg_chainreg, t, R, E, M)
    for kind, g, w in zip(("gaps", "constant", "retired"), got, want):
        assert len(g) == len(w) and g == w, (name, kind)
    assert cc.tap(L.al_dbg_chainreg, t, R, E, None) == (want[0], want[1], None)
    if M:                                                                 # the blocks alone: M = []
        assert cc.tap(L.al_dbg_chainreg, t, R, E, []) == cc.tap(L.al_dbg_chainreg_host, t, R, E, [])


def test_the_device_gives_the_golden_rows():
    from airlift_amd import capi
    L = capi.load()
    for name, chain, merged, R, E, want in cc.golden():
        t = cc.parse(chain); M = cc.parse_merged(merged)
        g, c, r = cc.tap(L.al_dbg_chainreg, t, R, E, M)
        assert cc.bed(g, t.names) == want["gaps"] and cc.bed(c, t.names) == want["constant"] and cc.bed(r, cc.retired_slots(t, M)) == want["retired"], name
