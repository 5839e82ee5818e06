"""The extension DP's kernels against the reference's ksw_extd2_sse, job by job, on the directed cases of tests/dp_cases.py.

Part one: the forms the al_dbg_ksw tap runs (d_ksw_extd2 on LDS rows, d_ksw_reg, and d_ksw_pk with AL_DBG bit 20), every output field."""
import ctypes as C
import os

import numpy as np
import pytest

import dp_cases as D

pytestmark = pytest.mark.gpu

_REF = {}


def reference(optname):
    """[(fields, cigar)] of ksw_extd2_sse for D.cases() under one option set (computed once per process)."""
    if optname not in _REF:
        dp = D.ref_dp(); o = D.OPTION_SETS[optname]
        _REF[optname] = [dp(o, j) for j in JOBS]
    return _REF[optname]


JOBS = D.cases()


def set_options(idx, o):
    m = idx.mo
    m.a, m.b, m.q, m.e, m.q2, m.e2, m.sc_ambi, m.zdrop, m.bw, m.end_bonus = o


@pytest.fixture(scope="module")
def small_index():
    import airlift_amd as A
    rng = np.random.default_rng(5)
    idx = A.Index(seqs=[bytes(b"ACGT"[i] for i in rng.integers(0, 4, 4000))], names=[b"chr"])
    yield idx
    idx.close()


TAP_FIELDS = ("score", "max", "max_q", "max_t", "mqe", "mqe_t", "zdropped", "reach_end")     # out9[0..7]; out9[8] = n_cigar


@pytest.mark.parametrize("form", ["one_cell_per_lane", "two_cells_per_lane"])
@pytest.mark.parametrize("optname", list(D.OPTION_SETS))
def test_tap_forms_equal_reference_in_every_field(small_index, optname, form, monkeypatch):
    """al_dbg_ksw on every case, plain (d_ksw_reg up to 22 target blocks, LDS rows above) and with AL_DBG bit 20 (d_ksw_pk up to 352 target
    bases where its precondition holds -- the sets outside it must fall back as the align stage does): all of out9 and the CIGAR."""
    import airlift_amd as A
    if form == "two_cells_per_lane":
        monkeypatch.setenv("AL_DBG", str(1 << 20))             # read when the context is created
    o = D.OPTION_SETS[optname]
    ref = reference(optname)
    jobs = JOBS + [D.oversize_job()]
    n = len(jobs)
    cap = max(len(c) for _, c in ref) + 1
    off = np.zeros(n + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(j.target) + len(j.query) for j in jobs])
    seqs = np.concatenate([x for j in jobs for x in (j.target, j.query)])
    tab = np.zeros((n, 6), dtype=np.int32)
    for i, j in enumerate(jobs):
        tab[i] = (off[i], off[i] + len(j.target), len(j.target), len(j.query), j.flag, 0)
    set_options(small_index, o)
    ctx = A.Context(small_index)
    set_options(small_index, D.SR)
    out = np.full((n, 9), -777, dtype=np.int32); cig = np.zeros((n, cap), dtype=np.uint32)
    rc = A.load().al_dbg_ksw(ctx.h, n, seqs.ctypes.data_as(C.c_void_p), seqs.nbytes, tab.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), cig.ctypes.data_as(C.c_void_p), cap)
    ctx.close()
    assert rc == 0
    assert out[n - 1, 8] == -1, "the 1025 x 10 job is above the tap's limit and must be refused, got n_cigar %d" % out[n - 1, 8]
    bad = []; compared = 0
    for i, (j, (rf, rcig)) in enumerate(zip(JOBS, ref)):
        compared += 1
        for k, name in enumerate(TAP_FIELDS):
            if int(out[i, k]) != rf[name]:
                bad.append("%s\n  [%s] %s: device %d, reference %d" % (D.describe(optname, j), form, name, out[i, k], rf[name]))
        ng = int(out[i, 8])
        assert 0 <= ng <= cap, "CIGAR of %d words does not fit the %d asked for: %s" % (ng, cap, D.describe(optname, j))
        if tuple(int(c) for c in cig[i, :ng]) != rcig:
            bad.append("%s\n  [%s] CIGAR: device %s, reference %s" % (D.describe(optname, j), form, D.cigar_str(cig[i, :ng]), D.cigar_str(rcig)))
        if len(bad) >= 4:
            break
    assert not bad, "\n".join(bad)
    assert compared == len(JOBS)


# ---- part two: the align stage's own kernels, by class ---------------------------------------------------------------------------------
# The cases go through al_dbg_ext_dp (the stage's class keying, job sort and launch table on caller-supplied jobs), each configuration in
# a fresh process (tests/helpers/dp_directed_child.py): the environment switches are read once per process.
import json
import subprocess
import sys

CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "dp_directed_child.py")
SLICES = ("lane16", "lane32", "g1", "g2", "g4", "g8", "g12", "g16", "g22", "g32", "lds")   # g12 / g16 / g22: class 7's jobs of 9-12, 13-16, 17-22 target blocks
SWITCHES = ("AL_DP_EXIT", "AL_DP_PK", "AL_DP_PK32", "AL_DBG", "AL_DBG2", "AL_DP_NO_SPLIT", "AL_DP_CONC")


def run_child(optname, lmax, mode, env):
    e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    e.update(env)
    r = subprocess.run([sys.executable, CHILD, optname, str(lmax), mode], capture_output=True, env=e, timeout=600)
    assert r.returncode == 0, "[%s, reads <= %d, %s list, %s]\n%s\n%s" % (optname, lmax, mode, env, r.stdout.decode()[-6000:], r.stderr.decode()[-3000:])
    res = json.loads(r.stdout.decode().strip().split("\n")[-1])
    assert res["compared"] == res["generated"] > 0                           # nothing skipped or filtered out after generation
    return res


def assert_covered(res, slices):
    for s in slices:
        c = res["cover"].get(s)
        assert c and c["left"] > 0 and c["right"] > 0 and c["rev0"] > 0 and c["rev1"] > 0, "no jobs of both directions and both strands for %s: %s" % (s, res["cover"])


CONFIGS = {                                                                  # name: (option set, longest read, list, environment, slices that must be reached)
    "default": ("sr", 256, "full", {}, SLICES),
    "exit_off": ("sr", 256, "full", {"AL_DP_EXIT": "0"}, SLICES),
    "one_cell_everywhere": ("sr", 256, "full", {"AL_DP_PK": "0"}, SLICES),
    "one_cell_32_blocks": ("sr", 256, "full", {"AL_DP_PK32": "0"}, SLICES),
    "no_lane_kernels": ("sr", 256, "full", {"AL_DBG": str(1 << 29)}, SLICES[2:]),       # the small jobs take g1 / g2
    "reads_to_504": ("sr", 504, "full", {}, SLICES),                         # the instances for queries above 256 bases
    "mixed_wavefronts": ("sr", 256, "sparse", {}, SLICES[5:]),               # one or two jobs per direction and block count: wavefronts of both directions
    "shadow": ("sr", 256, "full", {"AL_DBG2": "32"}, SLICES),
    "shadow_end_bonus0": ("end_bonus0", 256, "full", {"AL_DBG2": "32"}, SLICES),
    "shadow_end_bonus60": ("end_bonus60", 256, "full", {"AL_DBG2": "32"}, SLICES),
    "shadow_gaps": ("A2B4_O4_24_E2_1", 256, "full", {"AL_DBG2": "32"}, SLICES),   # (under O6_26_E2_1 the exit is off by its precondition a + b <= q + e: nothing to shadow)
    "O6_26_E2_1": ("O6_26_E2_1", 256, "full", {}, SLICES),
    "z25_r8": ("z25_r8", 256, "full", {}, SLICES),
    "B12": ("B12", 256, "full", {}, SLICES),
    "swap": ("swap", 256, "full", {}, SLICES),                             # the swapped gap models: outside the two-cells-per-lane form's precondition too
    "a16_gap64": ("a16_gap64", 256, "full", {}, SLICES),
    "ambi2": ("ambi2", 256, "full", {}, SLICES),                             # outside the two-cells-per-lane form's precondition: the one-cell kernels
    "a17": ("a17", 100, "full", {}, SLICES[:-2]),                            # (reads of 100 bases: with a = 17 longer ones leave the stage's tiles; no targets above 352 then)
}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_production_kernels_equal_reference_by_class(name):
    """max, max_q, max_t, reach_end, mqe_t when the end is reached, and the CIGAR of every job, zdropped too where the early exit cannot fire;
    every launch of the class table must have received jobs of both directions and both strands."""
    optname, lmax, mode, env, slices = CONFIGS[name]
    res = run_child(optname, lmax, mode, env)
    assert_covered(res, slices)
    assert res["zdropped_compared"] > 0
    names = ("lane16", "lane32", "lane64", "g1", "g2", "g4", "g8", "g22", "g32", "lds")
    by_class = dict(zip(names, res["dp_jobs"]))                              # the stage's own count of the jobs per class
    for s in slices:
        assert by_class["g22" if s in ("g12", "g16", "g22") else s] > 0, by_class
    assert sum(res["dp_jobs"]) == res["generated"], by_class
    if "AL_DBG" in env:
        assert by_class["lane16"] == 0 and by_class["lane32"] == 0
    if mode == "sparse":
        assert res["run_max"] <= 2                                           # no block count fills a wavefront with one direction
    else:
        assert res["run_min"] >= 8                                           # whole wavefronts of one direction
    if "AL_DBG2" in env:
        jobs, differing, rows, needed = res["shadow"][:4]
        assert jobs > 0 and differing == 0, res["shadow"]
        assert needed < rows, "the exit rule never held before the last row: rows needed %d of %d" % (needed, rows)
