"""-m gpu: the extension DP's early exit evaluated every S-th anti-diagonal (AL_DP_EXIT_STRIDE = 1, 2, 4, 8; al_dev_ksw2.h).
Whatever S is, the SAM must be the one the full DP (AL_DP_EXIT=0) gives, the shadow mode must find no job whose outputs differ at the row the
strided test leaves at, and flanks whose exit row falls on every residue mod 8 must come out as ksw_extd2_sse computes them.
tests/test_dp_exit_stride_cpu.py checks the rule; this checks the kernels."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import dp_cases as D
import dp_tap as T
from test_dp_exit_stride_cpu import extd_stride, flank_jobs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "airlift_amd", "bin", "airlift-align")
SETS = ["g1_mt150pe", "g3_adversarial"]
STRIDES = ["1", "2", "4", "8"]
SHADOW = re.compile(rb"DP exit shadow \(two-cells-per-lane jobs\): jobs (\d+), differing (\d+); rows needed (\d+) of (\d+)")
_FULL = {}


def _run(d, env):
    m = json.load(open(os.path.join(d, "meta.json")))
    cmd = [CLI, "-ax", "sr"] + (["-R", m["rg"]] if m.get("rg") else [])
    e = {k: v for k, v in os.environ.items() if k not in ("AL_DP_EXIT", "AL_DP_EXIT_STRIDE", "AL_DBG2")}
    r = subprocess.run(cmd + [m["ref"]] + m["reads"], cwd=d, capture_output=True, env=dict(e, **env), timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r.stdout, r.stderr


def full_dp_sam(d, name):
    if name not in _FULL:
        _FULL[name] = _run(d, dict(AL_DP_EXIT="0"))[0]
        assert _FULL[name].count(b"\n") > 0
    return _FULL[name]


@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("name", SETS)
def test_sam_equals_full_dp(golden_unpacked, name, stride):
    d = golden_unpacked[name]
    assert _run(d, dict(AL_DP_EXIT_STRIDE=stride))[0] == full_dp_sam(d, name)


@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("name", SETS)
def test_shadow_mode_follows_the_stride(golden_unpacked, name, stride):
    d = golden_unpacked[name]
    out, err = _run(d, dict(AL_DP_EXIT_STRIDE=stride, AL_DBG2="32"))
    assert out == full_dp_sam(d, name)
    hits = SHADOW.findall(err)
    assert hits, err.decode()[-2000:]
    assert sum(int(h[0]) for h in hits) > 0
    assert sum(int(h[1]) for h in hits) == 0                              # "differing 0"
    assert sum(int(h[2]) for h in hits) <= sum(int(h[3]) for h in hits)   # rows needed <= rows


def _flanks(qlens=range(65, 81), seed=22, form=1):
    """Perfect flanks of 65 ... 80 bases against 2 qlen - 1 (the rule first holds at the even row 2 qlen - 2) and the same with one target base
    deleted (an odd row): the first exit row on every residue mod 8, checked on the CPU restatement before any device call."""
    jobs = []; first = set()
    for query, target in flank_jobs(qlens, seed):
        q, t = np.ascontiguousarray(query, dtype=np.uint8), np.ascontiguousarray(target, dtype=np.uint8)
        for f in D.FLAGS_PRODUCTION:
            jobs.append(D.Job(t, q, f, "flank"))
        rows = extd_stride(query, target, D.SR.a, D.SR.b, D.SR.q, D.SR.e, D.SR.q2, D.SR.e2, D.band(D.SR), D.SR.zdrop, D.SR.end_bonus, 1, form)[1]
        assert rows < len(q) + len(t) - 1
        first.add((rows - 1) & 7)
    assert first == set(range(8)), first
    assert sorted({len(j.query) for j in jobs[::4]}) == list(qlens) and all(len(j.target) == 2 * len(j.query) - 1 for j in jobs)
    return jobs


FLANKS = _flanks()
_WANT = []


@pytest.mark.parametrize("stride", STRIDES)
def test_flanks_with_the_exit_row_on_every_residue(stride, monkeypatch):
    if not _WANT:
        dp = D.ref_dp()
        _WANT.extend(dp(D.SR, j) for j in FLANKS)
    monkeypatch.setenv("AL_DP_EXIT_STRIDE", stride)                       # (read when the context is created)
    monkeypatch.delenv("AL_DP_EXIT", raising=False); monkeypatch.delenv("AL_DBG2", raising=False)
    cap = max(len(c) for _, c in _WANT) + 1
    got, cig, _ = T.ext_dp_tap(D.SR, FLANKS, 256, cap)
    assert {g["class"] for g in got} == {7}, {g["class"] for g in got}   # 9 and 10 target blocks: k_ext_dp<12>, where the exit is compiled in
    T.compare_ext_dp(D.SR, FLANKS, _WANT, got, cig, "stride " + stride)


def _flanks8():
    """The 8-block class (targets of 65 ... 128 bases; d_ksw_pk's EXIT == 2, which keeps zdropped exact): flanks of 49 ... 64 bases with the first
    exit row of that form on every residue mod 8, and clipped flanks -- all but the query's first quarter random -- whose full run z-drops, so that a group
    that left too early would show in zdropped."""
    jobs = _flanks(range(49, 65), 27, 2)
    rng = np.random.default_rng(28)
    for qlen in range(49, 65, 3):
        query = rng.integers(0, 4, qlen, dtype=np.uint8)
        target = np.concatenate([query, rng.integers(0, 4, qlen - 1, dtype=np.uint8)])
        query = np.concatenate([query[:qlen // 4], rng.integers(0, 4, qlen - qlen // 4, dtype=np.uint8)])
        for f in D.FLAGS_PRODUCTION:
            jobs.append(D.Job(np.ascontiguousarray(target), np.ascontiguousarray(query), f, "clipped"))
    return jobs


FLANKS8 = _flanks8()
_WANT8 = []


@pytest.mark.parametrize("stride", STRIDES)
def test_8_block_class_keeps_zdropped(stride, monkeypatch):
    if not _WANT8:
        dp = D.ref_dp()
        _WANT8.extend(dp(D.SR, j) for j in FLANKS8)
        zd = [rf["zdropped"] for rf, _ in _WANT8]
        assert 0 < sum(zd) < len(zd), zd                                  # both kinds on the reference, before any device call
    monkeypatch.setenv("AL_DP_EXIT_STRIDE", stride)
    monkeypatch.delenv("AL_DP_EXIT", raising=False); monkeypatch.delenv("AL_DBG2", raising=False)
    cap = max(len(c) for _, c in _WANT8) + 1
    got, cig, _ = T.ext_dp_tap(D.SR, FLANKS8, 256, cap)
    assert {g["class"] for g in got} == {6}, {g["class"] for g in got}   # 7 and 8 target blocks: k_ext_dp<8>, the EXIT == 2 form
    T.compare_ext_dp(D.SR, FLANKS8, _WANT8, got, cig, "8-block, stride " + stride, zdropped=True)
