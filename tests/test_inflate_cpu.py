"""The BGZF inflater's host twin (al_dev_inflate.h: the function k_inflate computes, evaluated serially) against Python's zlib over the case list."""
import pytest

import inflate_cases as ic
from inflate_util import inflate_host


def test_the_twin_inflates_every_valid_case():
    assert len(ic.valid_cases()) > 300
    for c in ic.valid_cases():
        rc, out, st = inflate_host(c.data)
        assert (rc, st) == (c.chain, c.codes), (c.name, rc, st)
        assert out == c.expect, c.name


def test_the_twin_rejects_exactly_the_invalid_cases():
    assert len(ic.invalid_cases()) >= 20
    for c in ic.invalid_cases():
        rc, out, st = inflate_host(c.data)
        assert (rc, st) == (c.chain, c.codes), (c.name, rc, st)
        assert rc != 0 or any(st), c.name


def test_the_verdict_on_a_deflate_stream_is_zlibs():
    """accept / reject of the raw stream by Python zlib, for every case that has one: the incomplete-code rules are zlib's, not our reading of them"""
    n = 0
    for c in ic.valid_cases() + ic.invalid_cases():
        if c.raw is None:
            continue
        n += 1
        rc, out, st = inflate_host(c.data)
        ours = rc == 0 and not any(st)
        theirs, payload = ic.zlib_verdict(c.raw)
        assert ours == theirs, c.name
        if theirs:
            assert out == payload, c.name
    assert n >= 25


def test_a_bad_member_leaves_its_neighbours_alone():
    by_name = {c.name: c for c in ic.valid_cases()}
    before, after = by_name["acgt_257_l9"], by_name["hand_dist_edges_overlapping"]
    assert len(before.expect) > 0 and len(after.expect) > 0
    n = 0
    for c in ic.invalid_cases():
        if not ic.is_member_level(c):
            continue
        n += 1
        rc, out, st = inflate_host(before.data + c.data + after.data)
        assert rc == 0 and st == before.codes + c.codes + after.codes, c.name
        assert out.startswith(before.expect) and out.endswith(after.expect), c.name
    assert n >= 15
