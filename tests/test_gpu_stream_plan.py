"""-m gpu: a mapping context with fewer physical streams than stream roles (al_stream_plan.h; AL_STREAMS sets the number, otherwise the
process's hardware queue count decides) prints the reference's bytes, whichever roles share a stream: aliased roles turn a fork / join into
stream order, and no wait may end up on work that is submitted after it."""
import json
import os
import re
import subprocess

import pytest

from test_gpu_sam import CLI, _diff_report

pytestmark = pytest.mark.gpu
SETS = ["g1_mt150pe", "g3_adversarial", "g6_repeats"]    # the smallest inputs that reach the re-chain pass, the equal-x heap merges and k_align
TIMEOUT = 120                                            # a case takes seconds; a run that does not end is a finding about the plan's waits


def _run(golden_unpacked, name, env, extra=(), unset=()):
    d = golden_unpacked[name]
    m = json.load(open(os.path.join(d, "meta.json")))
    cmd = [CLI, "-ax", "sr"] + list(extra) + (["-R", m["rg"]] if m.get("rg") else [])
    e = {k: v for k, v in os.environ.items() if k not in unset}
    e.update(env)
    r = subprocess.run(cmd + [m["ref"]] + m["reads"], cwd=d, capture_output=True, env=e, timeout=TIMEOUT)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r, open(os.path.join(d, "expected.sam"), "rb").read()


@pytest.mark.parametrize("n", ["1", "2", "3", "4", "6", "10"])
@pytest.mark.parametrize("name", SETS)
def test_every_stream_count_identical(golden_unpacked, name, n):
    r, exp = _run(golden_unpacked, name, dict(AL_STREAMS=n))
    assert r.stdout == exp, _diff_report(r.stdout, exp, "%s_streams%s" % (name, n))


@pytest.mark.parametrize("env,extra", [(dict(AL_SPEC_MIN="1"), []), (dict(AL_CHAIN_OVL="0"), []), (dict(AL_DP_CONC="0"), []), (dict(AL_REGS_SPLIT="0"), []),
                                       (dict(AL_TEST_TILE_ALL="1"), []), ({}, ["-K", "60000"]), (dict(AL_TEST_POISON="170", AL_TEST_GUARD="1"), [])],
                         ids=["every_candidate_merged_ahead_on_spec_streams", "lane_chaining_on_the_main_stream", "dp_classes_one_after_the_other", "chain_post_sort_and_pass_in_one_kernel",
                              "tile_kernel_all_fragments", "several_batches", "poisoned_memory_guard_zones"])
@pytest.mark.parametrize("name", SETS)
def test_four_streams_paths_identical(golden_unpacked, name, env, extra):
    """The arrangement switches and test switches at the default of a HIP process, four streams: AL_SPEC_MIN=1 puts real work on spec / spec2,
    -K 60000 reuses the events and the spec_busy drain across batches."""
    r, exp = _run(golden_unpacked, name, dict(env, AL_STREAMS="4"), extra)
    assert r.stdout == exp, _diff_report(r.stdout, exp, "%s_streams4_%s" % (name, "_".join(env) or "K"))
    assert b"GUARD" not in r.stderr, r.stderr.decode()[-1500:]


@pytest.mark.parametrize("name", SETS)
def test_two_streams_to_a_file_identical(golden_unpacked, name, tmp_path):
    """Output to a regular file: the stream driver, with two contexts of two streams each."""
    out = tmp_path / "out.sam"
    _, exp = _run(golden_unpacked, name, dict(AL_STREAMS="2"), ["-t", "8", "-o", str(out)])
    got = out.read_bytes()
    assert got == exp, _diff_report(got, exp, "%s_streams2_file" % name)


@pytest.mark.parametrize("queues,n,source", [("16", 10, "GPU_MAX_HW_QUEUES in the environment"), (None, 4, "default")])
def test_stream_count_follows_the_queue_count(golden_unpacked, queues, n, source):
    """Without AL_STREAMS the context has as many streams as the process has hardware queues: ten (a stream per role) at 16 queues, four
    when the variable is not in the environment -- HIP's own default."""
    env = dict(AL_TIMING="1"); unset = ["AL_STREAMS"]
    if queues is None:
        unset.append("GPU_MAX_HW_QUEUES")
    else:
        env["GPU_MAX_HW_QUEUES"] = queues
    r, exp = _run(golden_unpacked, "g1_mt150pe", env, unset=unset)
    assert r.stdout == exp, _diff_report(r.stdout, exp, "g1_mt150pe_queues_%s" % queues)
    m = re.search(r"\[airlift\] streams: (\d+) physical for (\d+) roles \(([^)]*)\)", r.stderr.decode(errors="replace"))
    assert m, r.stderr.decode(errors="replace")[-1500:]
    assert (int(m.group(1)), int(m.group(2)), m.group(3)) == (n, 10, source)
