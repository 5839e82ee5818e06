"""-m gpu: a switch of the environment table (airlift_amd/csrc/al_env.h) still reaches its site.  Equal SAM bytes alone cannot show that -- a switch
nobody reads leaves the output equal too -- so each case looks for the stderr line only the switch's site prints, and compares the SAM with the golden
where the results stay valid (here: everywhere).  The command line on g1_mt150pe, one process per case."""
import pytest

from test_gpu_sam import _diff_report
from test_gpu_stream_plan import _run

pytestmark = pytest.mark.gpu
NAME = "g1_mt150pe"


def _case(golden_unpacked, env, tag):
    r, exp = _run(golden_unpacked, NAME, env)
    assert r.stdout == exp, _diff_report(r.stdout, exp, "%s_env_%s" % (NAME, tag))
    return r.stderr.decode(errors="replace")


def test_timing_and_streams_reach_the_first_context(golden_unpacked):
    err = _case(golden_unpacked, dict(AL_TIMING="1", AL_STREAMS="3"), "timing1_streams3")
    assert "[airlift] streams: 3 physical for 10 roles (AL_STREAMS)" in err, err[-1500:]


def test_timing_zero_prints_no_stream_count(golden_unpacked):
    """AL_TIMING=0 is present, so the timing reports appear, but the stream count's line asks for a non-zero value."""
    err = _case(golden_unpacked, dict(AL_TIMING="0", AL_STREAMS="3"), "timing0")
    assert "[airlift] streams:" not in err, err[-1500:]


def test_trace_reaches_the_tile_kernel_site(golden_unpacked):
    err = _case(golden_unpacked, dict(AL_TRACE="1", AL_TEST_TILE_ALL="1"), "trace_tile_all")
    assert "[airlift] trace: tile kernel (" in err, err[-1500:]


def test_dbg_is_read_at_context_creation(golden_unpacked):
    """Bit 27 (no LDS chain kernels) keeps the results valid; the context still says what every non-zero AL_DBG says."""
    err = _case(golden_unpacked, dict(AL_DBG="134217728"), "dbg27")
    assert "[airlift] AL_DBG=134217728: timing experiment" in err, err[-1500:]


def test_dp_exit_stride_outside_the_set_falls_back(golden_unpacked):
    err = _case(golden_unpacked, dict(AL_DP_EXIT_STRIDE="3"), "stride3")
    assert "[airlift] AL_DP_EXIT_STRIDE=3 is not 1, 2, 4 or 8: using 8" in err, err[-1500:]
