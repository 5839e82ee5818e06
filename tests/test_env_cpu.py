"""The table of environment variables (airlift_amd/csrc/al_env.h) as a stand-alone host program under AddressSanitizer + UBSan: `make san-env` links
tests/csrc/env_main.cpp, which includes nothing but that header and prints every field.  The lists below are written by hand -- NAMES from a search for
getenv("...") in the sources before the table existed, RULES from the expression each site had -- so that the header is checked against them and not
against itself."""
import glob
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "airlift_amd", "csrc")

# every variable the library and the CLI read
NAMES = """
AL_ALLOC_GBS AL_AUTO_BATCH AL_BATCH_MS AL_BATCH_READS AL_BIG_MERGE AL_CAP22 AL_CAP4 AL_CAP8 AL_CHAIN_COOP AL_CHAIN_OVL AL_CHAIN_OVL2 AL_CHAIN_WAVE_MAX
AL_CTXS AL_DBG AL_DBG2 AL_DBG_FRAG AL_DP_CONC AL_DP_EXIT AL_DP_EXIT_STRIDE AL_DP_NO_SPLIT AL_DP_PK AL_DP_PK32 AL_FIN_HEAVY AL_GROW_DIV AL_HBM_MARGIN_MB
AL_HEAP_OLD AL_HOST_INDEX AL_HOST_IO AL_IDX_THREADS AL_INFLATE_PIECE_KB AL_LONG_BATCH AL_LONG_BATCH_BIG_FROM AL_NO_FAST_EXIT AL_NO_PWRITE AL_NO_RCCL
AL_NO_RESERVE AL_ORDER_BLOCK AL_OUT_PIECE_MB AL_PG_PLAIN AL_PIECE_MB AL_POOL_CHUNK_GB AL_PREP_HEAVY AL_PROBE_MULT AL_PROBE_READS AL_RANK_BATCH
AL_RANK_TIMEOUT AL_REGS_SPLIT AL_RESERVE_KB_PER_READ AL_RUN_ID AL_SERIAL_PARSE AL_SIDE_PRIO AL_SLOTS AL_SORT_MEM AL_SPEC_MERGE AL_SPEC_MIN AL_STREAMS
AL_STREAM_MAP AL_TEST_BIG_CHUNK AL_TEST_DEFLATE_NOMEM AL_TEST_GUARD AL_TEST_HEAP_WAVE AL_TEST_INFLATE_HOST AL_TEST_INFLATE_NOMEM AL_TEST_NOMEM_ABOVE
AL_TEST_POISON AL_TEST_POISON_LOG AL_TEST_POISON_ONLY AL_TEST_RUN AL_TEST_SCRUB AL_TEST_SEG_BIG AL_TEST_SORT_BIG AL_TEST_SORT_BLK AL_TEST_TILE_ALL
AL_TEST_TILE_FB AL_TIMING AL_TRACE AL_TRACE_ALLOC AL_TWO_PROBES
GPU_MAX_HW_QUEUES LOCAL_RANK MASTER_PORT RANK TMPDIR TORCHELASTIC_RUN_ID WORLD_SIZE
""".split()

# AL_* tokens of the tests that are no environment variables of the library
NOT_ENV_PREFIX = ("AL_F_",        # flag bits of al_mapopt_t
                  "AL_ERR_",      # error codes of the C-ABI
                  "AL_INF_E_")    # status codes of the BGZF inflater
NOT_ENV = {"AL_MM_VERSION",       # a constant of the CLI
           "AL_REF_CACHE"}        # read by tools/gen_synth.py and the tests, not by the library

VALUES = ["", "0", "1", "-1", "1000000", "x"]      # besides unset: empty, 0, 1, a negative value (the clamps), a large value, a non-number


def atoi(s):
    m = re.match(r"\s*([+-]?\d+)", s)
    return int(m.group(1)) if m else 0


def clamp(x, lo, hi):
    return x if lo is None and hi is None else max(lo, x) if hi is None else min(hi, max(lo, x))


# rule classes: what the field prints for the variable's value v (None = unset)
def present():
    return lambda v: str(int(v is not None))


def nonzero():
    return lambda v: str(int(v is not None and atoi(v) != 0))


def equals1():
    return lambda v: str(int(v is not None and atoi(v) == 1))


def off_if_zero():
    return lambda v: str(int(not (v is not None and atoi(v) == 0)))


def integer(default, lo=None, hi=None):
    return lambda v: str(default if v is None else clamp(atoi(v), lo, hi))


def unsigned(default, bits):       # a negative value wraps, as the cast at the site did
    return lambda v: str(default if v is None else atoi(v) % (1 << bits))


def positive_or(default):
    return lambda v: str(atoi(v) if v is not None and atoi(v) > 0 else default)


def real(default):
    return lambda v: float(default if v is None else atoi(v))       # (every value of VALUES reads the same as a double)


def optional(lo=None, hi=None):
    return lambda v: "unset" if v is None else str(clamp(atoi(v), lo, hi))


def optional_real():
    return lambda v: "unset" if v is None else float(atoi(v))


def text():
    return lambda v: "unset" if v is None else v


def nonempty_text(default="unset"):
    return lambda v: v if v else default


def stride_value(v):
    return str(atoi(v)) if v is not None and atoi(v) in (1, 2, 4, 8) else "8"


def stride_refused(v):
    return "unset" if v is None or atoi(v) in (1, 2, 4, 8) else v


def c_mod(a, n):       # C's remainder: the sign of the dividend
    return a % n if a >= 0 else -((-a) % n)


# variable -> {printed field: rule}, from the expression each site had before the table; a third element adds values to VALUES
RULES = {
    # present
    "AL_TRACE": {"trace": present()}, "AL_TRACE_ALLOC": {"trace_alloc": present()}, "AL_SERIAL_PARSE": {"serial_parse": present()},
    "AL_PG_PLAIN": {"pg_plain": present()}, "AL_NO_RCCL": {"no_rccl": present()}, "AL_NO_PWRITE": {"call.no_pwrite": present()},
    "AL_HOST_IO": {"host_io": present()}, "AL_HOST_INDEX": {"host_index": present()}, "AL_NO_RESERVE": {"no_reserve": present()},
    "AL_NO_FAST_EXIT": {"no_fast_exit": present()}, "AL_AUTO_BATCH": {"call.auto_batch": present()}, "AL_TWO_PROBES": {"two_probes": present()},
    "AL_TEST_POISON_LOG": {"test_poison_log": present()}, "AL_TEST_GUARD": {"test_guard": present()},
    "AL_TEST_DEFLATE_NOMEM": {"test_deflate_nomem": present()}, "AL_TEST_INFLATE_NOMEM": {"test_inflate_nomem": present()},
    "AL_TEST_TILE_ALL": {"test_tile_all": present()}, "AL_TEST_TILE_FB": {"test_tile_fb": present()}, "AL_DP_NO_SPLIT": {"dp_no_split": present()},
    # one variable under two rules: present everywhere, non-zero for the first context's "streams: ..." line
    "AL_TIMING": {"timing": present(), "timing_nonzero": nonzero()},
    # non-zero, equals 1, on unless 0
    "AL_TEST_INFLATE_HOST": {"test_inflate_host": nonzero()},
    "AL_SIDE_PRIO": {"side_prio": equals1()}, "AL_HEAP_OLD": {"heap_old": equals1()},
    "AL_CHAIN_OVL": {"chain_ovl": off_if_zero()}, "AL_CHAIN_OVL2": {"chain_ovl2": off_if_zero()}, "AL_SPEC_MERGE": {"spec_merge": off_if_zero()},
    "AL_DP_PK": {"dp_pk": off_if_zero()}, "AL_DP_PK32": {"dp_pk32": off_if_zero()},
    # integers: default, clamp
    "AL_HBM_MARGIN_MB": {"hbm_margin_mb": integer(2048, lo=0)}, "AL_PIECE_MB": {"piece_mb": integer(8, lo=1)}, "AL_OUT_PIECE_MB": {"out_piece_mb": integer(32, lo=1)},
    "AL_GROW_DIV": {"grow_div": integer(8, lo=1)}, "AL_INFLATE_PIECE_KB": {"inflate_piece_kb": positive_or(16384)},
    "AL_TEST_HEAP_WAVE": {"test_heap_wave": integer(-1)}, "AL_CHAIN_COOP": {"chain_coop": integer(-1)}, "AL_FIN_HEAVY": {"fin_heavy": integer(-1)},
    "AL_REGS_SPLIT": {"regs_split": integer(1)}, "AL_BIG_MERGE": {"big_merge": integer(1)}, "AL_ORDER_BLOCK": {"order_block": integer(128)},
    "AL_CAP4": {"cap4": integer(4096)}, "AL_CAP8": {"cap8": integer(4096)}, "AL_CAP22": {"cap22": integer(3072)},
    "AL_CHAIN_WAVE_MAX": {"chain_wave_max": unsigned(8192, 32)},
    "AL_RANK_BATCH": {"call.rank_batch": integer(0)}, "AL_DP_CONC": {"dp_conc": integer(700000)}, "AL_SORT_MEM": {"call.sort_mem": unsigned(16 << 30, 64)},
    # doubles
    "AL_POOL_CHUNK_GB": {"pool_chunk_gb": real(0.0)}, "AL_RANK_TIMEOUT": {"rank_timeout": real(600.0)}, "AL_LONG_BATCH": {"long_batch": real(0.0)},
    "AL_LONG_BATCH_BIG_FROM": {"long_batch_big_from": real(2.0e8)}, "AL_ALLOC_GBS": {"alloc_gbs": real(30.0)}, "AL_BATCH_MS": {"batch_ms": real(25.0)},
    # optional: unset differs from every value
    "AL_IDX_THREADS": {"idx_threads": optional()}, "AL_DBG_FRAG": {"dbg_frag": optional()}, "AL_SLOTS": {"slots": optional(lo=2, hi=8)},
    "AL_CTXS": {"ctxs": optional()}, "AL_BATCH_READS": {"batch_reads": optional(lo=2)}, "AL_PROBE_READS": {"probe_reads": optional(lo=2)},
    "AL_PROBE_MULT": {"probe_mult": optional(lo=1)}, "AL_TEST_SEG_BIG": {"test_seg_big": optional()}, "AL_PREP_HEAVY": {"prep_heavy": optional()},
    "AL_SPEC_MIN": {"spec_min": optional()}, "AL_RESERVE_KB_PER_READ": {"reserve_kb_per_read": optional_real()},
    # text, parsed further at its site
    "AL_STREAMS": {"streams": text()}, "AL_STREAM_MAP": {"stream_map": text()}, "AL_TEST_POISON": {"test_poison": text()},
    "AL_TEST_POISON_ONLY": {"test_poison_only": text()}, "AL_TEST_SORT_BLK": {"test_sort_blk": text()}, "AL_TEST_SORT_BIG": {"test_sort_big": text()},
    "AL_TEST_BIG_CHUNK": {"test_big_chunk": text()}, "AL_TEST_RUN": {"test_run": text()}, "AL_TEST_NOMEM_ABOVE": {"test_nomem_above": text()},
    "AL_TEST_SCRUB": {"test_scrub": text()}, "GPU_MAX_HW_QUEUES": {"gpu_max_hw_queues": text()},
    # context creation
    "AL_DBG": {"ctx.dbg": integer(0)}, "AL_DBG2": {"ctx.dbg2": integer(0)}, "AL_DP_EXIT": {"ctx.dp_exit": off_if_zero()},
    "AL_DP_EXIT_STRIDE": ({"ctx.dp_exit_stride": stride_value, "ctx.dp_exit_stride_refused": stride_refused}, ["2", "3", "4", "8", "16"]),
    # per call
    "RANK": {"call.rank": optional()}, "WORLD_SIZE": {"call.world_size": optional()},
    "LOCAL_RANK": ({"call.pick_device(-1,8)": lambda v: str(0 if v is None else c_mod(atoi(v), 8)),
                    "call.pick_device(-1,8,11)": lambda v: str(c_mod(11 if v is None else atoi(v), 8)),
                    "call.pick_device(-1,0,11)": lambda v: str(11 if v is None else atoi(v))}, ["3", "8", "13"]),
    "AL_RUN_ID": {"call.run_id": nonempty_text(), "call.run_id_vouched": present()},
    "TORCHELASTIC_RUN_ID": {"call.run_id": nonempty_text()}, "MASTER_PORT": {"call.run_id": nonempty_text()},
    "TMPDIR": {"call.tmpdir": nonempty_text("/tmp")},
}


def _rule(name):
    r = RULES[name]
    return r if isinstance(r, tuple) else (r, [])


@pytest.fixture(scope="module")
def program():
    r = subprocess.run(["make", "san-env"], cwd=CSRC, capture_output=True)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-3000:]
    return os.path.join(CSRC, "build", "san_env")


def run(program, **set_):
    env = {k: v for k, v in os.environ.items() if k not in NAMES}
    env.update(ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    env.update(set_)
    r = subprocess.run([program], capture_output=True, env=env, timeout=60)
    assert r.returncode == 0, (r.stdout + r.stderr).decode(errors="replace")[-3000:]
    return dict(l.split("=", 1) for l in r.stdout.decode().splitlines())


@pytest.fixture(scope="module")
def unset(program):
    return run(program)


def header_names():
    return set(re.findall(r'"([A-Z][A-Z0-9_]*)"', open(os.path.join(CSRC, "al_env.h")).read()))


def test_names_of_the_table_are_the_names_read_before():
    assert len(NAMES) == len(set(NAMES)) and sum(n.startswith("AL_") for n in NAMES) == 78
    assert header_names() == set(NAMES)


def test_no_getenv_outside_the_table():
    stray = [os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*")) if os.path.isfile(p) and os.path.basename(p) != "al_env.h" and "getenv(" in open(p, errors="replace").read()]
    assert stray == []


def test_every_name_is_in_the_design_document():
    doc = set(re.findall(r"\bAL_[A-Z0-9_]+", open(os.path.join(ROOT, "DESIGN.md")).read()))
    assert [n for n in NAMES if n.startswith("AL_") and n not in doc] == []


def test_every_switch_the_tests_name_exists():
    """A test that sets a variable the library does not read still matches its golden, and tests nothing."""
    files = glob.glob(os.path.join(ROOT, "tests", "*.py")) + glob.glob(os.path.join(ROOT, "tests", "helpers", "*")) + [os.path.join(ROOT, "bench.py"), os.path.join(ROOT, "__graft_entry__.py")]
    unknown = {}
    for p in files:
        if not os.path.isfile(p):
            continue
        for t in set(re.findall(r"\bAL_[A-Z0-9_]+", open(p, errors="replace").read())):
            if t not in NAMES and t not in NOT_ENV and not t.startswith(NOT_ENV_PREFIX):
                unknown.setdefault(t, []).append(os.path.relpath(p, ROOT))
    assert unknown == {}


def test_what_the_process_sets_itself_is_read_per_call():
    """The CLI and the self-tests set variables while the process runs (--sort-mem, no -K, the cases of a self-test): a value cached at the
    first look at the table would miss them.  The search sees setenv / unsetenv with a literal name only -- all csrc/ has; a putenv or a name
    put together at run time would escape it."""
    own = set()
    for p in glob.glob(os.path.join(CSRC, "*")):
        if os.path.isfile(p):
            own |= set(re.findall(r'\b(?:un)?setenv\("([A-Z0-9_]+)"', open(p, errors="replace").read()))
    assert own == {"AL_SORT_MEM", "AL_AUTO_BATCH", "AL_NO_PWRITE", "AL_RANK_BATCH"}
    assert [n for n in own if not all(f.startswith("call.") for f in _rule(n)[0])] == []


def test_every_name_has_a_rule_and_every_field_a_name(unset):
    assert sorted(RULES) == sorted(NAMES)
    fields = set()
    for n in NAMES:
        fields |= set(_rule(n)[0])
    assert fields | {"call.pick_device(5,8)"} == set(unset)


def test_defaults(unset):
    for n in NAMES:
        for f, rule in _rule(n)[0].items():
            want = rule(None)
            assert (float(unset[f]) if isinstance(want, float) else unset[f]) == want, (n, f)
    assert unset["call.pick_device(5,8)"] == "5"


@pytest.mark.parametrize("name", NAMES)
def test_rule_and_nothing_else_moves(program, unset, name):
    rules, more = _rule(name)
    for v in VALUES + more:
        got = run(program, **{name: v})
        for f, rule in rules.items():
            want = rule(v)
            assert (float(got[f]) if isinstance(want, float) else got[f]) == want, (name, v, f)
        assert {f: x for f, x in got.items() if f not in rules} == {f: x for f, x in unset.items() if f not in rules}, (name, v)


def test_run_id_order(program):
    """The first non-empty of AL_RUN_ID, TORCHELASTIC_RUN_ID and MASTER_PORT; an empty AL_RUN_ID still vouches for the id (the presence rule)."""
    assert run(program, AL_RUN_ID="a", TORCHELASTIC_RUN_ID="b", MASTER_PORT="29500")["call.run_id"] == "a"
    got = run(program, AL_RUN_ID="", TORCHELASTIC_RUN_ID="b", MASTER_PORT="29500")
    assert got["call.run_id"] == "b" and got["call.run_id_vouched"] == "1"
    assert run(program, TORCHELASTIC_RUN_ID="", MASTER_PORT="29500")["call.run_id"] == "29500"
