"""The library's environment switches (csrc/tunables.hpp: one list, one parser).  tests/cpp/host_tunables.cpp, built with plain g++,
prints the list and every entry's value under the environment it is started with; the expectations below are written out here --
what each switch meant before there was a list, with the unifications DESIGN.md section 8 names -- and are not derived from the
header.  Then the places the list has to agree with: getenv in csrc/ occurs in that header only, the retired names occur nowhere,
every ZKHIP_* variable a test or a tool sets is an entry (or one of the four that Python code reads), every entry has its row in
DESIGN.md."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zk-cryptography_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "host_tunables.cpp")

U = "unset"
INT_MAX = 2147483647
BUDGET = 2 << 30
ON = dict(kind="flag", default=1, lo=0, hi=1, outside="ignored", when="once")
OFF = dict(ON, default=0)
# the flags: on when the leading integer is non-zero -- "" and "abc" have none, which reads as 0
FLAG_ROW = {"": 0, "0": 0, "1": 1, "abc": 0, "7": 1, "-1": 1, "2": 1, "01": 1, "10": 1}


def _int(default, lo, hi, outside, when="once"):
    return dict(kind="int", default=default, lo=lo, hi=hi, outside=outside, when=when)


# name -> (the entry, {value of the variable: what the library reads}); every row holds "", "0", "1", "abc", "-1", one value in
# the range, the one below the range and the one above it
SWITCHES = {
    "PIPE": (ON, FLAG_ROW),
    "PIPE_WGS": (_int(256, 1, 512, "ignored"), {"": 256, "0": 256, "1": 1, "abc": 256, "64": 64, "512": 512, "513": 256, "-1": 256}),
    "ROUND_DOT": (ON, FLAG_ROW),
    "ROUND_DOT_MIN_LOG": (_int(U, 8, 64, "clamped"), {"": 8, "0": 8, "1": 8, "abc": 8, "12": 12, "7": 8, "65": 64, "-1": 8}),
    "ROUND_GRID": (_int(0, 1, INT_MAX, "ignored"), {"": 0, "0": 0, "1": 1, "abc": 0, "96": 96, "2147483648": 0, "-1": 0}),
    "STAGE": (_int(-1, 0, 1, "ignored"), {"": 0, "0": 0, "1": 1, "abc": 0, "2": -1, "-1": -1}),
    "STAGE_MIN_LOG_ONE": (_int(18, 12, 30, "ignored"), {"": 18, "0": 18, "1": 18, "abc": 18, "15": 15, "11": 18, "31": 18, "-1": 18}),
    "STAGE_MIN_LOG_MANY": (_int(18, 12, 30, "ignored"), {"": 18, "0": 18, "1": 18, "abc": 18, "30": 30, "11": 18, "31": 18, "-1": 18}),
    "CROSS_VALU": (OFF, FLAG_ROW),
    "CROSS_GRID": (_int(0, 1, INT_MAX, "ignored"), {"": 0, "0": 0, "1": 1, "abc": 0, "64": 64, "2147483648": 0, "-1": 0}),
    "MF": (_int(1, 0, 9, "ignored"), {"": 0, "0": 0, "1": 1, "abc": 0, "5": 5, "9": 9, "10": 1, "13": 1, "-1": 1}),
    "MF_OCC": (_int(0, 1, 64, "ignored"), {"": 0, "0": 0, "1": 1, "abc": 0, "2": 2, "64": 64, "65": 0, "200": 0, "-1": 0}),
    "FINE_LDS": (_int(79872, 0, 158 * 1024, "clamped"),
                 {"": 0, "0": 0, "1": 1, "abc": 0, "40960": 40960, "161793": 158 * 1024, "-1": 0}),
    "OVERLAP_MIN_LOG": (_int(24, 19, 25, "ignored"), {"": 24, "0": 24, "1": 24, "abc": 24, "19": 19, "18": 24, "26": 24, "-1": 24}),
    "MSM_SMALL": (ON, FLAG_ROW),
    "MSM_BATCH_DELTA": (_int(1, 0, 8, "ignored"), {"": 0, "0": 0, "1": 1, "abc": 0, "2": 2, "8": 8, "9": 1, "-1": 1}),
    "LEVEL_TABLE_DELTA": (_int(U, -3, 4, "ignored"), {"": 0, "0": 0, "1": 1, "abc": 0, "-2": -2, "-4": U, "5": U, "-1": -1}),
    "OPEN_PIPELINES": (OFF, FLAG_ROW),
    "GKR_FUSE_SMALL": (ON, FLAG_ROW),
    "GKR_HOST_TRANSCRIPT": (OFF, FLAG_ROW),
    # the whole string a decimal number as strtoull reads one (a sign included: "-1" wraps to the largest value), else the default
    "PLONK_CACHE_BUDGET": (dict(kind="bytes", default=BUDGET, lo=0, hi=2 ** 63 - 1, outside="ignored", when="fresh"),
                           {"": BUDGET, "0": 0, "1": 1, "abc": BUDGET, "4096": 4096, "4096k": BUDGET, "12 ": BUDGET, "-1": 2 ** 64 - 1}),
    "RCCL_LIB": (dict(kind="text", default=0, lo=0, hi=0, outside="ignored", when="once"),
                 {"": "text:", "0": "text:0", "1": "text:1", "abc": "text:abc", "/x/librccl.so.1": "text:/x/librccl.so.1", "-1": "text:-1"}),
}
REMOVED = ["EVAL_ONE_PASS", "FOLD_LDS", "GKR_GRAPH", "GKR_LANE_PRIO", "MSM_C", "OPEN_BATCH_LOG", "OPEN_SLOTS", "PIPE_MAX_Q", "PIPE_MID",
           "PIPE_TAIL", "ROUND_TSPLIT"]
PYTHON_READS = {"ZKHIP_LIB", "ZKHIP_DIAG_LIB", "ZKHIP_BENCH_ONE_GPU", "ZKHIP_SELFTEST_FAILURE_INJECTION"}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("tunables") / "host_tunables")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", path, SRC])
    return path


def _run(exe, env):
    base = {k: v for k, v in os.environ.items() if not k.startswith("ZKHIP_")}
    out = subprocess.run([exe], env=dict(base, **env), stdout=subprocess.PIPE, check=True, timeout=60).stdout.decode()
    entries, values = {}, {}
    for line in out.splitlines():
        head, _, meaning = line.partition(" | ")
        f = head.split(" ", 2)
        if f[0] == "entry":
            entries[f[1]] = (f[2], meaning)
        else:
            assert f[0] == "value", line
            values[f[1]] = f[2] if len(f) > 2 else ""
    return entries, values


def test_the_list_is_the_documented_one(exe):
    entries, values = _run(exe, {})
    assert list(entries) == ["ZKHIP_" + n for n in SWITCHES] and len(entries) == 22
    for name, (e, _) in SWITCHES.items():
        text, meaning = entries["ZKHIP_" + name]
        assert text == "%s def=%s lo=%d hi=%d %s %s" % (e["kind"], e["default"], e["lo"], e["hi"], e["outside"], e["when"]), name
        assert meaning.strip() and "\n" not in meaning
        # nothing set: the default
        assert values["ZKHIP_" + name] == (U if e["kind"] == "text" else str(e["default"])), name


def test_every_switch_under_every_value(exe):
    # one run per column of the matrix: the k-th value of every switch's row at once
    for k in range(max(len(row) for _, row in SWITCHES.values())):
        env, want = {}, {}
        for name, (_, row) in SWITCHES.items():
            if k < len(row):
                value = list(row)[k]
                env["ZKHIP_" + name] = value
                want["ZKHIP_" + name] = str(row[value])
        _, values = _run(exe, env)
        for name in want:
            assert values[name] == want[name], (name, env[name], values[name], want[name])
    for name, (_, row) in SWITCHES.items():
        assert {"", "0", "1", "abc", "-1"} <= set(row), name


def test_a_switch_reads_its_own_variable_only(exe):
    _, base = _run(exe, {})
    for name in SWITCHES:
        _, values = _run(exe, {"ZKHIP_" + name: "1"})
        for other in SWITCHES:
            if other != name:
                assert values["ZKHIP_" + other] == base["ZKHIP_" + other], (name, other)


def _files(*tops, ext=None):
    for top in tops:
        top = os.path.join(ROOT, top)
        if os.path.isfile(top):
            yield top
        for d, dirs, names in os.walk(top):
            dirs[:] = [x for x in dirs if x not in ("build", "__pycache__")]
            for n in names:
                if ext is None or n.endswith(ext):
                    yield os.path.join(d, n)


def _text(path):
    with open(path, errors="replace") as f:
        return f.read()


def test_getenv_occurs_in_the_header_only():
    hits = [os.path.relpath(p, CSRC) for p in _files("zk-cryptography_amd/csrc", ext=(".hip", ".hpp", ".h", ".cpp")) if "getenv" in _text(p)]
    assert hits == ["tunables.hpp"]


def test_no_retired_name_is_left():
    pat = re.compile(r"ZKHIP_(%s)\b" % "|".join(REMOVED))
    me = os.path.abspath(__file__)
    for p in _files("zk-cryptography_amd/csrc", "tests", "tools", "bench.py", "README.md", "DESIGN.md", "INTEGRATION.md",
                    ext=(".hip", ".hpp", ".h", ".cpp", ".py", ".sh", ".md", ".c")):
        if os.path.abspath(p) != me:
            assert not pat.search(_text(p)), p


def test_what_tests_and_tools_set_is_on_the_list():
    known = {"ZKHIP_" + n for n in SWITCHES} | PYTHON_READS
    pat = re.compile(r"\bZKHIP_[A-Z0-9_]+\b")
    abi = re.compile(r"ZKHIP_(OK|ERR_[A-Z]+)$")          # the C ABI's status codes are no variables
    me = os.path.abspath(__file__)
    for p in _files("tests", "tools", "bench.py", ext=(".py", ".sh")):
        if os.path.abspath(p) == me:
            continue
        for name in set(pat.findall(_text(p))):
            assert name in known or abi.match(name), (p, name)


def test_every_entry_has_its_row_in_the_design_document():
    doc = _text(os.path.join(ROOT, "DESIGN.md"))
    start = doc.index("Environment switches")
    section = doc[start:]
    nxt = re.search(r"(?m)^#{1,6} ", section[1:])
    section = section[:nxt.start() + 1] if nxt else section
    rows = re.findall(r"(?m)^\| `(ZKHIP_[A-Z0-9_]+)` \|", section)
    assert rows == ["ZKHIP_" + n for n in SWITCHES]
