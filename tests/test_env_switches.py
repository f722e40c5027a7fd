"""The library's environment switches are written once, in csrc/env_switches.h: nothing else under csrc/ calls getenv, the table's
names are unique and documented, and every CIS_* variable a test or tool sets is a name somebody reads (a typo would otherwise pass
silently and prove nothing).  Needs neither the library nor a device."""
import ast
import glob
import os
import re
import shutil
import subprocess

from conftest import REPO

CSRC = os.path.join(REPO, "columbiaimagesearch_amd", "csrc")
ROW = re.compile(r'^\s*X\((\w+),\s*"(CIS_[A-Z0-9_]+)",\s*(\w+),\s*([^,]+),\s*(LATCHED|PER_CALL),\s*"([^"]+)"\)', re.M)
KINDS = {"PRESENT", "NONZERO", "INT", "INT_POS", "REAL", "STR"}


def table():
    rows = ROW.findall(open(os.path.join(CSRC, "env_switches.h")).read())
    assert len(rows) >= 70, "the X(...) lines of env_switches.h no longer match this test's pattern"
    return rows


def python_read_names():
    """CIS_* variables that Python code reads: the package, bench.py, the tests and their helper scripts."""
    files = glob.glob(os.path.join(REPO, "columbiaimagesearch_amd", "**", "*.py"), recursive=True) + [os.path.join(REPO, "bench.py")]
    files += glob.glob(os.path.join(REPO, "tests", "*.py")) + glob.glob(os.path.join(REPO, "tests", "tools", "*.py"))
    names = set()
    for path in files:
        if os.path.basename(path) == "test_env_switches.py":
            continue
        src = open(path).read()
        names |= set(re.findall(r'environ\.get\(\s*"(CIS_[A-Z0-9_]+)"', src))
        names |= set(re.findall(r'environ\[\s*"(CIS_[A-Z0-9_]+)"\s*\](?!\s*=[^=])', src))  # a read, not an assignment
    return names


def c_constants():
    """the error, dtype and precision constants of include/cis_hip.h: CIS_* names that are no environment variables"""
    return set(re.findall(r"\bCIS_[A-Z0-9_]+", open(os.path.join(REPO, "include", "cis_hip.h")).read()))


def names_set_in(src):
    """Every CIS_* name a file can hand to an environment, wherever it sits (setenv / delenv / os.environ[...] directly, or through a
    route table or a multi-line env= dict): the string constants that are exactly a CIS_* name and the keyword arguments CIS_X=.
    Attribute accesses (`_lib.CIS_EINVAL`) are neither; a constant of the C header spelled as a string is taken out by name."""
    names = set()
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, ast.Constant) and isinstance(node.value, str) and re.fullmatch(r"CIS_[A-Z0-9_]+", node.value):
            names.add(node.value)
        elif isinstance(node, ast.keyword) and node.arg and re.fullmatch(r"CIS_[A-Z0-9_]+", node.arg):
            names.add(node.arg)
    return names - c_constants()


def test_only_the_header_calls_getenv():
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h"))):
        if os.path.basename(path) != "env_switches.h":
            assert "getenv(" not in open(path).read(), path
    assert open(os.path.join(CSRC, "env_switches.h")).read().count("getenv(") == 1


def test_table_is_well_formed():
    rows = table()
    for col in (0, 1):
        vals = [r[col] for r in rows]
        assert len(set(vals)) == len(vals), sorted(v for v in vals if vals.count(v) > 1)
    for ident, name, kind, dflt, when, text in rows:
        assert kind in KINDS, name
        assert name == "CIS_" + ident.upper(), name
        if kind in ("PRESENT", "NONZERO", "STR"):
            assert dflt.strip() == "0", name
        if when == "LATCHED":
            assert dflt.strip() != "SITE", name
    # every line of the list is a row this test saw: a row the pattern misses would escape the checks
    body = open(os.path.join(CSRC, "env_switches.h")).read()
    assert len(re.findall(r"^\s*X\(", body, flags=re.M)) == len(rows)


def test_every_switch_is_documented():
    doc = open(os.path.join(REPO, "INTEGRATION.md")).read()
    section = doc.split("## Environment switches of `libcis_hip.so`")[1].split("\n## ")[0]
    documented = set(re.findall(r"CIS_[A-Z0-9_]+", section))
    for prefix, tail in re.findall(r"`(CIS_[A-Z0-9]+)_[A-Z0-9]+`((?:\s*/\s*`_[A-Z0-9_]+`)+)", section):  # `CIS_STREAM_SEG` / `_SS` / `_K`
        documented |= {prefix + t for t in re.findall(r"_[A-Z0-9_]+", tail)}
    missing = sorted(name for _, name, *_ in table() if name not in documented)
    assert not missing, missing
    # ... and its row's last column says when it is read: "per call", "once per process", or "once per process: `A`, `B`; per call: the rest"
    latched = {name for _, name, _, _, when, _ in table() if when == "LATCHED"}
    said = set()
    for line in section.split("\n"):
        cells = line.split(" | ")
        if len(cells) == 3 and cells[0].startswith("| `CIS_"):
            read = cells[2].rstrip(" |")
            assert re.fullmatch(r"per call|once per process(: (`CIS_[A-Z0-9_]+`(, )?)+; per call: the rest)?", read), line[:60]
            if read.startswith("once"):
                said |= set(re.findall(r"CIS_[A-Z0-9_]+", read if ":" in read else cells[0]))
    assert said == latched, sorted(said ^ latched)


def test_tests_and_tools_set_only_names_somebody_reads():
    known = {name for _, name, *_ in table()} | python_read_names()
    assert {"CIS_LIB_PATH", "CIS_POOL_NO_PIN", "CIS_FIXED_STRIDE", "CIS_CHECK_BACKEND", "CIS_BENCH_N"} <= known
    files = glob.glob(os.path.join(REPO, "tests", "*.py")) + glob.glob(os.path.join(REPO, "tests", "tools", "*.py"))
    files += glob.glob(os.path.join(REPO, "tools", "*.py"))
    seen = set()
    for path in sorted(files):
        if os.path.basename(path) == "test_env_switches.py":
            continue
        used = names_set_in(open(path).read())
        assert used <= known, (os.path.relpath(path, REPO), sorted(used - known))
        seen |= used
    # the walk still finds what the tests set: on setenv lines, in the CNN route tables, on the second line of an env= dict
    assert {"CIS_SEG_MAX", "CIS_STREAM_SS", "CIS_CNN_NO_TAIL", "CIS_S4_ZL", "CIS_BENCH_MIN_REPS"} <= seen
    # a misspelled switch is caught on a setenv line, in a multi-line env= dict and in a route table; the C constants are not switches
    typos = '''
monkeypatch.setenv("CIS_SEG_MAXX", "1")
env = dict(os.environ, CIS_BENCH_N="1000",
           CIS_NO_TNY="1")
ROUTES = [("tail", {"CIS_CNN_NO_TAILL": "1"}), ("graph", {"CIS_CNN_GRAPH": "1"})]
for knob in ("CIS_S4_ZL", "CIS_S4_FRACC"):
    monkeypatch.delenv(knob, raising=False)
assert rc == _lib.CIS_EINVAL and x.dtype == getattr(_lib, "CIS_F32")
'''
    assert names_set_in(typos) - known == {"CIS_SEG_MAXX", "CIS_NO_TNY", "CIS_CNN_NO_TAILL", "CIS_S4_FRACC"}


def test_accessors_parse_as_the_hand_written_lines_did(tmp_path):
    """tests/tools/env_switches_semantics.cpp: old expression against accessor for every kind, on odd values; the latch of once<id>()"""
    cxx = next((c for c in (shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"), "/opt/rocm/lib/llvm/bin/clang++") if c and os.path.exists(c)), None)
    assert cxx, "no host C++ compiler (the build itself needs hipcc's clang++)"
    exe = str(tmp_path / "env_switches_semantics")
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-I", CSRC, os.path.join(REPO, "tests", "tools", "env_switches_semantics.cpp"), "-o", exe])
    env = {k: val for k, val in os.environ.items() if not k.startswith("CIS_")}
    out = subprocess.run([exe], env=env, capture_output=True, text=True)
    assert out.returncode == 0 and "\n0 mismatches" in "\n" + out.stdout, out.stdout[-2000:]
