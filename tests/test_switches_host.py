"""The SML_* environment switches have one declaration each: struct Switches in sml_amd/csrc/capi.hip for the library,
sml_amd/switches.py for the Python package.  These tests hold the sources, INTEGRATION.md's table and the retired names to
that.  No GPU."""
import glob
import os
import re

import pytest

from conftest import REPO

CSRC = os.path.join(REPO, "sml_amd", "csrc")
# read by bench.py, tests/ or tools/ alone: neither declaration knows them, INTEGRATION.md's table lists them
ELSEWHERE = {"SML_A3_INPROC", "SML_A3_ORDER", "SML_BENCH_STRONG_LEG",                      # bench.py
             "SML_TEST_EIGHT_PROCESSES", "SML_TEST_JOB_TIMEOUT_S", "SML_GRAD_PIN_RATIOS",  # tests/
             "SML_FWD_F64_RATIOS", "SML_BARE_F64_RATIOS",
             "SML_HARNESS_EXTRA_PERIODS", "SML_PREFETCH", "SML_EVS_DBG"}                   # tools/
# (spelled without their prefix, so that this file passes its own last test)
RETIRED = ["SML_" + n for n in ("BWD_PRE", "PEER_POLL_IN_ADAM", "REPLAY_K0", "A3_KNOWN_LISTS", "PREP_NOWAVE", "PREP_COUNT", "EVENT_FLAGS")]
ENV_READ = re.compile(r"""environ(?:\.get\(|\[)\s*["'](SML_[A-Z0-9_]+)["']\]?(?!\s*=[^=])""")


def read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def csrc_files():
    return sorted(p for ext in ("hip", "h", "inc") for p in glob.glob(os.path.join(CSRC, "*." + ext)))


def switches_struct():
    """(text of capi.hip, span of struct Switches { ... };)"""
    src = read(os.path.join(CSRC, "capi.hip"))
    m = re.search(r"^struct Switches \{\n.*?^\};\n", src, re.S | re.M)
    assert m and "static Switches read()" in m.group(0)
    return src, m.span()


def library_switches():
    src, (a, b) = switches_struct()
    return set(re.findall(r'"(SML_[A-Z0-9_]+)"', src[a:b]))


def python_switches():
    from sml_amd import switches
    return set(switches.SWITCHES)


def test_the_library_names_its_switches_in_the_one_table_only():
    names = library_switches()
    assert len(names) == 16 and "SML_MF_DISTINCT" in names
    literals = set()
    for p in csrc_files():
        literals |= set(re.findall(r'"(SML_[A-Z0-9_]+)"', read(p)))
    assert literals == names, sorted(literals ^ names)
    # one field per switch, each with its meaning beside it
    src, (a, b) = switches_struct()
    fields = [l for l in src[a:b].splitlines() if "SML_" in l]
    assert len(fields) == len(names) and all(re.search(r";\s+// \S", l) for l in fields), fields


def test_the_library_reaches_the_environment_through_the_two_helpers_inside_the_table_only():
    src, (a, b) = switches_struct()
    for p in csrc_files():
        text = read(p)
        lines = [l for l in text.splitlines() if "getenv(" in l]
        if p.endswith("capi.hip"):
            assert len(lines) == 2 and lines[0].startswith("int env_int(const char* name, int dflt) {") and \
                lines[1].startswith("const char* env_str(const char* name, const char* dflt) {"), lines
            outside = text[:a] + text[b:]
            assert len(re.findall(r"\benv_int\(|\benv_str\(", outside)) == 2, "an env_int / env_str call outside struct Switches"
        else:
            assert not lines and not re.search(r"\benv_int\(|\benv_str\(", text), p


def test_entry_points_read_the_table_at_their_top_never_in_a_batch_loop():
    src, (_, end) = switches_struct()
    assert src.index('extern "C" {', end) > 0
    helpers, entries = src[end:src.index('extern "C" {', end)], src[src.index('extern "C" {', end):]
    assert "Switches::read()" not in helpers          # helpers take the value as an argument
    reads = list(re.finditer(r"Switches::read\(\)", entries))
    assert len(reads) >= 10
    for m in reads:
        before = entries[:m.start()]
        top = before[before.rindex("\nint sml_"):]           # from the entry point's signature to its read
        assert "for (" not in top and "Switches::read()" not in top, top[:200]


def py_files():
    return sorted(glob.glob(os.path.join(REPO, "sml_amd", "*.py")))


def test_the_python_package_reads_its_switches_through_the_accessor():
    from sml_amd import switches
    declared = python_switches()
    used = set()
    for p in py_files():
        text = read(p)
        assert '__import__("os")' not in text, p
        used |= set(re.findall(r'switches\.get\(\s*"(SML_[A-Z0-9_]+)"', text))
        if os.path.basename(p) == "switches.py":
            continue
        direct = {(os.path.basename(p), n) for n in ENV_READ.findall(text)}
        # (engine.peer_tensor saves and restores SML_PEER_MEM around its rewrite of it for sml_peer_alloc: the library's switch,
        # not a read of the Python package's -- it goes with that rewrite, which needs a C ABI change)
        assert direct <= {("engine.py", "SML_PEER_MEM")}, direct
    assert used == declared, sorted(used ^ declared)
    for name, (default, meaning) in switches.SWITCHES.items():
        assert (default is None or isinstance(default, str)) and meaning, name
    with pytest.raises(KeyError):
        switches.get("SML_NO_SUCH_SWITCH")


def test_the_accessor_reads_the_environment_at_the_call(monkeypatch):
    from sml_amd import switches
    monkeypatch.delenv("SML_COMM", raising=False)
    assert switches.get("SML_COMM") == "peer"
    monkeypatch.setenv("SML_COMM", "rccl")
    assert switches.get("SML_COMM") == "rccl"
    monkeypatch.delenv("SML_ONE_DEVICE", raising=False)
    assert switches.get("SML_ONE_DEVICE") is None


def test_class_attribute_switches_stay_assignable_class_attributes():
    from sml_amd.engine import HipEngine
    for attr, kind in (("EVAL_MODE", str), ("SIDE_EVAL_CUS", int), ("SIDE_EVAL_WORKGROUPS", int), ("TRANSFERRED_MAX_BYTES", int)):
        assert isinstance(HipEngine.__dict__[attr], kind), attr


def test_integration_md_lists_exactly_the_declared_switches():
    doc = read(os.path.join(REPO, "INTEGRATION.md"))
    section = doc[doc.index("## Environment switches"):]
    section = section[:section.index("\n## ", 3)] if "\n## " in section[3:] else section
    listed = set()
    for row in section.splitlines():
        if row.startswith("| `SML_"):
            listed |= set(re.findall(r"`(SML_[A-Z0-9_]+)`", row.split("|")[1]))
    want = library_switches() | python_switches() | ELSEWHERE
    assert listed == want, sorted(listed ^ want)
    # ... and ELSEWHERE really is everything bench.py, tests/ and tools/ read beyond the two declarations
    found = set()
    for p in [os.path.join(REPO, "bench.py")] + glob.glob(os.path.join(REPO, "tests", "*.py")) + glob.glob(os.path.join(REPO, "tools", "*.py")):
        found |= set(ENV_READ.findall(read(p)))
    assert found - library_switches() - python_switches() == ELSEWHERE, sorted((found - library_switches() - python_switches()) ^ ELSEWHERE)


def test_retired_switches_are_named_nowhere_but_in_design_md_retired_section():
    paths = [os.path.join(REPO, f) for f in ("bench.py", "INTEGRATION.md", "README.md")]
    for top in ("sml_amd", "tools", "tests", "include"):
        for root, dirs, files in os.walk(os.path.join(REPO, top)):
            dirs[:] = [d for d in dirs if d not in ("__pycache__", "_ref", "golden")]
            paths += [os.path.join(root, f) for f in files if f.endswith((".py", ".hip", ".h", ".inc", ".md", ".sh", ".cpp", ".txt"))]
    for p in paths:
        text = read(p)
        assert not [n for n in RETIRED if re.search(n + r"\b", text)], p
    design = read(os.path.join(REPO, "DESIGN.md"))
    start = design.index("## 7. Tried and rejected")
    assert not [n for n in RETIRED if re.search(n + r"\b", design[:start])]
    assert all(n in design[start:] for n in RETIRED)
