"""The ROMAN_* environment switches without a GPU: roman_amd/csrc/switches.h is the one place that reads them; tests/switches_main.cpp,
built here with the host compiler and -fsanitize=address,undefined (runtimes linked into the program), sets the environment with
setenv / unsetenv and prints the parsed struct.  Every expected value below restates the expression that read the variable in
roman_hip.hip BEFORE the header existed (quoted beside it) — the table pins those rules, oddities included."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "roman_amd", "csrc")

# every name roman_hip.hip passed to getenv before switches.h
NAMES = ["ROMAN_DEBUG", "ROMAN_TEST_CAPNNZ", "ROMAN_TEST_CAPLIST", "ROMAN_COS_SEL", "ROMAN_SORT_EQMAX", "ROMAN_COS_DEAL", "ROMAN_COS_BLOCK",
         "ROMAN_WIDE", "ROMAN_WIDE_IDX16", "ROMAN_COUNT_PRE", "ROMAN_SMALL_FUSED", "ROMAN_SMALL_ONLY", "ROMAN_COUNT_WHOLE", "ROMAN_COUNT_ZLDS",
         "ROMAN_LISTS", "ROMAN_LISTS_LDS", "ROMAN_SMALL", "ROMAN_WIDE_TEAMS", "ROMAN_WIDE_UPPER", "ROMAN_WIDE_COMPACT", "ROMAN_NUM_XCC",
         "ROMAN_WIDE_SPIN_MS"]
ONCE = ["ROMAN_DEBUG", "ROMAN_WIDE", "ROMAN_SMALL_FUSED", "ROMAN_SMALL_ONLY", "ROMAN_SMALL"]       # were `static const` reads

LIB = -1            # "the library decides"
FLAG_VALUES = (None, "", "0", "1", "x")             # None: unset
INT_VALUES = (None, "", "0", "1", "7", "-3", "x")

# switch -> (values, {field: expected per value})
TABLE = {
    # static const bool dbg = getenv("ROMAN_DEBUG") != nullptr;
    "ROMAN_DEBUG": (FLAG_VALUES, {"debug": (0, 1, 1, 1, 1)}),
    # wideEnv ? wideEnv[0] == '1' : (the library's rule)          — no empty check: "" is "never"
    "ROMAN_WIDE": (FLAG_VALUES, {"wide": (LIB, 0, 0, 1, 0)}),
    # !(fusedEnv && fusedEnv[0] == '0')   /   !(onlyEnv && onlyEnv[0] == '0')   /   !(smallEnv && smallEnv[0] == '0')
    "ROMAN_SMALL_FUSED": (FLAG_VALUES, {"small_fused": (1, 1, 0, 1, 1)}),
    "ROMAN_SMALL_ONLY": (FLAG_VALUES, {"small_only": (1, 1, 0, 1, 1)}),
    "ROMAN_SMALL": (FLAG_VALUES, {"small": (1, 1, 0, 1, 1)}),
    # cos_sel_applies: if (env && env[0]) return env[0] == '1';
    # roman_debug_cosine: selEnv && (!strcmp(selEnv, "approx") || !strcmp(selEnv, "gated")), then approx = selEnv[0] == 'a'
    "ROMAN_COS_SEL": (FLAG_VALUES + ("approx", "gated", "approximate", "a"),
                      {"cos_sel": (LIB, LIB, 0, 1, 0, 0, 0, 0, 0), "cos_sel_matrix": (0, 0, 0, 0, 0, 2, 1, 0, 0)}),
    # (dealEnv && dealEnv[0]) ? dealEnv[0] == '1' : (the library's rule)
    "ROMAN_COS_DEAL": (FLAG_VALUES, {"cos_deal": (LIB, LIB, 0, 1, 0)}),
    # maps of at most 48 objects: (blockEnv && blockEnv[0]) ? blockEnv[0] == '1' : B <= 2 * num_cu
    # larger maps:                !(blockEnv && blockEnv[0] == '0') && (few blocks)
    "ROMAN_COS_BLOCK": ((None, "", "0", "1", "2"), {"cos_block": (LIB, LIB, 0, 1, 0), "cos_block_large": (1, 1, 0, 1, 1)}),
    # (preEnv ? preEnv[0] != '0' : true) && ... && Lneed <= (preEnv ? 16000 : 4096): the limit rises whenever the field is not LIB
    "ROMAN_COUNT_PRE": (FLAG_VALUES, {"count_pre": (LIB, 1, 0, 1, 1)}),
    # wholeEnv ? wholeEnv[0] != '0' : B >= num_cu
    "ROMAN_COUNT_WHOLE": (FLAG_VALUES, {"count_whole": (LIB, 1, 0, 1, 1)}),
    # listsEnv ? (listsEnv[0] == '0' ? 0 : 1) : (the library's rule)
    "ROMAN_LISTS": (FLAG_VALUES, {"lists": (LIB, 1, 0, 1, 1)}),
    # if (e_ && e_[0]) a_ucfg = (D.idx16 && e_[0] != '0') ? 1 : 0;
    "ROMAN_WIDE_UPPER": (FLAG_VALUES, {"wide_upper": (LIB, LIB, 0, 1, 1)}),
    # !(i16Env && i16Env[0] == '0')   /   !(zEnv && zEnv[0] == '0')
    "ROMAN_WIDE_IDX16": (FLAG_VALUES, {"wide_idx16": (1, 1, 0, 1, 1)}),
    "ROMAN_COUNT_ZLDS": (FLAG_VALUES, {"count_zlds": (1, 1, 0, 1, 1)}),
    # (e && e[0]) ? std::max(0, atoi(e)) : 512
    "ROMAN_SORT_EQMAX": (INT_VALUES, {"sort_eq_max": (512, 512, 0, 1, 7, 0, 0)}),
    # std::min(room, llEnv ? (size_t)std::max(0, atoi(llEnv)) : room)                 — field -1: room
    "ROMAN_LISTS_LDS": (INT_VALUES, {"lists_lds": (-1, 0, 0, 1, 7, 0, 0)}),
    # forced = teamEnv ? atoi(teamEnv) : c->wide_teams; if (teamEnv || c->wide_teams >= 0) ...
    "ROMAN_WIDE_TEAMS": (INT_VALUES, {"wide_teams_set": (0, 1, 1, 1, 1, 1, 1), "wide_teams": (0, 0, 0, 1, 7, -3, 0)}),
    # if (e_ && e_[0]) a_ccfg = (int)strtol(e_, nullptr, 0);
    "ROMAN_WIDE_COMPACT": (INT_VALUES + ("0x10",), {"wide_compact_set": (0, 0, 1, 1, 1, 1, 1, 1), "wide_compact": (0, 0, 0, 1, 7, -3, 0, 16)}),
    # if (tcap && !H.valid) S->capNnz = atoll(tcap);   /   if (tlist && !H.valid) S->capList = atoll(tlist);
    "ROMAN_TEST_CAPNNZ": (INT_VALUES, {"test_capnnz_set": (0, 1, 1, 1, 1, 1, 1), "test_capnnz": (0, 0, 0, 1, 7, -3, 0)}),
    "ROMAN_TEST_CAPLIST": (INT_VALUES, {"test_caplist_set": (0, 1, 1, 1, 1, 1, 1), "test_caplist": (0, 0, 0, 1, 7, -3, 0)}),
    # if (e) { v = atoi(e); if (v >= 1 && v <= 64) nx = v; }                          — field 0: the device's count
    "ROMAN_NUM_XCC": (INT_VALUES + ("64", "65"), {"num_xcc": (0, 0, 0, 1, 7, 0, 0, 64, 0)}),
    # if (e) { v = atof(e); if (v >= 0.0) ms = v; }                                   — field -1: the library's 4000 ms
    "ROMAN_WIDE_SPIN_MS": (INT_VALUES + ("2.5",), {"wide_spin_ms": (-1, 0, 0, 1, 7, -1, 0, 2.5)}),
}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("switches") / "switches_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-I", CSRC, "-o", str(exe), os.path.join(ROOT, "tests", "switches_main.cpp")])
    env = {k: v for k, v in os.environ.items() if not k.startswith("ROMAN_")}

    def run(*steps):
        """one process; the parsed struct of every `print` step as {(switch, field): number}"""
        out = subprocess.run([str(exe), *steps], env=env, capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        return [{tuple(w.split("=")[0].split(":")): float(w.split("=")[1]) for w in line.split()} for line in out.stdout.splitlines()]
    return run


def step(name, value):
    return f"-{name}" if value is None else f"{name}={value}"


def test_every_switch_is_in_the_table_and_read_nowhere_else(driver):
    printed = driver("print")[0]
    assert sorted({n for n, _ in printed}) == sorted(NAMES) == sorted(TABLE)
    assert sorted(f for _, f in printed) == sorted(f for _, (_, fields) in TABLE.items() for f in fields)     # every field has its expectations
    header = open(os.path.join(CSRC, "switches.h")).read()
    assert sorted(set(re.findall(r'getenv\("(\w+)"\)', header))) == sorted(NAMES)
    for f in os.listdir(CSRC):
        if f != "switches.h" and f.endswith((".hip", ".h")):
            assert "getenv" not in open(os.path.join(CSRC, f)).read(), f


def test_per_call_switches_parse_like_the_expressions_they_replace(driver):
    steps, want = [], []
    for name in NAMES:
        if name in ONCE:
            continue
        values, fields = TABLE[name]
        for k, v in enumerate(values):
            steps += [step(name, v), "print"]
            want.append((name, v, {f: e[k] for f, e in fields.items()}))
        steps.append(step(name, None))
    got = driver(*steps)
    assert len(got) == len(want)
    base = driver("print")[0]
    for g, (name, v, fields) in zip(got, want):
        for f, e in fields.items():
            assert g[(name, f)] == e, (name, v, f)
        assert {k: x for k, x in g.items() if k[0] != name} == {k: x for k, x in base.items() if k[0] != name}, (name, v)   # and touches no other switch


@pytest.mark.parametrize("k", range(len(FLAG_VALUES)))
def test_read_once_switches_parse_like_the_expressions_they_replace(driver, k):
    """(a process per value: the first read is the only one)"""
    got = driver(*[step(name, TABLE[name][0][k]) for name in ONCE], "print")[0]
    for name in ONCE:
        for f, e in TABLE[name][1].items():
            assert got[(name, f)] == e[k], (name, TABLE[name][0][k], f)


def test_both_uses_of_cos_block(driver):
    got = driver(*[s for v in (None, "", "0", "1", "2") for s in (step("ROMAN_COS_BLOCK", v), "print")])
    small = [g[("ROMAN_COS_BLOCK", "cos_block")] for g in got]                # maps of at most 48 objects: '1' always, anything else set never
    large = [g[("ROMAN_COS_BLOCK", "cos_block_large")] for g in got]          # larger maps: only '0' never
    assert small == [LIB, LIB, 0, 1, 0]
    assert large == [1, 1, 0, 1, 1]


def test_read_once_stays_and_per_call_follows(driver):
    a, b, c = driver("ROMAN_WIDE=1", "ROMAN_SMALL=0", "-ROMAN_DEBUG", "ROMAN_LISTS=1", "print",
                     "ROMAN_WIDE=0", "-ROMAN_SMALL", "ROMAN_DEBUG=1", "ROMAN_SMALL_FUSED=0", "ROMAN_SMALL_ONLY=0", "ROMAN_LISTS=0", "ROMAN_SORT_EQMAX=9", "print",
                     "-ROMAN_WIDE", "-ROMAN_LISTS", "print")
    once = [(n, f) for n in ONCE for f in TABLE[n][1]]
    assert [a[k] for k in once] == [0, 1, 1, 1, 0]                            # debug, wide, small_fused, small_only, small as first read
    assert [b[k] for k in once] == [c[k] for k in once] == [a[k] for k in once]
    assert (a[("ROMAN_LISTS", "lists")], b[("ROMAN_LISTS", "lists")], c[("ROMAN_LISTS", "lists")]) == (1, 0, LIB)
    assert (a[("ROMAN_SORT_EQMAX", "sort_eq_max")], b[("ROMAN_SORT_EQMAX", "sort_eq_max")]) == (512, 9)
