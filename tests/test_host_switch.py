"""The table of the library's tri-state switches (hite_amd/csrc/hite_switch.h) on the HOST: a stand-alone program that includes the
header alone, built with g++ -std=c++17 -Wall -Werror, run as a child process once per setting of the environment.  Every child starts
without the five variables, so nothing of the caller's shell leaks in.  The program prints, per switch, what resolves with the
context's value at -1, 0 and 1 and what the setter's range check answers for -2 .. 2; the expected values are the rules, written out
below -- the program is not asked what they are."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "hite_switch.h"
#include <stdio.h>
int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "default")) {
        // the process default of the copy switch; the parent set HITE_COPY_INTERVAL=whole
        const HiteSwitch s = HITE_SW_COPY_INTERVAL;
        printf("%d", hite_switch_resolve(nullptr, s));
        setenv("HITE_COPY_INTERVAL", "aligned", 1);
        printf(" %d", hite_switch_resolve(nullptr, s));                     // resolved once: the first value sticks
        printf(" %d", (int)hite_switch_set_default(s, 1));
        setenv("HITE_COPY_INTERVAL", "whole", 1);
        printf(" %d", hite_switch_resolve(nullptr, s));                     // set: the environment is not asked
        printf(" %d", (int)hite_switch_set_default(s, 2));                  // refused, nothing stored
        printf(" %d", hite_switch_resolve(nullptr, s));
        printf(" %d", (int)hite_switch_set_default(s, -1));
        printf(" %d", hite_switch_resolve(nullptr, s));                     // -1: the environment again (whole)
        setenv("HITE_COPY_INTERVAL", "aligned", 1);
        printf(" %d", hite_switch_resolve(nullptr, s));                     // ... once
        printf(" %d", (int)hite_switch_set_default(s, -1));
        printf(" %d\n", hite_switch_resolve(nullptr, s));
        return 0;
    }
    for (int s = 0; s < HITE_SW_N; s++) {
        int32_t sw[HITE_SW_N];
        printf("%s", hite_switch_table[s].env);
        for (int v = -1; v <= 1; v++) {
            for (int32_t &x : sw) x = -1;
            sw[s] = v;
            printf(" %d", hite_switch_resolve(sw, (HiteSwitch)s));
        }
        for (int v = -2; v <= 2; v++) {
            for (int32_t &x : sw) x = 7;
            const bool ok = hite_switch_set(sw, (HiteSwitch)s, v);
            for (int q = 0; q < HITE_SW_N; q++)
                if (sw[q] != (ok && q == s ? v : 7)) return 2;              // stores the value in its own place, or nothing
            printf(" %d", (int)(ok && !hite_switch_set(nullptr, (HiteSwitch)s, v)));    // (no context: refused)
        }
        printf("\n");
    }
    return 0;
}
"""

SWITCHES = ("HITE_COPY_INTERVAL", "HITE_FILL_TILES", "HITE_GATHER_CHUNKS", "HITE_FALLBACK_OVERLAP", "HITE_WIDE_TB_RUNS")
# the values that mean 0; everything else -- unset, empty, "00", "1", "aligned" -- means 1
OFF = {"HITE_COPY_INTERVAL": ("0", "whole"), "HITE_FILL_TILES": ("0",), "HITE_GATHER_CHUNKS": ("0",), "HITE_FALLBACK_OVERLAP": ("0",),
       "HITE_WIDE_TB_RUNS": ("0",)}
RUNS = [{}] + [{v: x} for v in SWITCHES for x in ("0", "1", "", "00")] + [{"HITE_COPY_INTERVAL": "whole"}, {"HITE_COPY_INTERVAL": "aligned"}]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("switch")
    (d / "switch.cpp").write_text(PROGRAM)
    exe = d / "switch"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "hite_amd", "csrc"), "-o", str(exe), str(d / "switch.cpp")],
                   check=True)
    return str(exe)


def run(program, env_set, *args):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(env_set)
    return subprocess.run([program] + list(args), env=env, check=True, capture_output=True, text=True).stdout


@pytest.mark.parametrize("env_set", RUNS, ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()) or "nothing set")
def test_resolve_and_range_check(program, env_set):
    lines = run(program, env_set).splitlines()
    assert [ln.split()[0] for ln in lines] == list(SWITCHES)
    for name, ln in zip(SWITCHES, lines):
        got = [int(x) for x in ln.split()[1:]]
        from_env = 0 if name in env_set and env_set[name] in OFF[name] else 1
        #       context at -1: the environment; at 0 and 1: the context     the setter accepts -1, 0, 1
        assert got == [from_env, 0, 1] + [0, 1, 1, 1, 0], (name, env_set, got)


def test_the_process_default_of_the_copy_switch(program):
    out = run(program, {"HITE_COPY_INTERVAL": "whole"}, "default")
    #                   whole sticks  set(1) ok -> 1  set(2) refused -> 1  set(-1) ok -> whole, sticks  set(-1) ok -> aligned
    assert out.split() == ["0", "0", "1", "1", "0", "1", "1", "0", "0", "1", "1"]
