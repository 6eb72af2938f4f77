"""The cases of the wide fall-back's traceback tests (tests/wide_walk_cases.py), checked on the CPU alone with the twin (O.align_pair, as
tests/align_check.py runs it): EVERY pair ends in the fall-back -- (320, 0, .), or (320, 1, 0) for the two pairs it is meant to drop --
and the twin's path holds the runs each case is named for, to the step.  Without this the GPU test (test_gpu_wide_walk.py) could pass
on pairs that never reach align_wide_tb_runs_kernel, or whose gaps broke up into runs of other lengths."""
import numpy as np

import oracle_lib as O
import wide_walk_cases as WC
from align_check import twin, twin_class

_runs = {}


def runs(c):
    if c.name not in _runs:
        ops, ti, _ = twin(c.a, c.b, WC.CAP)
        _runs[c.name] = (twin_class(ti), None if ops is None else WC.runs_of(ops, len(c.b)), ops)
    return _runs[c.name]


def test_every_case_ends_in_the_fall_back():
    cases = WC.table() + WC.many()
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:
        cls, r, ops = runs(c)
        assert WC.is_class(c, cls), (c.name, cls)
        assert (ops is None) == c.dropped
        assert len(c.a) <= 2600 or c.name.startswith("K_long_centre"), c.name       # (the fall-back's own limit needs 1 024 more)
    assert sum(c.dropped for c in cases) == 2 and len(WC.many()) > 64


def test_the_paths_hold_the_runs_the_cases_are_named_for():
    for c in WC.table() + WC.many():
        cls, r, _ = runs(c)
        if r is None:
            continue
        d, l, u = r
        assert set(c.diag) <= set(d) and set(c.left) <= set(l) and set(c.up) <= set(u), (c.name, d, l, u)
        assert sum(d) + sum(u) == len(c.a) and sum(d) + sum(l) == len(c.b)
    by = {c.name: c for c in WC.table()}
    assert WC.DIAG_RUNS == (1, 63, 64, 65, 127, 128, 129) and WC.LEFT_RUNS == (1, 63, 64, 65, 200)
    for k in WC.DIAG_RUNS:                      # exactly k steps BETWEEN TWO GAPS: neither the first nor the last run of the path
        d = runs(by["K_diag_%d" % k])[1][0]
        assert k in d[1:-1]
    for k in WC.LEFT_RUNS:
        assert runs(by["K_left_%d" % k])[1][1] == [k]
    # both orders of an up and a left run around a diagonal run (front to back: the walk meets them the other way round)
    assert runs(by["K_diag_64"])[1][1:] == ([6], [WC.SEND, 5]) and runs(by["K_up_128_left"])[1][1:] == ([9], [WC.SEND, 7])


def test_the_edges_are_where_the_cases_say():
    by = {c.name: c for c in WC.table()}

    def ops_of(name):
        return runs(by[name])[2]

    o = ops_of("K_row_longer_at_both_ends")                    # 5 row bases in front of the first centre base, 6 behind the last
    assert int(o[0]) == 5 and int(o[-1]) == len(by["K_row_longer_at_both_ends"].b) - 7
    o = ops_of("K_centre_longer_at_both_ends")                 # 5 centre bases in front of the first row base, 6 behind the last
    assert (o[:5] >> 15).all() and (o[-6:] >> 15).all() and int(o[5]) == 0 and not int(o[-7]) >> 15
    o = ops_of("K_i_reaches_0")                                # the walk reaches row 0 with 30 columns to go
    assert int(o[0]) == 30
    o = ops_of("K_j_reaches_0")                                # ... column 0 with 20 rows to go
    assert (o[:20] >> 15).all() and int(o[20]) == 0
    # rows shorter than 64 bases, centres shorter than 64 rows
    assert sum(len(c.a) < 64 for c in by.values()) >= 2 and sum(len(c.b) < 64 for c in by.values()) >= 1
    # diagonal steps without a match: the stretches are aligned column to column
    c = by["K_mismatch_n_lower_in_row"]
    o = ops_of(c.name)
    for lo, hi in ((700, 790), (820, 890), (1010, 1030)):
        rows = [int(x) for x in o if not int(x) >> 15 and lo <= int(x) < hi]
        assert len(rows) >= hi - lo - 2, (lo, hi, len(rows))
    assert not np.isin(by["K_row_all_n"].b, list(b"ACGT")).any() and runs(by["K_row_all_n"])[1][0] == [len(by["K_row_all_n"].b)]
    # the dropped pairs are one base beyond the longest the fall-back keeps
    for kind in ("row", "centre"):
        kept, dropped = by["K_long_%s_kept" % kind], by["K_long_%s_dropped" % kind]
        assert len(dropped.a) + len(dropped.b) - len(kept.a) - len(kept.b) == 1
        assert O.align_pair(kept.a, kept.b, WC.CAP)[1]["status"] == 0 and O.align_pair(dropped.a, dropped.b, WC.CAP)[1]["status"] == 1
