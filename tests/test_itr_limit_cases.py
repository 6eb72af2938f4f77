"""CPU: the records of tests/itr_limit_cases.py reach the limits they are named for (shown with the plain restatement of the
definition, counts printed), the restatement equals the twin (oracle/hite_oracle_itr.c) on every one of them and on the inputs of
tests/golden/itr_search.json.gz, the twin equals the tool at the limits (tests/golden/itr_limits.json.gz), no case takes the path
on which the tool's stale state would matter (flags 0), and every check_* that tests/test_gpu_itr_limits.py runs on the device
passes with the twin in the device's place."""
import numpy as np

import itr_limit_cases as IC
from conftest import load_golden


def test_table_is_what_the_cases_assume():
    assert IC.STRIP == 64 and IC.LDS_H == IC.STRIP and IC.MAX_H > 3 * IC.STRIP + 1 and IC.MAX_H % IC.STRIP != 0
    assert IC.closed_ks() == (6, 7, 8, 63, 64, 65, 127, 128, 129, 191, 192, 193, 499, 500, 501, 600)
    assert IC.seam_ps() == list(range(60, 67)) + list(range(126, 131)) + list(range(190, 195))
    assert IC.GUARD_MAX_H == (0, 63, 64, 65, 499, 500, 10000)


def test_flags_are_zero_on_every_case():
    n = 0
    for name, cases in IC.all_families() + [("guard", IC.guard_batch())]:
        rows = IC.twin(name, cases)
        assert int(rows[:, 7].max()) == 0, name
        n += len(cases)
    hbm, lds = IC.slot_batches()
    print("itr limits: %d distinct cases, twin flags 0 on all; slot batches of %d and %d records" % (n, len(hbm), len(lds)))
    assert len(hbm) == 4 * IC.HBM_BLOCKS + 5 and len(lds) == 4 * IC.LDS_BLOCKS + 7 and max(len(c[1]) for c in lds) <= 80


def test_restatement_equals_twin_on_every_case():
    for name, cases in IC.all_families() + [("guard", IC.guard_batch())]:
        rows = IC.twin(name, cases)
        got = np.asarray([IC.restate_case(c)[0] for c in cases], dtype=np.int32)
        IC.assert_rows(got, rows, cases, "restatement, " + name)
        print("itr limits: restatement == twin on %d cases of %s" % (len(cases), name))


def test_restatement_equals_twin_on_the_tool_fixture_inputs():
    g = load_golden("itr_search")
    n = 0
    for part, step, e in (("pairs", 12, 0), ("pairs", 29, 40), ("whole", 6, 0)):
        cases = [IC.case("%s #%d" % (part, k), s, e) for k, s in list(enumerate(g[part]["seqs"]))[::step]]
        got = np.asarray([IC.restate_case(c)[0] for c in cases], dtype=np.int32)
        IC.assert_rows(got, IC.run(IC.twin_search, cases), cases, "restatement, " + part)
        n += len(cases)
    print("itr limits: restatement == twin on %d inputs of the tool fixture" % n)
    assert n > 350


def test_closed_form():
    cases, rows = IC.closed_form()
    assert IC.check_closed_form(IC.twin_search) == len(cases) == 3 * 16 * 3
    by = dict((c[0], r) for c, r in zip(cases, rows.tolist()))
    assert by["closed k=6 spacer=0 (10, 16, 32, 32)"] == IC.EMPTY_ROW
    assert by["closed k=7 spacer=0 (10, 16, 32, 32)"] == [6, 7, 7, 7, 7, 1, 6, 0]
    assert by["closed k=501 spacer=1 (10, 16, 32, 32)"] == by["closed k=600 spacer=2 (10, 16, 32, 32)"] == [4936, 500, 500, 500, 500, 1, 499, 0]
    got = np.asarray([IC.restate_case(c)[0] for c in cases], dtype=np.int32)
    IC.assert_rows(got, rows, cases, "restatement == closed form")
    assert all(len(IC.restate_case(c)[1]["cells"]) <= 1 for c in cases), "the maximum of a perfect repeat is alone"


def test_seams_reach_the_boundaries():
    cases = IC.seams()
    reach, row1 = IC.seam_reach(cases)
    gapped = sum(1 for c in cases if c[0].startswith("seam") and IC.restate_case(c)[1]["gaps"])
    print("itr limits: %d seam cases, %d with a gap on the path; gaps across a boundary %s; %d alignments enter row 1 at the first "
          "column of a later strip" % (len(cases), gapped, sorted(reach.items()), row1))
    for b in (IC.STRIP, 2 * IC.STRIP, 3 * IC.STRIP):
        for kind in "EF":
            assert reach.get((kind, b), 0) >= 5, (kind, b, reach)
    assert row1 >= 5
    assert IC.check_seams(IC.twin_search) == len(cases)


def test_ties_reach_two_strips_and_one_lane():
    cases = IC.ties()
    fewest, strips, same_lane = IC.tie_reach(cases)
    print("itr limits: %d tie cases, at least %d cells at the maximum in each; first and last in different strips in %d; two in one row "
          "a multiple of 64 columns apart (one lane, two strips) in %d" % (len(cases), fewest, strips, same_lane))
    assert fewest >= 2 and strips >= 5 and same_lane >= 5
    rows = IC.twin("ties", cases)
    for c, r in zip(cases, rows):
        assert (int(r[1]), int(r[2])) == IC.restate_case(c)[1]["cells"][0], c[0]
    assert IC.check_ties(IC.twin_search) == len(cases)


def test_alphabet_and_thresholds():
    cases, found = IC.alphabet()
    rows = IC.twin("alphabet", cases)
    by = dict((c[0], r.tolist()) for c, r in zip(cases, rows))
    for h in (IC.LDS_H, IC.LDS_H + 1, IC.MAX_H):
        assert by["all N h=%d" % h] == [10 * h - 64, h, h, h, h, 1, h - 1, 0]
    n_thr = sum(f is not None for f in found)
    print("itr limits: %d alphabet / threshold cases, %d with `found` in closed form (%d found)" % (len(cases), n_thr, sum(f or 0 for f in found)))
    assert n_thr == len(IC.IDENT_FRACTIONS) * len(IC.IDENT_THRESHOLDS) + 4
    for (m, n) in IC.IDENT_FRACTIONS:
        r = by["identity %d/%d at 0.7" % (m, n)]
        assert r[3:5] == [m, n] and r[1] == n, r
    # lower case and IUPAC fold to N on both ends: the same rows as the record with N written out
    for c, r in zip(cases, rows):
        if c[0].startswith("letters"):
            folded = "".join(ch if ch in "ACGT" else "N" for ch in c[1])
            assert IC.twin_search([folded], c[2]).tolist() == [r.tolist()] and folded != c[1]
    assert IC.check_alphabet(IC.twin_search) == len(cases)


def test_rules_are_told_apart():
    """cases whose row changes when a tie of open and extend marks an opening, and when an N of seq2 is no wildcard"""
    planted = [c for c in IC.seams() if c[0].startswith("open tie E")]
    short = planted + IC.seams()[::6]
    tie = sum(IC.restate_case(c, tie_opens=True)[0] != IC.restate_case(c)[0] for c in short)
    tie_planted = sum(IC.restate_case(c, tie_opens=True)[0] != IC.restate_case(c)[0] for c in planted)
    wild = sum(IC.restate_case(c, n2_wild=False)[0] != IC.restate_case(c)[0] for c in IC.alphabet()[0])
    print("itr limits: %d of %d seam cases change under open-on-tie (%d of the %d planted), %d of %d alphabet cases without the N wildcard "
          "of seq2" % (tie, len(short), tie_planted, len(planted), wild, len(IC.alphabet()[0])))
    assert tie_planted >= 10
    assert tie >= 5 and wild >= 5


def test_lengths():
    cases = IC.lengths()
    rows = IC.twin("lengths", cases)
    by = dict((c[0], r.tolist()) for c, r in zip(cases, rows))
    for L in (0, 1, 2, 3, 12, 13):
        assert by["whole L=%d" % L] == IC.EMPTY_ROW
    assert by["whole L=14"] == by["whole L=15"] == [6, 7, 7, 7, 7, 1, 6, 0]
    hs = [IC.h_of(c) for c in cases]
    print("itr limits: %d length cases, h from %d to %d, %d at the cap, %d with overlapping ends" % (
        len(cases), min(hs), max(hs), hs.count(IC.MAX_H), sum(1 for c in cases if c[2] > 0 and len(c[1]) < 2 * min(c[2], IC.MAX_H))))
    assert hs.count(IC.MAX_H) >= 10 and min(hs) == 0
    assert IC.check_lengths(IC.twin_search) == len(cases)


def test_bands():
    cases = IC.bands()
    hs = np.asarray([IC.h_of(c) for c in cases])
    found = int(IC.twin("bands", cases)[:, 5].sum())
    print("itr limits: %d band records, h <= 64: %d, 65 .. 128: %d, above: %d, at the cap: %d; %d found" % (
        len(cases), int((hs <= 64).sum()), int(((hs > 64) & (hs <= 128)).sum()), int((hs > 128).sum()), int((hs == IC.MAX_H).sum()), found))
    assert len(cases) == 1500 and set(range(60, 71)) | set(range(124, 133)) | set(range(495, 501)) == set(hs.tolist())
    assert len({c[3] for c in cases}) == 4 and found > 500
    assert IC.check_bands(IC.twin_search) == len(cases)


def test_path_equivalence_and_order():
    n, n_hbm = IC.check_path_equivalence(IC.twin_search)
    m, lo, hi = IC.check_order(IC.twin_search)
    print("itr limits: %d records of h <= %d in %d groups, %d of them beside a record of h = %d; order batch of %d, h %d .. %d" % (
        n, IC.LDS_H, len(IC.short_groups()[0]), n_hbm, IC.LDS_H + 1, m, lo, hi))
    assert n_hbm > 500 and lo <= 7 and hi == IC.MAX_H
    assert IC.h_of(IC.case("", IC.short_groups()[1])) == IC.LDS_H + 1


def test_slot_batches():
    hbm, lds = IC.slot_batches()
    slots = IC.HBM_BLOCKS * IC.WAVES
    after_long = sum(1 for k in range(slots, len(hbm)) if IC.h_of(hbm[k]) < IC.h_of(hbm[k - slots]))
    hs = sorted({IC.h_of(c) for c in hbm})
    assert hs == list(range(IC.LDS_H + 1, IC.LDS_H + 7)) + [IC.MAX_H] and after_long >= 2
    gaps = sum(1 for c in IC.slot_pool() if c[0].startswith("slot long") and IC.restate_case(c)[1]["gaps"])
    slots = IC.LDS_BLOCKS * IC.WAVES
    assert all(IC.h_of(lds[k]) < IC.h_of(lds[k - slots]) for k in range(slots, len(lds)))
    print("itr limits: HBM batch of %d, %d short records follow a long one through their slot, %d of 10 long records with a gap; "
          "LDS batch of %d" % (len(hbm), after_long, gaps, len(lds)))
    assert gaps >= 8
    assert IC.check_slots(IC.twin_search, 0) == len(hbm) and IC.check_slots(IC.twin_search, 1) == len(lds)


def test_guard_table():
    cases = IC.guard_batch()
    hs = [IC.h_of(c) for c in cases]
    skipped = dict((mh, int((IC.guard_expected(mh)[:, 7] == 8).sum())) for mh in IC.GUARD_MAX_H)
    print("itr limits: guard batch h = %s; rows skipped per max_h: %s" % (hs, skipped))
    assert skipped[0] == len(cases) - 1 and skipped[IC.MAX_H] == skipped[10000] == 0 and skipped[IC.LDS_H] == skipped[IC.LDS_H + 1] + 1
    assert IC.guard_expected(0)[0].tolist() == IC.EMPTY_ROW
    # the twin in the place of the device entry: a record beyond max_h is skipped, every other row is the twin's
    def model(seqs, e, mh):
        rows = np.array(IC.twin_search(seqs, e))
        for k, s in enumerate(seqs):
            if min(IC.MAX_H, len(s) // 2) > mh:
                rows[k] = IC.SKIPPED_ROW
        return rows
    assert IC.check_max_h(model) == len(cases)


def test_twin_equals_the_tool_at_the_limits():
    n, n_found = IC.check_fixture(IC.twin_search, load_golden("itr_limits"))
    print("itr limits: twin == the tool on %d records at -i 0.7 -l 7 and -i 0.8 -l 10 (%d found)" % (n, n_found))
    assert n >= 300 and n_found > 200
