"""CPU-only: the host layer of FiLTR's steps 4 to 8 in hite_amd/util.py against what the reference's own functions made of the same
inputs (tests/golden/ltr_library.json.gz, written by tools/gen_ltr_library_fixture.py): get_intact_ltr_copies -- util's restatement
on dicts and tests/ltrcopy_twin.py, the definition the device is held to --, search_ltr_structure / is_ltr_has_structure,
estimate_insert_time, filter_single_copy_ltr (the protein search replaced by the recorded tables), get_LTR_seq_from_scn file for
file, assign_label_to_lib, filter_ltr_by_copy_num with the twin in place of the device, and the generator of the genome."""
import os

import pytest

import ltrcopy_cases as LC
import ltrcopy_twin as LT
from conftest import load_golden


@pytest.fixture(scope="module")
def gold():
    return load_golden("ltr_library")


@pytest.fixture()
def genome(gold, tmp_path):
    from hite_amd import util

    ref, scn = str(tmp_path / "ref.fa"), str(tmp_path / "in.scn")
    util.store_fasta(gold["contigs"], ref)
    with open(scn, "w") as f:
        f.write(gold["scn"])
    _cand, ltr_lines = util.read_scn(scn, None)
    _terms, l2c = util.left_ltr_terminals(scn, gold["contigs"])
    return ref, scn, ltr_lines, l2c


def test_the_genome_regenerates(gold):
    from hite_amd import synth

    g = synth.make_ltr_library_genome(seed=20251021)
    assert g["contigs"] == gold["contigs"] and g["scn"] == gold["scn"] and g["truth"] == gold["truth"]
    fams = {}
    for t in g["truth"]:
        fams.setdefault(t["family"], []).append(t)
    assert sorted(len(v) for f, v in fams.items() if f >= 0) == [1, 1, 1, 2, 2, 5] and {t["tsd"] for t in g["truth"]} == {None, 4, 5, 6}
    assert sum(t["line"] is None for t in g["truth"]) == 1 and any(t["name"].split("-")[1] == "1" for t in g["truth"])
    last = [t for t in g["truth"] if t["family"] == -2][0]
    assert int(last["line"].split(" ")[7]) == len(g["contigs"][last["chr"]])


def test_get_intact_ltr_copies_crafted(gold, tmp_path):
    from hite_amd import util

    cases = {c["label"]: c for c in LC.crafted()}
    assert [c["label"] for c in gold["crafted"]] == list(cases)
    for gc in gold["crafted"]:
        c = cases[gc["label"]]
        assert gc["std"] == [list(t) for t in c["std"]] and gc["contig_len"] == c["contig_len"]
        covered = [[tuple(r[:3]) for r in recs if LT.cover_ok(L, r[3], r[1], r[2], 0.985)] for L, recs in zip(c["el_len"], c["records"])]
        assert [[list(r) for r in recs] for recs in covered] == gc["covered"]
        exp = {n: [tuple(x) for x in v] for n, v in gc["intact_ltr_copies"]}
        # the twin: the records that passed the coverage rule, every one covered again (clip 0, coverage 0)
        got = LT.support_records([1] * len(covered), [[r + (0,) for r in recs] for recs in covered], c["std"], c["contig_len"], full_length_coverage=0.0)
        assert {"el%d" % k: v for k, v in enumerate(got) if v} == exp
        # ... and from the raw records, the coverage rule included
        got = LT.support_records(c["el_len"], c["records"], c["std"], c["contig_len"])
        assert {"el%d" % k: v for k, v in enumerate(got) if v} == exp
        # util's restatement on the reference's dicts, the order of the keys included
        names = ["ctg%d" % k for k in range(len(c["contig_len"]))]
        lines = {k: " ".join(str(x) for x in (s + 1, e, e - s, s + 1, s + 100, 100, e - 99, e, 100, "95.00", k, names[ct])) for k, (ct, s, e) in enumerate(c["std"])}
        copies = {"el%d" % k: [(names[r[0]], r[1], r[2], r[2] - r[1] + 1, "+") for r in recs] for k, recs in enumerate(covered) if recs}
        res = util.get_intact_ltr_copies(copies, lines, 0.95, (names, {n: "A" * ln for n, ln in zip(names, c["contig_len"])}))
        assert [[n, [[names.index(x[0]), x[1], x[2]] for x in v]] for n, v in res.items()] == gc["intact_ltr_copies"]


def test_get_intact_ltr_copies_genome(gold, genome):
    from hite_amd import util

    ref, _scn, ltr_lines, l2c = genome
    ltr_copies = {n: [tuple(r) for r in v] for n, v in gold["ltr_copies"]}
    res = util.get_intact_ltr_copies(ltr_copies, ltr_lines, 0.95, ref)
    assert [[n, [list(r) for r in v]] for n, v in res.items()] == gold["intact_ltr_copies"]
    names = list(gold["contigs"])
    std = util._scn_std(ltr_lines, {n: k for k, n in enumerate(names)})
    order = list(ltr_copies)
    got = LT.support_records([1] * len(order), [[(names.index(r[0]), r[1], r[2], 0) for r in ltr_copies[n]] for n in order], std,
                             [len(gold["contigs"][n]) for n in names], full_length_coverage=0.0)
    assert {n: [[names[c], s, e] for c, s, e in v] for n, v in zip(order, got) if v} == dict((n, v) for n, v in gold["intact_ltr_copies"])
    assert sorted(len(v) for _n, v in gold["intact_ltr_copies"]) == [1, 1, 1, 1, 1, 2, 2, 2, 2, 4, 4, 4, 4]


def test_filter_ltr_by_copy_num_with_the_twin(gold, genome, tmp_path):
    """the whole of step 4's search through the finder's twin: the dict the reference's rules gave on the twin's copies"""
    from hite_amd import util

    ref, _scn, ltr_lines, l2c = genome
    names = list(gold["contigs"])
    table = str(tmp_path / "msa_flank.txt")
    with open(table, "w") as f:
        for k, n in enumerate(l2c):
            f.write("%s\t%d\n" % (n, k != 3))
    seen = []

    def support(elements, std, cover, thr):
        seen.append((len(elements), cover, thr))
        return LT.support([gold["contigs"][n] for n in names], elements, std, cover, thr)

    copies, internal = util.filter_ltr_by_copy_num(table, l2c, ltr_lines, ref, str(tmp_path), None, 1, 0.95, 0, support=support)
    assert seen == [(len(l2c) - 1, 0.985, 0.95)]
    skipped = list(l2c)[3]
    exp = {n: [tuple(r) for r in v] for n, v in gold["intact_ltr_copies"] if n != skipped}
    assert copies == exp and list(copies) == [n for n in l2c if n in exp] and set(internal) == set(l2c) - {skipped}
    p = ltr_lines[l2c[list(l2c)[0]]].split(" ")
    assert internal[list(l2c)[0]] == gold["contigs"][p[11]][int(p[4]):int(p[6]) - 1]


def test_structure_and_insert_time(gold, genome):
    from hite_amd import util

    _ref, _scn, ltr_lines, l2c = genome
    for name, exp in gold["structure"]:
        line = ltr_lines[l2c[name]]
        assert list(util.is_ltr_has_structure(name, line, gold["contigs"][line.split(" ")[11]])) == exp
    by_name = {t["name"]: t for t in gold["truth"]}
    for name, (_n, has, tsd) in gold["structure"]:
        t = by_name[name]
        if t["tsd"] and t["family"] >= 0:
            assert has and len(tsd) >= min(t["tsd"], 4)
    assert [r[1] for n, r in gold["structure"] if by_name[n]["family"] < 0] == [False, False]          # the windows cut at the chromosome ends
    assert sum(1 for _n, r in gold["structure"] if not r[1]) >= 3
    for left, right, exp in gold["windows"]:
        assert list(util.search_ltr_structure("w", left, right)) == exp
    assert {len(w[2][2]) for w in gold["windows"]} == {0, 4, 5, 6} and [w[2][1] for w in gold["windows"]].count(False) >= 3
    for identity, miu, exp in gold["insert_time"]:
        assert util.estimate_insert_time(identity, miu) == exp
    assert gold["insert_time"][0][2] == 0.0


def test_filter_single_copy_ltr(gold, genome, tmp_path, monkeypatch):
    from hite_amd import util

    ref, _scn, ltr_lines, l2c = genome
    libs = {}
    for lib, prot in gold["proteins"].items():
        libs[lib] = str(tmp_path / lib)
        util.store_fasta(prot, libs[lib])

    def domain_info(cons, lib, output_table, threads, temp_dir, search=None, ctx=None):
        with open(output_table, "w") as f:
            f.write("TE_name\tdomain_name\tTE_start\tTE_end\tdomain_start\tdomain_end\n\n")
            for r in gold["domain_tables"][os.path.basename(lib)]:
                f.write("\t".join(str(x) for x in r) + "\n")

    monkeypatch.setattr(util, "get_domain_info", domain_info)
    intact = {n: [tuple(r) for r in v] for n, v in gold["intact_ltr_copies"]}
    p = ltr_lines
    internal = {n: gold["contigs"][p[k].split(" ")[11]][int(p[k].split(" ")[4]):int(p[k].split(" ")[6]) - 1] for n, k in l2c.items()}
    homo, filtered = str(tmp_path / "homo.txt"), str(tmp_path / "filtered.txt")
    util.filter_single_copy_ltr(homo, filtered, str(tmp_path / "single.fa"), intact, internal, libs["LTRPeps.lib"], libs["OtherPeps.lib"], str(tmp_path),
                                1, ref, l2c, ltr_lines, None, 0)
    assert open(homo).read() == gold["intact_LTR_homo"] and open(filtered).read() == gold["filtered_single_copy_LTRs"]
    assert not os.path.exists(str(tmp_path / "single.fa"))
    reasons = {ln.split("\t")[1] for ln in gold["filtered_single_copy_LTRs"].splitlines()}
    assert len(reasons) >= 2 and {ln.split("\t")[1] for ln in gold["intact_LTR_homo"].splitlines()} == {"0", "1"}
    # without the libraries: said in the log, and the rule runs on empty tables -- no single-copy element stays
    said = []
    log = type("L", (), {"logger": type("G", (), {"info": staticmethod(said.append), "debug": staticmethod(said.append)})})
    util.filter_single_copy_ltr(homo, filtered, str(tmp_path / "single.fa"), intact, internal, str(tmp_path / "none" / "LTRPeps.lib"),
                                str(tmp_path / "none" / "OtherPeps.lib"), str(tmp_path), 1, ref, l2c, ltr_lines, log, 0)
    assert sum("not found" in s for s in said) == 2
    rows = [ln.split("\t") for ln in open(homo).read().splitlines()]
    assert [r[0] for r in rows] == list(intact) and all((r[1] == "1") == (len(intact[r[0]]) >= 2) for r in rows)
    assert all("no_intact_protein" in ln for ln in open(filtered).read().splitlines())


def test_get_LTR_seq_from_scn_file_for_file(gold, genome, tmp_path):
    from hite_amd import util

    ref = genome[0]
    scn = str(tmp_path / "six.scn")
    with open(scn, "w") as f:
        f.write(gold["six_scn"])
    out = {k: str(tmp_path / k) for k in gold["step6"]}
    util.get_LTR_seq_from_scn(ref, scn, out["confident_ltr.terminal.fa"], out["confident_ltr.internal.fa"], out["intact_LTR.fa"], gold["dirty_dicts"],
                              out["intact_LTR.list"], gold["miu"])
    for k, text in gold["step6"].items():
        assert open(out[k]).read() == text and text, k
    rows = [ln.split("\t") for ln in gold["step6"]["intact_LTR.list"].splitlines()]
    n_lines = len(gold["six_scn"].splitlines()) - 1
    assert len(rows) == n_lines - 2                       # the covered neighbour and, as in the reference, the last line
    assert {r[3] for r in rows} > {"TSD:NA"} and all(r[2] == "motif:TGCA" for r in rows[1:]) and {r[-1] for r in rows} > {"0"}
    assert gold["step6"]["confident_ltr.internal.fa"].count(">") == gold["step6"]["intact_LTR.fa"].count(">") - 1        # the dirty element


def test_assign_label_to_lib(gold, tmp_path):
    from hite_amd import util

    src = {"confident_ltr_cut.fa": gold["step6"]["confident_ltr.terminal.fa"] + gold["step6"]["confident_ltr.internal.fa"],
           "confident_ltr.terminal.fa": gold["step6"]["confident_ltr.terminal.fa"], "confident_ltr.internal.fa": gold["step6"]["confident_ltr.internal.fa"]}
    for k, text in src.items():
        path = str(tmp_path / k)
        with open(path, "w") as f:
            f.write(text)
        util.assign_label_to_lib(path, gold["labels"])
        assert open(path).read() == gold["labelled"][k] and "#LTR/" in gold["labelled"][k], k
    # (the reference's names end in -LTR and -int here: what it looks for, _LTR and _INT, are the names of its LTR_retriever branch)
    assert "-int#" in gold["labelled"]["confident_ltr_cut.fa"] and "-LTR#" in gold["labelled"]["confident_ltr_cut.fa"]
