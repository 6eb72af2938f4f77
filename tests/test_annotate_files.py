"""CPU-only: the host layer of the genome annotation (hite_amd/util.py: annotation_columns, the RepeatMasker-layout writers, the
restated reader get_full_length_copies_from_gff_v1 with FMEA_new, annotate_genome) and the parsers of the two drop-in scripts.  The
device stage is replaced by the twin (annot=); tests/golden/annotate_gff.json.gz holds what the reference's own reader makes of this
build's GFF (tools/gen_annotate_fixture.py)."""
import importlib.util
import json
import os

import numpy as np
import pytest

import annotate_cases as AC
import annotate_twin as AT
from conftest import load_golden
from hite_amd import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _script(name):
    spec = importlib.util.spec_from_file_location("annot_script_" + name, os.path.join(ROOT, "hite_amd", "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _count(lib_row, genome_row):
    """a brute count on an alignment written out by hand: (record fields score, matches, columns), mismatches, gaps in either row"""
    assert len(lib_row) == len(genome_row)
    m = sum(a == b and a != "-" for a, b in zip(lib_row, genome_row))
    gl, gg = lib_row.count("-"), genome_row.count("-")
    x = len(lib_row) - m - gl - gg
    return (2 * m - 4 * x - 5 * (gl + gg), m, len(lib_row)), x, gl, gg


ALIGNMENTS = [("ACGTACGTAC", "ACGTACGTAC"), ("ACGTACGTAC", "ACGAACGTAC"), ("ACGTACGTACGT", "ACG-ACGTACGT"), ("ACG-TACGTACG", "ACGGTACGTACG"),
              ("ACGTACGT--ACGTTT", "ACCTAC-TGGACGATT"), ("AC--GTACGTA-CGT", "ACTTGTAC-TAACGA")]


@pytest.mark.parametrize("lib_row,genome_row", ALIGNMENTS)
def test_annotation_columns_vs_a_brute_count(lib_row, genome_row):
    (score, m, cols), x, gl, gg = _count(lib_row, genome_row)
    q_len, g_len = len(lib_row) - gl, len(genome_row) - gg
    rec = (0, 100, 100 + g_len, 0, 0, 5, 5 + q_len, score, m, cols)
    assert util.annotation_columns(rec) == (x, gl, gg) == util.annotation_columns(rec, g_len, q_len)
    assert gl + gg == 6 * m - 4 * cols - score


def test_the_gap_counts_sum_to_g_on_every_record_of_every_case():
    n = 0
    for c in AC.small_cases():
        recs, _status = AT.annotate(c["seqs"], c["lib"], c["piece_len"])
        for r in recs:
            x, gl, gg = util.annotation_columns(r)
            assert gl + gg == 6 * r[8] - 4 * r[9] - r[7] and x >= 0 and gl >= 0 and gg >= 0 and r[8] + x + gl + gg == r[9], (c["label"], r)
            n += 1
    assert n >= 25
    recs = AC.planted_twin()[0]
    assert all(sum(util.annotation_columns(r)[1:]) == 6 * r[8] - 4 * r[9] - r[7] and min(util.annotation_columns(r)) >= 0 for r in recs)
    assert sum(sum(util.annotation_columns(r)[1:]) > 0 for r in recs) > 100      # copies with indels


# (seq, g_start, g_end, lib, strand, q_start, q_end, score, matches, columns)
TABLE = [(0, 99, 1099, 0, 0, 0, 1000, 2000, 1000, 1000),                # a whole copy
         (0, 1999, 2499, 1, 1, 100, 600, 2 * 480 - 4 * 20, 480, 500),   # C, 20 mismatches of 500: 4.0
         (1, 0, 300, 2, 0, 50, 352, 2 * 290 - 4 * 7 - 5 * 8, 290, 305),  # 7 mismatches, 3 gaps in the library row, 5 in the genome row
         (1, 400, 500, 1, 1, 0, 100, 2 * 97 - 4 * 3, 97, 100)]           # C at the first base of the entry; 3.0
REF_NAMES, REF_LENS = ["chr1", "scaffold_2"], [5000, 500]
LIB_NAMES, LIB_LENS = ["TE_a#DNA/hAT", "TE_b#LTR/Gypsy", "TE_c"], [1000, 700, 400]
OUT_LINES = ["  2000   0.0  0.0  0.0  chr1      100     1099 (3901) + TE_a DNA/hAT      1   1000    (0)     1\n",
             "   880   4.0  0.0  0.0  chr1     2000     2499 (2501) C TE_b LTR/Gypsy  (100)    600    101     2\n",
             "   512   2.4  1.7  1.0  scaffold_2        1      300 (200) + TE_c Unknown     51    352   (48)     3\n",
             "   182   3.0  0.0  0.0  scaffold_2      401      500 (0) C TE_b LTR/Gypsy  (600)    100      1     4\n"]
GFF_LINES = ["##gff-version 2\n",
             "chr1\tRepeatMasker\tdispersed_repeat\t100\t1099\t0.0\t+\t.\tTarget \"Motif:TE_a\" 1 1000\n",
             "chr1\tRepeatMasker\tdispersed_repeat\t2000\t2499\t4.0\t-\t.\tTarget \"Motif:TE_b\" 101 600\n",
             "scaffold_2\tRepeatMasker\tdispersed_repeat\t1\t300\t2.4\t+\t.\tTarget \"Motif:TE_c\" 51 352\n",
             "scaffold_2\tRepeatMasker\tdispersed_repeat\t401\t500\t3.0\t-\t.\tTarget \"Motif:TE_b\" 1 100\n"]


def test_out_lines_of_a_fixed_table(tmp_path):
    assert util.annotation_columns(TABLE[2]) == (7, 3, 5)
    path = tmp_path / "x.out"
    util.write_repeatmasker_out(TABLE, REF_NAMES, REF_LENS, LIB_NAMES, LIB_LENS, str(path))
    lines = open(path).readlines()
    assert len(lines) == 3 + len(TABLE) and lines[0].split()[:2] == ["SW", "perc"] and lines[1].split()[0] == "score" and lines[2] == "\n"
    assert lines[3:] == OUT_LINES
    assert all(len(ln.split()) == 15 for ln in lines[3:]) and not os.path.exists(str(path) + ".tmp")
    # one-decimal rounding: 7 / 297 = 2.357 -> 2.4, 5 / 300 = 1.667 -> 1.7, 3 / 300 -> 1.0


def test_gff_lines_of_a_fixed_table(tmp_path):
    path = tmp_path / "x.gff"
    util.write_repeatmasker_gff(TABLE, REF_NAMES, LIB_NAMES, str(path))
    assert open(path).readlines() == GFF_LINES
    recs, last = util.read_repeatmasker_gff(str(path))
    assert last == "TE_b" and recs["TE_b"] == {"chr1": [(101, 600, 2000, 2499)], "scaffold_2": [(1, 100, 401, 500)]}


def _golden_files(tmp_path, g):
    lib_path, ref_path = str(tmp_path / "lib.fa"), str(tmp_path / "genome.fa")
    for path, seqs in ((lib_path, g["lib"]), (ref_path, g["genome"])):
        with open(path, "w") as f:
            for name, s in seqs:
                f.write(">%s\n%s\n" % (name, s))
    return lib_path, ref_path, {name.split("#")[0]: name.split("#")[1] for name, _s in g["lib"]}


def test_the_gff_read_back_equals_what_the_reference_s_reader_made_of_it(tmp_path):
    g = load_golden("annotate_gff")
    lib_path, ref_path, te_classes = _golden_files(tmp_path, g)
    assert len(g["records"]) >= 55 and len(g["lib"]) == 6 and len(g["genome"]) == 3 and len(g["variants"]) == 2
    for v in g["variants"]:
        gff_path = str(tmp_path / "annot.gff")
        util.write_repeatmasker_gff(v["records"], [n for n, _s in g["genome"]], [n for n, _s in g["lib"]], gff_path)
        assert open(gff_path).read() == v["gff"]                      # the writer still writes what the reference's reader was given
        copies, flank, annotations = util.get_full_length_copies_from_gff_v1(lib_path, ref_path, gff_path, g["full_length_threshold"], te_classes)
        assert copies == v["full_length_copies"] and list(copies) == list(v["full_length_copies"]), v["label"]
        assert flank == v["flank_full_length_copies"]
        assert json.loads(json.dumps(annotations)) == v["full_length_annotations"]
        assert [list(x) for x in copies.values()] == [list(x) for x in v["full_length_copies"].values()]      # the order inside an entry
    a, b = (v["flank_full_length_copies"] for v in g["variants"])
    assert a != b and any(len(s) == 400 + 10 for s in b["Chr1-Helitron_7"].values()) and any(len(s) == 400 + 100 for s in a["Chr1-Helitron_7"].values())
    n_full = sum(len(x) for x in g["variants"][0]["full_length_annotations"].values())
    assert 20 <= n_full < len(g["records"])                           # some chains and copies fall short of 95 %


def test_an_empty_gff(tmp_path):
    g = load_golden("annotate_gff")
    lib_path, ref_path, te_classes = _golden_files(tmp_path, g)
    gff_path = str(tmp_path / "empty.gff")
    util.write_repeatmasker_gff([], [], [], gff_path)
    assert util.get_full_length_copies_from_gff_v1(lib_path, ref_path, gff_path, 0.95, te_classes) == ({}, {}, {})


def test_tbl_union_of_bases_vs_a_bit_map(tmp_path):
    rng = np.random.default_rng(8)
    ref_lens = [3000, 1200]
    lib_names = ["a#DNA/hAT", "b#DNA/hAT", "c#LTR/Copia", "d"]
    recs = []
    for _ in range(60):
        seq = int(rng.integers(0, 2))
        gs = int(rng.integers(0, ref_lens[seq] - 10))
        ge = min(ref_lens[seq], gs + int(rng.integers(1, 400)))
        recs.append((seq, gs, ge, int(rng.integers(0, 4)), int(rng.integers(0, 2)), 0, ge - gs, 2 * (ge - gs), ge - gs, ge - gs))
    rows = util.repeatmasker_tbl_rows(recs, ref_lens, lib_names)
    assert [r[0] for r in rows] == ["DNA/hAT", "LTR/Copia", "Unknown", "total"]
    for cls, n, bases in rows:
        maps = [np.zeros(n_, dtype=bool) for n_ in ref_lens]
        mine = [r for r in recs if cls == "total" or util._lib_name_class(lib_names[r[3]])[1] == cls]
        for r in mine:
            maps[r[0]][r[1]:r[2]] = True
        assert n == len(mine) and bases == sum(int(m.sum()) for m in maps), cls
    assert rows[-1][2] < sum(r[2] for r in rows[:-1])                  # classes overlap on the genome: the total is a union too
    path = tmp_path / "x.tbl"
    util.write_repeatmasker_tbl(recs, ["s1", "s2"], ref_lens, lib_names, str(path))
    txt = open(path).read().split("\n")
    assert txt[0] == "sequences: 2" and txt[1] == "total length: 4200 bp" and txt[-2].split()[0] == "total"
    assert txt[-2].split()[1:3] == [str(rows[-1][1]), str(rows[-1][2])] and txt[-2].split()[3] == "%.2f%%" % (100.0 * rows[-1][2] / 4200)
    assert "byte-compatible" in util.write_repeatmasker_tbl.__doc__


def test_script_parsers_accept_the_reference_s_flags():
    a = _script("annotate_genome").build_parser().parse_args(["-t", "8", "--classified_TE_consensus", "lib.fa", "--tmp_output_dir", "/o", "--annotate", "1",
                                                              "-r", "g.fa", "-w", "/w"])
    assert (a.t, a.classified_TE_consensus, a.tmp_output_dir, a.annotate, a.r, a.work_dir) == ("8", "lib.fa", "/o", "1", "g.fa", "/w")
    a = _script("annotate_genome").build_parser().parse_args(["-t", "8", "--classified_TE_consensus", "lib.fa", "--annotate", "0", "-r", "g.fa"])
    assert a.tmp_output_dir is None and a.work_dir == "/tmp"
    p = _script("pan_annotate_genome").build_parser()
    a = p.parse_args(["--panTE_lib", "p.fa", "--reference", "g.fa", "--genome_name", "g1", "--annotate", "1", "--threads", "4", "--output_dir", "/o",
                      "--work_dir", "/w"])
    assert (a.panTE_lib, a.reference, a.genome_name, a.annotate, a.threads, a.output_dir, a.work_dir) == ("p.fa", "g.fa", "g1", 1, 4, "/o", "/w")
    assert p.parse_args(["--panTE_lib", "p.fa", "--reference", "g.fa", "--genome_name", "g1", "--threads", "4"]).annotate == 1


class _Log:
    def __init__(self):
        self.lines = []
        self.logger = self

    def info(self, msg):
        self.lines.append(msg)


def miniature(tmp_path):
    """a genome of two contigs with whole copies of three entries on both strands, a partial copy (the 20 bases after it differ from the
    entry's, so that it ends where it was cut), and a Helitron-named entry"""
    rng = np.random.default_rng(21)
    lib = {"mini_tir#DNA/hAT": AC.rand(rng, 500), "mini_ltr#LTR/Gypsy": AC.rand(rng, 900), "Chr1-Helitron_2#RC/Helitron": AC.rand(rng, 350)}
    e = list(lib.values())
    c1 = [AC.rand(rng, 700), e[0], AC.rand(rng, 400), AC.revcomp(e[1]), AC.rand(rng, 300), e[0][:300], AC.changed(e[0][300:320]), AC.rand(rng, 480), e[2], AC.rand(rng, 200)]
    c2 = [AC.rand(rng, 150), AC.revcomp(e[0]), AC.rand(rng, 600), e[1], AC.rand(rng, 100)]
    planted = [("mini_tir", "ctg1", 700, 1200), ("mini_ltr", "ctg1", 1600, 2500), ("Chr1-Helitron_2", "ctg1", 3600, 3950), ("mini_tir", "ctg2", 150, 650),
               ("mini_ltr", "ctg2", 1250, 2150)]
    lib_path, ref_path = str(tmp_path / "lib.fa"), str(tmp_path / "genome.fa")
    with open(lib_path, "w") as f:
        for name, s in lib.items():
            f.write(">%s\n%s\n" % (name, AC.text(s)))
    with open(ref_path, "w") as f:
        f.write(">ctg1\n%s\n>ctg2\n%s\n" % (AC.text(*c1), AC.text(*c2)))
    return lib_path, ref_path, planted


def check_annotation_files(out_path, gff_path, tbl_path, n_records):
    """the three files parse and the .out and the .gff carry the same records -> the records as (seq, begin, end, strand, name, qb, qe)"""
    out = [ln.split() for ln in open(out_path).readlines()[3:]]
    gff = [ln.rstrip("\n").split("\t") for ln in open(gff_path) if not ln.startswith("#")]
    assert len(out) == len(gff) == n_records
    a = [(f[4], int(f[5]), int(f[6]), f[8], f[9]) + ((int(f[13]), int(f[12])) if f[8] == "C" else (int(f[11]), int(f[12]))) for f in out]
    b = [(f[0], int(f[3]), int(f[4]), "C" if f[6] == "-" else "+", f[8].split(" ")[1].replace('"', "").split(":")[1], int(f[8].split(" ")[2]),
          int(f[8].split(" ")[3])) for f in gff]
    assert a == b and [f[1] for f in out] == [f[5] for f in gff] and [int(f[14]) for f in out] == list(range(1, n_records + 1))
    tbl = open(tbl_path).read().split("\n")
    assert tbl[-2].split()[0] == "total" and int(tbl[-2].split()[1]) == n_records
    return a


def test_annotate_genome_with_the_twin_writes_the_three_files(tmp_path, monkeypatch):
    lib_path, ref_path, planted = miniature(tmp_path)
    out_dir = tmp_path / "out"
    out_dir.mkdir()
    log = _Log()
    util.annotate_genome(str(out_dir), lib_path, ref_path, "0", 4, log, annot=AT.annotate_array)
    util.annotate_genome(str(out_dir), lib_path, ref_path, None, 4, log, annot=AT.annotate_array)
    assert os.listdir(out_dir) == [] and log.lines == []
    util.annotate_genome(str(out_dir), lib_path, ref_path, "1", 4, log, annot=AT.annotate_array)
    assert sorted(os.listdir(out_dir)) == ["HiTE.gff", "HiTE.out", "HiTE.tbl"]
    assert any("HiTE.cat.gz" in ln for ln in log.lines)
    recs = check_annotation_files(str(out_dir / "HiTE.out"), str(out_dir / "HiTE.gff"), str(out_dir / "HiTE.tbl"), 6)
    assert ("ctg1", 701, 1200, "+", "mini_tir", 1, 500) in recs and ("ctg1", 1601, 2500, "C", "mini_ltr", 1, 900) in recs
    assert ("ctg1", 2801, 3100, "+", "mini_tir", 1, 300) in recs and ("ctg2", 151, 650, "C", "mini_tir", 1, 500) in recs
    # the pan script's stage on the same files: the full-length copies are the planted whole copies
    pan = _script("pan_annotate_genome")
    pan.run_annotation(str(out_dir), 4, lib_path, ref_path, 1, "g1", log, annot=AT.annotate_array)
    assert sorted(os.listdir(out_dir)) == ["g1.full_length.copies", "g1.full_length.gff", "g1.gff", "g1.out", "g1.tbl"]
    check_full_length(str(out_dir), "g1", planted, ref_path)


def check_full_length(out_dir, genome_name, planted, ref_path):
    lines = open(os.path.join(out_dir, genome_name + ".full_length.gff")).readlines()
    assert lines[0] == "##gff-version 3\n" and lines[1].startswith("##date ")
    rows = [ln.rstrip("\n").split("\t") for ln in lines[2:]]
    got = sorted((f[8].split(";")[1][len("name="):], f[0], int(f[3]) - 1, int(f[4])) for f in rows)
    assert got == sorted(planted)                                      # every planted full-length copy and nothing else (the partial copy is not)
    assert [(f[0], int(f[3])) for f in rows] == sorted((f[0], int(f[3])) for f in rows) and all(f[1] == "HiTE" and f[6] == "+" for f in rows)
    assert {f[2] for f in rows} == {"DNA/hAT", "LTR/Gypsy", "RC/Helitron"}
    copies = json.load(open(os.path.join(out_dir, genome_name + ".full_length.copies")))
    _names, contigs = util.read_fasta(ref_path)
    assert sorted((n, k) for n, v in copies.items() for k in v) == sorted((n, "%s:%d-%d" % (c, a, b)) for n, c, a, b in planted)
    assert all(s == contigs[k.split(":")[0]][int(k.split(":")[1].split("-")[0]):int(k.split("-")[-1])] for v in copies.values() for k, s in v.items())
