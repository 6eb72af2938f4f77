"""CPU-only: the LTR stage script (hite_amd/scripts/judge_LTR_transposons.py) -- the argv main.py builds for it (main.py:673-679)
through the script's own parser, and a run of the whole stage on the genome of planted families with the twins in place of the
device: the scan, the pair search and the copy support through their twins; the flank stage (util.ltr_flank_filter), whose star
alignment exists on the device only, is replaced by a rule on the names and the library de-duplication by a copy, so that what is
checked is the chain of files, the publishing and the labels.  The device runs util.ltr_library in tests/test_gpu_ltr_library.py."""
import importlib.util
import os
import shutil
import sys

import pytest

import ltrcopy_twin as CT
import ltrscan_twin as LT
import pairhsp_twin as PT
from conftest import load_golden

HERE = os.path.dirname(os.path.abspath(__file__))
SCRIPTS = os.path.join(os.path.dirname(HERE), "hite_amd", "scripts")
# 'judge_LTR_transposons.py ' + ' -g ' + reference + ' -t ' + str(threads) + ... as main.py:673-679 joins it, split as a shell splits it
MAIN_ARGV = ["-g", "{OUT}/genome.fa.clean", "-t", "8", "--tmp_output_dir", "{OUT}", "--recover", "0", "--miu", "1.3e-08", "--use_FiLTR", "1",
             "--use_NeuralTE", "1", "--is_wicker", "0", "--is_output_lib", "1", "--debug", "0", "-w", "{WORK}", "--prev_TE", "{OUT}/tmp_lib.fa"]
FILES = ("confident_ltr.terminal.fa", "confident_ltr.internal.fa", "confident_ltr_cut.fa", "intact_LTR.list", "intact_LTR.fa",
         "filtered_single_copy_LTRs.txt", "intact_LTR.fa.classified", "chr_name.map")


@pytest.fixture(scope="module")
def script():
    if SCRIPTS not in sys.path:
        sys.path.insert(0, SCRIPTS)
    spec = importlib.util.spec_from_file_location("dropin_judge_LTR", os.path.join(SCRIPTS, "judge_LTR_transposons.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_reference_argv_parses(script):
    a = script.build_parser().parse_args(MAIN_ARGV)
    assert a.g == "{OUT}/genome.fa.clean" and a.t == 8 and a.tmp_output_dir == "{OUT}" and a.recover == 0 and float(a.miu) == 1.3e-8
    assert (a.use_FiLTR, a.use_NeuralTE, a.is_wicker, a.is_output_lib, a.debug) == (1, 1, "0", 1, 0)
    assert a.work_dir == "{WORK}" and a.prev_TE == "{OUT}/tmp_lib.fa" and a.classified is None
    assert set(script.OUTPUTS) == set(FILES[:6])


def twin_library(contigs_by_path):
    """util.ltr_library with the twins in place of the device stages"""
    from hite_amd import util

    def copy_dedup(path, _work, _threads, _type, _thr, _debug):
        shutil.copy(path, path + ".cons")

    def library(reference, out_dir, **kw):
        names, contigs = util.read_fasta(reference)
        contigs_by_path[reference] = contigs
        support = lambda elements, std, cover, thr: CT.support([contigs[n] for n in names], elements, std, cover, thr)  # noqa: E731
        return util.ltr_library(reference, out_dir, scan=LT.scan_array, hsps=PT.pair_hsps, support=support, dedup=copy_dedup, **kw)
    return library


def flank_rule(terminals, reference, flanking_len=100, max_copy_num=100, ctx=None, cluster=None, frame_vote=None, seconds=None, **_kw):
    """every left terminal is kept but the one that starts first on its chromosome"""
    first = {}
    for n in terminals:
        c, s = n.split("-")[0], int(n.split("-")[1])
        first[c] = min(first.get(c, s), s)
    return {n: (int(n.split("-")[1]) != first[n.split("-")[0]], "low", None) for n in terminals}, {}


def test_stage_with_the_twins(script, tmp_path, monkeypatch, capsys):
    from hite_amd import util

    gold = load_golden("ltr_library")
    out, work = tmp_path / "out", tmp_path / "work"
    out.mkdir()
    contigs = {"scaffold_%s" % n: s for n, s in gold["contigs"].items()}
    util.store_fasta(contigs, str(out / "genome.fa.clean"))
    monkeypatch.setattr(util, "ltr_flank_filter", flank_rule)
    monkeypatch.delenv("HITE_FILTR_DIR", raising=False)
    argv = [x.replace("{OUT}", str(out)).replace("{WORK}", str(work)) for x in MAIN_ARGV]          # (tmp_lib.fa does not exist: nothing to mask)
    seen = {}
    assert script.main(argv, library=twin_library(seen)) == 0
    err = capsys.readouterr().err
    assert "NOT classified" in err and "LTR/Unknown" in err
    for name in FILES:
        assert (out / name).exists() and not (out / (name + ".tmp")).exists(), name
    assert list(work.iterdir()) == []                                   # the scratch directory is gone
    assert (out / "chr_name.map").read_text().splitlines() == ["chr_%d\tscaffold_%s" % (k, n) for k, n in enumerate(gold["contigs"])]
    (ref_path, ref_contigs), = seen.items()
    assert ref_path.endswith("genome.rename.fa.masked") and list(ref_contigs.values()) == list(gold["contigs"].values())
    # the elements: found by the scan, counted by the copy support -- the family of five has copies, the single ones fall to the
    # single-copy rule, which without protein libraries keeps none
    rows = [ln.split("\t") for ln in (out / "intact_LTR.list").read_text().splitlines()]
    assert len(rows) >= 4 and all(len(r) == 13 and r[1] == "pass" and r[11] == "LTR/Unknown" for r in rows)
    assert all(r[2].startswith("motif:") and r[3].startswith("TSD:") and r[6].startswith("IN:") for r in rows)
    names, seqs = util.read_fasta(str(out / "intact_LTR.fa"))
    assert list(dict.fromkeys(r[0] for r in rows)) == names          # (two lines of one element give two rows and one sequence, as in the reference)
    for n in names:
        c, span = n.split(":")
        a, b = (int(x) for x in span.split(".."))
        assert seqs[n] == ref_contigs[c][a - 1:b]
    cnames, cseqs = util.read_fasta(str(out / "intact_LTR.fa.classified"))
    assert cnames == [n + "#LTR/Unknown" for n in names] and list(cseqs.values()) == list(seqs.values())
    reasons = [ln.split("\t") for ln in (out / "filtered_single_copy_LTRs.txt").read_text().splitlines()]
    assert reasons and all("no_intact_protein" in r[1] for r in reasons)
    tn, ts = util.read_fasta(str(out / "confident_ltr.terminal.fa"))
    inn, _ = util.read_fasta(str(out / "confident_ltr.internal.fa"))
    cut, cs = util.read_fasta(str(out / "confident_ltr_cut.fa"))
    assert len(tn) >= len(names) and len(inn) >= 1 and all(n.endswith("#LTR/Unknown") and n.startswith("LTR_") for n in tn + inn + cut)
    assert sorted(cs.values()) == sorted(list(ts.values()) + list(util.read_fasta(str(out / "confident_ltr.internal.fa"))[1].values()))
    # --recover: the files are there, nothing runs
    assert script.main(argv[:7] + ["1"] + argv[8:], library=lambda *a, **k: pytest.fail("ran")) == 0
    # labels from a file
    labelled = str(tmp_path / "labels.fa")
    util.store_fasta({n + "#LTR/" + ("Copia" if k % 2 else "Gypsy"): seqs[n] for k, n in enumerate(names)}, labelled)
    out2 = tmp_path / "out2"
    assert script.main(argv[:5] + [str(out2)] + argv[6:] + ["--classified", labelled], library=twin_library({})) == 0
    rows2 = [ln.split("\t") for ln in (out2 / "intact_LTR.list").read_text().splitlines()]
    assert [r[11] for r in rows2] == ["LTR/" + ("Copia" if names.index(r[0]) % 2 else "Gypsy") for r in rows2] and [r[:11] + r[12:] for r in rows2] == [r[:11] + r[12:] for r in rows]
    assert {n.split("#")[1] for n in util.read_fasta(str(out2 / "confident_ltr_cut.fa"))[0]} == {"LTR/Copia", "LTR/Gypsy"}
    assert (out2 / "intact_LTR.fa.classified").read_text() == open(labelled).read()


def test_the_retriever_branch_is_refused(script, tmp_path, capsys):
    argv = [x.replace("{OUT}", str(tmp_path)).replace("{WORK}", str(tmp_path)) for x in MAIN_ARGV]
    argv[argv.index("--use_FiLTR") + 1] = "0"
    assert script.main(argv) == 2 and "LTR_retriever" in capsys.readouterr().err
    assert list(tmp_path.iterdir()) == []
