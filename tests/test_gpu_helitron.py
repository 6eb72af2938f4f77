"""GPU parity of the Helitron candidate scan (hite_amd/csrc/hite_helitron.hip, the in-tree stage where the reference runs
HelitronScanner): HIP == the CPU twin (tests/helitron_twin.py) record for record, field for field and in order, and score for
score at every position of both strands, on the cases of tests/helitron_cases.py; the counts of anchors, heads, tails and pairs
too.  The volume case is held against the scoring code compiled for the host (tests/helitron_host.py, which
tests/test_helitron_cases.py holds against the twin): the Python twin would take minutes there.  Then the capacity and argument
errors of the entry point, and the stage script on a miniature genome with no candidate file."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import helitron_cases as HC
import helitron_host as HH
import helitron_twin as T
from hite_amd import util

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "hite_amd", "scripts", "judge_Helitron_transposons.py")


@pytest.fixture(scope="module")
def ctx():
    import hite_amd

    c = hite_amd.Context(0)
    yield c
    c.close()


def check(ctx, c):
    hp, tp = util.parse_lcvs(c["head"], "head"), util.parse_lcvs(c["tail"], "tail")
    st_gpu, st = {}, {}
    want = T.scan(c["seqs"], c["head"], c["tail"], stats=st, **c["kw"])
    kw = dict(c["kw"])
    got = ctx.helitron_scan(c["seqs"], hp, tp, kw.get("head_threshold", 1), kw.get("tail_threshold", 1), kw["len_range"], stats=st_gpu)
    assert got.dtype == np.int32 and got.shape == (len(want), 6), c["label"]
    assert got.tolist() == [list(r) for r in want], c["label"]
    assert st_gpu == st, c["label"]
    sc = ctx.helitron_scores(c["seqs"], hp, tp)
    assert np.array_equal(sc, T.scores(c["seqs"], c["head"], c["tail"])), c["label"]
    exp = c["expect"]
    if exp["records"] is not None:
        assert [tuple(r) for r in got.tolist()] == exp["records"], c["label"]
    return len(want)


SMALL = HC.small_cases()


@pytest.mark.parametrize("group", ["sequence ends", "gaps", "limits", "bytes", "strands", "scores", "pairing"])
def test_small_cases(ctx, group):
    """sequence length (empty, 1, 2, 5 bases; first and last possible position; one base short; sequence borders), the gap range and
    one beyond it, a gap of 63 and a body of 32, non-ACGT bytes under dots, letters and literals, both strands and a palindrome,
    1 / 2 / 7 patterns on one position with thresholds at and above the score, the pairing rules at len_min and len_max"""
    key = {"sequence ends": ("tiny", "only empty", "body at", "gap range cut", "sequence border", "literal across"),
           "gaps": ("head gap", "tail gap", "two gaps", "no gap"), "limits": ("gap 63", "body 32"),
           "bytes": ("N under", "N in", "lower case"), "strands": ("reverse complement", "palindrome"),
           "scores": ("score ", "a repeated line"),
           "pairing": ("length ", "the nearer", "a tail upstream", "two heads", "order of")}[group]
    mine = [c for c in SMALL if c["label"].startswith(key)]
    assert mine
    for c in mine:
        check(ctx, c)


def test_every_small_case_is_in_a_group():
    keys = ("tiny", "only empty", "body at", "gap range cut", "sequence border", "literal across", "head gap", "tail gap", "two gaps", "no gap", "gap 63",
            "body 32", "N under", "N in", "lower case", "reverse complement", "palindrome", "score ", "a repeated line", "length ", "the nearer",
            "a tail upstream", "two heads", "order of")
    assert all(c["label"].startswith(keys) for c in SMALL)


def test_batch_shapes(ctx):
    """the tool's 304 + 576 patterns (more than a wavefront, no multiple of 64), 65 / 129, one a side, none on a side"""
    n = [check(ctx, c) for c in HC.batch_cases()]
    assert n[0] >= 24 and n[-3:] == [0, 0, 0]
    assert ctx.helitron_scan([], util.parse_lcvs(["TCACG"], "head"), util.parse_lcvs([], "tail")).shape == (0, 6)


def test_volume(ctx, tmp_path):
    """3 000 random sequences of 100 .. 30 000 bases with 40 planted elements, the tool's lists and defaults"""
    head, tail = HC.lcv_lists()
    hp, tp = util.parse_lcvs(head, "head"), util.parse_lcvs(tail, "tail")
    seqs, truth = HC.volume()
    assert len(seqs) == 3000 and min(map(len, seqs)) == 100 and max(map(len, seqs)) == 30000
    st_gpu, st = {}, {}
    got = ctx.helitron_scan(seqs, hp, tp, stats=st_gpu, cap=1 << 10)
    want = HH.scan(HH.build(tmp_path), seqs, hp, tp, stats=st)
    assert len(want) > 1000 and np.array_equal(got, want) and st_gpu == st
    plus = {(int(r[0]), int(r[1])) for r in got if r[3] == 0}
    minus = {(int(r[0]), int(r[2])) for r in got if r[3] == 1}
    for q, s, e, strand in truth:             # a planted head always pairs: with its own tail or with a nearer one
        assert ((q, e) in minus) if strand else ((q, s) in plus)


def _raw(ctx, seqs, head, tail, ht=1, tt=1, lmin=20, lmax=200, cap=64, off=None, n=None, n_head=None, n_tail=None):
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    sb = [s.encode() for s in seqs]
    o = np.zeros(len(sb) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in sb], out=o[1:])
    if off is not None:
        o = np.asarray(off, dtype=np.int64)
    buf = np.frombuffer(b"".join(sb) + b"\0" * 16, dtype=np.uint8)
    out = [np.full(max(cap, 1) + 2, -7, dtype=np.int32) for _ in range(5)]
    strand = np.full(max(cap, 1) + 2, 9, dtype=np.uint8)
    n_out, st = C.c_int64(-1), np.zeros(4, dtype=np.int64)
    rc = ctx.lib.hite_helitron_scan(ctx.h, C.c_int64(len(sb) if n is None else n), p(buf), p(o), C.c_int32(len(head) if n_head is None else n_head), p(head),
                                    C.c_int32(len(tail) if n_tail is None else n_tail), p(tail), C.c_int32(ht), C.c_int32(tt), C.c_int32(lmin),
                                    C.c_int32(lmax), C.c_int64(cap), p(out[0]), p(out[1]), p(out[2]), p(strand), p(out[3]), p(out[4]),
                                    C.byref(n_out), p(st))
    return rc, n_out.value, out, strand


def test_capacity_and_argument_errors(ctx):
    c = [x for x in SMALL if x["label"] == "order of the records"][0]
    seqs = [s.decode() for s in c["seqs"]]
    hp, tp = util.parse_lcvs(c["head"], "head"), util.parse_lcvs(c["tail"], "tail")
    want = c["expect"]["records"]
    rc, n, out, strand = _raw(ctx, seqs, hp, tp, lmin=30, lmax=80, cap=len(want))
    assert (rc, n) == (0, len(want)) and out[1][:n].tolist() == [r[1] for r in want] and strand[:n].tolist() == [r[3] for r in want]
    rc, n, out, strand = _raw(ctx, seqs, hp, tp, lmin=30, lmax=80, cap=len(want) - 1)       # HITE_ECAP with the room; the first cap are written
    assert (rc, n) == (-4, len(want)) and out[2][:n - 1].tolist() == [r[2] for r in want[:-1]]
    assert out[2][n - 1:].tolist() == [-7] * 2 and strand[n - 1:].tolist() == [9] * 2       # ... and nothing behind them (cap + 2 entries)
    rc, n, _o, _s = _raw(ctx, seqs, hp, tp, lmin=30, lmax=80, cap=0)
    assert (rc, n) == (-4, len(want))
    bad = lambda **kw: _raw(ctx, seqs, hp, tp, **kw)[0]  # noqa: E731
    assert bad(n=-1) == -1 and bad(n_head=-1) == -1 and bad(n_tail=-1) == -1 and bad(cap=-1) == -1
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])])
    off[2], off[3] = off[3], off[2] - 1
    assert bad(off=off) == -1                                                                # descending offsets
    assert bad(lmin=81, lmax=80) == -1 and bad(lmin=0) == -1 and bad(ht=0) == -1 and bad(tt=0) == -1
    assert bad(lmin=80, lmax=80) == 0
    for field, value in (("body_len", 0), ("body_len", 33), ("gap_max", 64), ("gap_min", 5), ("care", 1), ("body", 3 << 12)):
        h2 = hp.copy()
        h2[field][0] = value
        assert _raw(ctx, seqs, h2, tp)[0] == -1, field
        t2 = tp.copy()
        t2[field][0] = value
        assert _raw(ctx, seqs, hp, t2)[0] == -1, field
    many = np.repeat(hp, 1025)
    assert _raw(ctx, seqs, many, tp)[0] == -1 and _raw(ctx, seqs, many[:1024], tp, lmin=30, lmax=80, cap=0)[1] == len(want)
    assert _raw(ctx, [], hp, tp)[:2] == (0, 0) and _raw(ctx, ["", ""], hp, tp)[:2] == (0, 0) and _raw(ctx, seqs, hp[:0], tp[:0])[:2] == (0, 0)
    with pytest.raises(Exception):
        ctx.helitron_scan(seqs, hp, tp, len_range=(9, 3))


def _hsdir(tmp_path):
    head, tail = HC.lcv_lists()
    hsdir = tmp_path / "TrainingSet"
    hsdir.mkdir()
    (hsdir / "head.lcvs").write_text("\n".join(head) + "\n")
    (hsdir / "tail.lcvs").write_text("\n".join(tail) + "\n")
    return hsdir


def _run_stage(tmp_path, g, names, seqs, extra, env):
    out = tmp_path / "out"
    out.mkdir(exist_ok=True)
    (out / "genome.fa").write_text("".join(">c%d\n%s\n" % (i, s) for i, s in enumerate(g["contigs"])))
    (out / "longest_repeats_0.flanked.fa").write_text("".join(">%s\n%s\n" % (n, s) for n, s in zip(names, seqs)))
    argv = ["--seqs", str(out / "longest_repeats_0.flanked.fa"), "-r", str(out / "genome.fa"), "-t", "2", "--tmp_output_dir", str(out), "--ref_index", "0",
            "--flanking_len", "50", "--recover", "0", "--debug", "0", "--min_TE_len", "80", "-w", str(tmp_path)] + extra
    return out, subprocess.run([sys.executable, SCRIPT] + argv, capture_output=True, text=True, env=env)


def test_stage_script_scans_its_own_candidates(tmp_path):
    head, tail = HC.lcv_lists()
    hsdir = _hsdir(tmp_path)
    g, names, seqs = HC.stage_input()
    env = {k: v for k, v in os.environ.items() if k != "HITE_HSDIR"}
    assert util.helitron_lcv_dir(None) is None or "HITE_HSDIR" in os.environ          # no TrainingSet beside the package
    out, rc = _run_stage(tmp_path, g, names, seqs, [], env)
    assert rc.returncode == 2 and "no candidate file" in rc.stderr and not (out / "candidate_helitron_0.fa").exists()
    out, rc = _run_stage(tmp_path, g, names, seqs, ["--HSDIR", str(hsdir)], env)
    assert rc.returncode == 0, rc.stderr[-2000:]
    cn, cc = util.read_fasta(str(out / "candidate_helitron_0.fa"))
    want = T.scan(seqs, head, tail)
    assert cn == ["%s_%d_%d_%s" % (names[q], s + 1, e, "-" if st else "+") for q, s, e, st, _h, _t in want]
    for n, (q, s, e, st, _h, _t) in zip(cn, want):
        assert cc[n] == (T.revcomp(seqs[q][s:e]).decode() if st else seqs[q][s:e])
    assert all(cc[n].startswith("TC") and cc[n][-4:-2] == "CT" for n in cn)
    n_fam, hit = HC.stage_recall(g, cn)
    assert n_fam >= 5 and hit >= 0.8 * n_fam, (n_fam, hit)
    assert (out / "candidate_helitron_0.HelitronScanner.fa").exists() and util.read_fasta(str(out / "candidate_helitron_0.fa.cons"))[0]
    assert (out / "confident_helitron_0.fa").exists()


def test_stage_chain_from_the_recorded_argv_without_a_candidate_file(tmp_path):
    """split -> coarse -> Helitron with the argv main.py builds (tests/golden/main_argv.json, which names no candidate file and no
    --HSDIR) and $HITE_HSDIR set: the Helitron stage scans the coarse stage's flanked repeats itself"""
    import json

    with open(os.path.join(ROOT, "tests", "golden", "main_argv.json")) as f:
        cmds = [c for c in json.load(f)[0]["commands"] if "--ref_index" not in c or c[c.index("--ref_index") + 1] == "0"]
    cmds = [c for c in cmds if c[0] in ("split_genome_chunks.py", "coarse_boundary.py", "judge_Helitron_transposons.py")]
    assert [c[0] for c in cmds] == ["split_genome_chunks.py", "coarse_boundary.py", "judge_Helitron_transposons.py"]
    assert "--HSDIR" not in cmds[2] and "--candidates" not in cmds[2]
    g, _names, _seqs = HC.stage_input()
    out, work = tmp_path / "out", tmp_path / "work"
    out.mkdir(); work.mkdir()
    (out / "genome.fa.clean").write_text("".join(">chr%d\n%s\n" % (i + 1, s) for i, s in enumerate(g["contigs"])))
    env = dict(os.environ, HITE_HSDIR=str(_hsdir(tmp_path)))
    for c in cmds:
        argv = [a.replace("{OUT}", str(out)).replace("{WORK}", str(work)) for a in c[1:]]
        rc = subprocess.run([sys.executable, os.path.join(os.path.dirname(SCRIPT), c[0])] + argv, capture_output=True, text=True, env=env)
        assert rc.returncode == 0, (c[0], rc.stderr[-2000:])
    assert not (out / "candidate_helitron_0.cons.fa").exists()
    cn, cc = util.read_fasta(str(out / "candidate_helitron_0.fa"))
    assert cn and all(cc[n].startswith("TC") and cc[n][-4:-2] == "CT" and cc[n][-2] in "AG" and cc[n][-1] in "AG" for n in cn)
    assert (out / "confident_helitron_0.fa").exists()
