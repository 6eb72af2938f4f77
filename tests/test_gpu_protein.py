"""GPU parity of the translated protein search (hite_amd/csrc/hite_prot.hip, the in-tree stage where the reference runs
`blastx -evalue 1e-20 -outfmt 6`): HIP == the CPU twin (tests/protein_twin.py + tests/protein_twin.c) record for record, field for
field and in order; the counts of seed hits, distinct survivors and tasks too.  Then the host code on top of it
(util.get_domain_info / util.rescue_low_copy with the switch set) with no blastx on PATH."""
import ctypes as C
import os
import tempfile

import numpy as np
import pytest

import protein_cases as PC
import protein_twin as T

pytestmark = pytest.mark.gpu

ALL = 1e9          # an E-value every positive score passes (S_min = 1): the tests of the stages before the threshold


@pytest.fixture(scope="module")
def ctx():
    import hite_amd

    c = hite_amd.Context(0)
    yield c
    c.close()


def check(ctx, queries, proteins, evalue=ALL):
    """HIP == twin; -> (records, twin stats)"""
    lib = ctx.protein_lib(proteins)
    st_gpu, st = {}, {}
    got = ctx.protein_search(queries, lib, evalue=evalue, stats=st_gpu)
    lib.release()
    want = T.search(queries, proteins, evalue=evalue, stats=st)
    assert (st_gpu.get("hits", 0), st_gpu.get("survivors", 0), st_gpu.get("tasks", 0)) == (st["hits"], st["survivors"], st["tasks"])
    assert got.tolist() == [list(r) for r in want]
    return want, st


def test_translation(ctx):
    rng = np.random.default_rng(1)
    seqs = []
    for n in list(range(0, 9)) + [190, 191, 192, 193, 194]:
        s = PC.rand_dna(rng, n)
        seqs += [s, s.lower(), "".join(c if rng.random() > 0.1 else "N" for c in s), "".join(c.lower() if rng.random() < 0.5 else c for c in s)]
    seqs.append("ATGGCCTGANN")
    got = ctx.translate6(seqs)
    assert got == [T.translate6(s) for s in seqs]
    assert got[-1] == ["MA*", "WPX", "GLX", "XQA", "XRP", "SGH"]
    assert ctx.translate6([]) == [] and ctx.translate6(["", "AC"]) == [[""] * 6] * 2


def test_index_and_seeds(ctx):
    rng = np.random.default_rng(2)
    same = PC.rand_protein(rng, 90)
    prots = ["ARN", "ARND", "ARNDC", same, same,
             "wHcMkLLpQ" + PC.rand_protein(rng, 40).lower(),                      # lower case
             "ARNDBZXU*JO" + PC.rand_protein(rng, 30) + "X" + "CQEG",              # non-standard letters are X
             "AAAA" + "ARAR" + "AARA" + "AAAR" + PC.rand_protein(rng, 20) + "WWWWCWCW"]   # one- and two-letter 4-mers are no seeds
    # WHCM two hundred times: a bucket longer than a wavefront
    for _ in range(40):
        prots.append("".join(PC.rand_protein(rng, int(rng.integers(5, 30))) + "WHCM" for _ in range(5)) + PC.rand_protein(rng, 7))
    assert sum(p.count("WHCM") for p in prots) >= 200 and len(prots) <= 64 and max(len(p) for p in prots) <= 600
    queries = [PC.back_translate(rng, "ARND"),                                     # twelve bases == a four-residue protein
               PC.back_translate(rng, "ARNDC"), PC.back_translate(rng, "ARN"),
               PC.back_translate(rng, same),                                       # seeds at the first and at the last residue of the frame
               PC.revcomp(PC.back_translate(rng, same[10:70])),
               PC.rand_dna(rng, 301) + PC.back_translate(rng, "KLWHCMPQ") + PC.rand_dna(rng, 200),
               PC.back_translate(rng, prots[7]), PC.back_translate(rng, prots[6].replace("*", "W")),
               PC.back_translate(rng, prots[10][:80]) + "A" + PC.back_translate(rng, prots[11][-60:]),
               "ACGT" * 30, "N" * 50, ""]
    want, st = check(ctx, queries, prots)
    assert st["hits"] >= 200 + 4 and st["survivors"] > 0
    by_query = {}
    for r in want:
        by_query.setdefault(r[0], []).append(r)
    # (a seed of three distinct letters scores at most W W C H = 39 < 41: the four- and five-residue pairs are seed hits, never survivors)
    assert 0 not in by_query and 1 not in by_query and 2 not in by_query
    assert {r[1] for r in by_query[3][:2]} == {3, 4} and by_query[3][0][3:7] == (1, 270, 1, 90) and by_query[3][0][7:] == by_query[3][1][7:]
    assert by_query[4][0][2] < 0 and by_query[4][0][3] > by_query[4][0][4] and by_query[4][0][5:7] == (11, 70)
    assert 9 not in by_query and 10 not in by_query and 11 not in by_query


def test_ungapped_filter(ctx):
    rng = np.random.default_rng(3)
    # scores 40 and 41 (A R N D C C = 39, S/T = 1), drops of exactly 16 and of 17 (A/R = -1) in both directions, segments cut by the
    # ends of the frame and of the protein
    prots = ["ARNDCCS", "ARNDCCSS",
             "CWHMA" + "A" * 16 + "WWHC", "CWHMA" + "A" * 17 + "WWHC",
             PC.rand_protein(rng, 120)]
    dom = prots[4]
    queries = [PC.back_translate(rng, "ARNDCCT"), PC.back_translate(rng, "ARNDCCTT"),
               PC.back_translate(rng, "CWHMA" + "R" * 16 + "WWHC"), PC.back_translate(rng, "CWHMA" + "R" * 17 + "WWHC"),
               PC.back_translate(rng, dom[40:]) + PC.rand_dna(rng, 90),         # the protein's end inside the frame, the frame's start inside the protein
               PC.rand_dna(rng, 91) + PC.back_translate(rng, dom[:70])]          # the other way round
    want, st = check(ctx, queries, prots)
    surv = {}
    for s in st["survivor_list"]:
        surv.setdefault((s[0] // 6, s[1]), []).append(s)
    assert (0, 0) not in surv and surv[(1, 1)] == [(6, 1, 0, 0, 7)]
    assert (0, 24) in [(s[3], s[4]) for s in surv[(2, 2)]]                       # exactly 16: the segment runs through to the end
    assert (3, 3) not in surv                                                    # 17: both halves stay below 41 (C W H M A = 37, W W H C = 39)
    assert any(s[3] == 0 for s in surv[(4, 4)]) and any(s[3] == 30 and s[4] == 99 for s in surv[(5, 4)])
    assert [r[:2] for r in want if r[0] == 0 and r[1] == 0] == [] and [r[:2] for r in want if r[0] == 1 and r[1] == 1] == [(1, 1)]


def _domain_cases(rng):
    prots = [PC.rand_protein(rng, n) for n in (300, 240, 200, 50, 330, 400, 120)]
    q = []
    fl = lambda n: PC.rand_dna(rng, n)  # noqa: E731
    for div in (0.0, 0.2, 0.4):                                                    # planted domains, both strands
        s = fl(150) + PC.back_translate(rng, PC.diverge(rng, prots[0], div)) + fl(151)
        q += [s, PC.revcomp(s)]
    a, b = prots[1][:120], prots[1][120:]
    for k in (23, 24, 25):                                                         # k residues more in the frame: the lower edge of the band
        q.append(fl(31) + PC.back_translate(rng, a + PC.rand_protein(rng, k) + b) + fl(20))
    a, b = prots[4][:140], prots[4][140:]
    for k in (38, 39, 40):                                                         # k residues of the protein missing in the frame: the upper edge
        q.append(fl(32) + PC.back_translate(rng, a + b[k:]) + fl(20))
    q.append(fl(200) + PC.back_translate(rng, prots[3]) + fl(200))                # a protein shorter than the band
    q.append(PC.back_translate(rng, prots[2]))                                     # the row window clipped at 0 and at L_f
    q.append(PC.back_translate(rng, prots[2][100:]) + fl(100))
    for gap in (129, 128):                                                         # two domains on one diagonal: segments 129 / 128 apart
        mid = PC.diverge(rng, prots[5][100:100 + gap - 1], 1.0)
        q.append(fl(30) + PC.back_translate(rng, prots[5][:100] + mid + prots[5][100 + gap - 1:]) + fl(30))
    bt = PC.back_translate(rng, prots[0])
    q += [fl(60) + bt[:450] + "A" + bt[450:] + fl(60), fl(60) + bt[:450] + bt[451:] + fl(60)]      # +1 / -1 base: two frames
    dm = prots[6]
    q.append(fl(40) + PC.back_translate(rng, dm[:60]) + "TAATGA" + PC.back_translate(rng, dm[62:]) + fl(40))      # stops inside
    q.append(fl(40) + PC.back_translate(rng, dm[:50]) + "N" * 30 + PC.back_translate(rng, dm[60:]) + fl(40))      # an N run inside
    return q, prots


def test_gapped_alignment(ctx):
    rng = np.random.default_rng(4)
    q, prots = _domain_cases(rng)
    assert len(q) <= 64 and max(len(s) for s in q) <= 3000
    want, st = check(ctx, q, prots)
    best = {}
    for r in want:
        best.setdefault(r[0], r)
    for k in range(6):                                                             # the planted domain, whole at 0 % and mostly at 20 / 40 %
        assert best[k][1] == 0 and (best[k][2] > 0) == (k % 2 == 0) and best[k][6] - best[k][5] >= 250
    assert best[0][2:] == (1, 151, 1050, 1, 300, best[0][7], 300, 300) and best[1][3:7] == (len(q[1]) - 150, len(q[1]) - 1049, 1, 300)
    tasks = {}
    for t in st["task_list"]:
        tasks.setdefault((t[0] // 6, t[1]), []).append(t)
    # the halves are more than 16 diagonals apart: two tasks each.  k more residues in the frame: the task of the lower diagonal reaches
    # the other half while k <= 39 (all three; the task of the upper one reaches down while k <= 24); k residues of the protein missing:
    # the task of the lower diagonal reaches up while k <= 39, the other one never reaches down
    for k, joined in ((6, True), (7, True), (8, True), (9, True), (10, True), (11, False)):
        p, lo, hi = (1, 100, 140) if k < 9 else (4, 120, 160 + (38, 39, 40)[k - 9])
        assert len(tasks[(k, p)]) == 2
        across = [r for r in want if r[0] == k and r[1] == p and r[5] <= lo and r[6] >= hi]
        assert bool(across) == joined, k
    assert best[12][1] == 3 and best[12][5:7] == (1, 50)
    assert best[13][3:7] == (1, 600, 1, 200) and best[14][3:7] == (1, 300, 101, 200)
    assert len(tasks[(15, 5)]) == 2 and len(tasks[(16, 5)]) == 1
    for k in (17, 18):
        two = [r for r in want if r[0] == k and r[1] == 0][:2]
        assert len(two) == 2 and two[0][2] != two[1][2] and two[0][2] > 0 and two[1][2] > 0
    assert best[19][1] == 6 and best[19][5:7] == (1, 120) and best[20][1] == 6


def test_threshold(ctx):
    rng = np.random.default_rng(5)
    prots = [PC.rand_protein(rng, 150), PC.rand_protein(rng, 90)]
    q = [PC.rand_dna(rng, 100) + PC.back_translate(rng, PC.diverge(rng, prots[0], 0.3)) + PC.rand_dna(rng, 50),
         PC.rand_dna(rng, 77) + PC.back_translate(rng, prots[1][:25])]
    want, _ = check(ctx, q, prots)
    n_res = sum(len(p) for p in prots)
    for rec in (want[0], [r for r in want if r[0] == 1][0]):
        m, S = len(q[rec[0]]) // 3, rec[7]
        at, above = T.evalue_of(m, n_res, S), T.evalue_of(m, n_res, S + 1)
        assert T.smin(m, n_res, at) == S == ctx.protein_smin(m, n_res, at) and ctx.protein_smin(m, n_res, above) == S + 1
        here, _ = check(ctx, [q[rec[0]]], prots, evalue=at)
        assert (0,) + rec[1:] in here
        gone, _ = check(ctx, [q[rec[0]]], prots, evalue=above)
        assert (0,) + rec[1:] not in gone and len(gone) < len(here)
    # the default threshold
    assert [r[:2] for r in check(ctx, q, prots, evalue=1e-20)[0]] == [(0, 0)]


def test_cap_determinism_and_empty_results(ctx):
    rng = np.random.default_rng(6)
    q, prots = _domain_cases(rng)
    lib_a, lib_b = ctx.protein_lib(prots), ctx.protein_lib(prots)
    first = ctx.protein_search(q, lib_a, evalue=ALL)
    assert len(first) > 8
    assert np.array_equal(first, ctx.protein_search(q, lib_a, evalue=ALL))
    assert np.array_equal(first, ctx.protein_search(q, lib_b, evalue=ALL))
    assert np.array_equal(first, ctx.protein_search(q, lib_a, evalue=ALL, batch_bases=2000, cap=1))     # several batches, each asked twice
    # HITE_ECAP: the first cap records, nothing behind them
    buf, off = ctx._csr(q)
    cap = 5
    out = np.full((10, cap + 3), -7, dtype=np.int32)
    n_out = C.c_int64(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = ctx.lib.hite_protein_search(ctx.h, lib_a.h, C.c_int64(len(q)), p(buf), p(off), C.c_double(ALL), C.c_int64(cap),
                                     *[p(out[k]) for k in range(10)], C.byref(n_out), None)
    assert rc == -4 and n_out.value == len(first)
    assert np.array_equal(out[:, :cap].T, first[:cap]) and (out[:, cap:] == -7).all()
    # valid empty results
    assert ctx.protein_search([], lib_a).shape == (0, 10)
    assert ctx.protein_search(["ACGT" * 50, "", "NNNN"], lib_a, evalue=ALL).shape == (0, 10)
    empty = ctx.protein_lib([])
    assert ctx.protein_search(q[:2], empty, evalue=ALL).shape == (0, 10)
    none = ctx.protein_lib(["", "AR"])
    assert ctx.protein_search(q[:2], none, evalue=ALL).shape == (0, 10)
    # limits of the definition
    from hite_amd import HiteError
    with pytest.raises(HiteError):
        ctx.protein_lib(["A" * 65536])
    with pytest.raises(HiteError):
        ctx.protein_search(["A" * 196606], lib_a)
    for lib in (lib_a, lib_b, empty, none):
        lib.release()


# ---- through the host code: no blastx on PATH ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def low_copy_case(tmp_path_factory):
    T.clib()                      # (built while the compiler is still on PATH)
    rng = np.random.default_rng(7)
    d = tmp_path_factory.mktemp("domains")
    prots = {"dom%d" % k: PC.rand_protein(rng, n) for k, n in enumerate((220, 180, 260, 150))}
    for name in ("TIRPeps.lib", "HelitronPeps.lib", "non_LTR.lib"):
        with open(d / name, "w") as f:
            for n, s in prots.items():
                f.write(">%s some description\n%s\n" % (n, s))
    pl = list(prots.values())
    low, whole = {}, []
    for k in range(4):            # a whole protein at 20 % divergence (its first and last six residues as they are), both strands
        p = pl[k]
        s = PC.rand_dna(rng, 150 + k) + PC.back_translate(rng, p[:6] + PC.diverge(rng, p[6:-6], 0.2) + p[-6:]) + PC.rand_dna(rng, 140)
        low["whole_%d" % k] = s if k % 2 == 0 else PC.revcomp(s)
        whole.append("whole_%d" % k)
        low["part_%d" % k] = PC.rand_dna(rng, 120) + PC.back_translate(rng, p[:int(0.6 * len(p))]) + PC.rand_dna(rng, 130 + k)      # 60 %
        low["none_%d" % k] = PC.rand_dna(rng, 700 + 13 * k)
    return str(d), prots, low, whole


def _twin_rows(util, low, prots, threads):
    """the table blastx_domain_table yields from the twin's -outfmt 6 lines, partition by partition as get_domain_info deals them"""
    pn, n_res = list(prots.keys()), sum(len(s) for s in prots.values())
    rows = []
    for part in util.pet_partitions(list(low.items()), threads):
        if not part:
            continue
        names, seqs = [n for n, _ in part], [s for _, s in part]
        lines = T.outfmt6(T.search(seqs, [prots[n] for n in pn], evalue=1e-20), names, pn, [len(s) for s in seqs], n_res)
        with tempfile.NamedTemporaryFile("w", suffix=".out", delete=False) as f:
            f.write("".join(ln + "\n" for ln in lines))
            path = f.name
        rows.extend(util.blastx_domain_table(path, 100))
        os.unlink(path)
    return rows


@pytest.mark.parametrize("te_type", ["helitron", "non_ltr", "tir"])
def test_domain_recall_through_the_host_code(ctx, low_copy_case, te_type, tmp_path, monkeypatch):
    from hite_amd import util

    libdir, prots, low, whole = low_copy_case
    nothing = tmp_path / "empty_path"
    nothing.mkdir()
    monkeypatch.setenv("PATH", str(nothing))
    monkeypatch.delenv("HITE_DOMAIN_SEARCH", raising=False)
    lib = os.path.join(libdir, util._PROTEIN_LIB[te_type])
    same = lambda names, contigs: {n: contigs[n] for n in names}  # noqa: E731   (no tandem repeats in these sequences)
    if te_type != "tir":
        cons = tmp_path / "low.fa"
        util.store_fasta(low, str(cons))
        for threads in (1, 3):
            table = str(tmp_path / ("table%d" % threads))
            assert util.get_domain_info(str(cons), lib, table, threads, str(tmp_path / ("tmp%d" % threads)), search="gpu", ctx=ctx)
            rows = [tuple(ln.rstrip("\n").split("\t")) for ln in open(table).read().splitlines()[2:]]
            want = _twin_rows(util, low, prots, threads)
            assert rows == [tuple(str(x) for x in r) for r in want] and len(rows) >= len(whole)
            assert sorted(util.intact_domain_names(table, lib)) == sorted(whole)
        # the switch unset: no search, as before
        table = str(tmp_path / "table_off")
        assert not util.get_domain_info(str(cons), lib, table, 1, str(tmp_path / "tmp_off"))
        assert open(table).read().splitlines()[2:] == []
        rescued, rest = util.rescue_low_copy(te_type, low, 1, str(tmp_path / "work"), tandem_masker=same, ctx=ctx, library_dir=libdir,
                                             domain_search="gpu")
        assert rescued == {n: low[n] for n in whole}
        assert list(rest) == [n for n in low if n not in whole]
        # by the environment variable, as the stage scripts get it
        monkeypatch.setenv("HITE_DOMAIN_SEARCH", "gpu")
        assert list(util.rescue_low_copy(te_type, low, 1, str(tmp_path / "work_env"), tandem_masker=same, ctx=ctx, library_dir=libdir)[0]) == list(rescued)
        monkeypatch.delenv("HITE_DOMAIN_SEARCH")
        rescued, rest = util.rescue_low_copy(te_type, low, 1, str(tmp_path / "work_off"), tandem_masker=same, ctx=ctx, library_dir=libdir)
        assert rescued == {} and rest == low
    else:
        with_tir, no_tir = util.remove_no_tirs(low, 1, ctx=ctx)
        assert any(n in no_tir for n in whole)
        rescued, rest = util.rescue_low_copy("tir", low, 1, str(tmp_path / "work"), tandem_masker=same, ctx=ctx, library_dir=libdir,
                                             domain_search="gpu")
        assert set(rescued) == set(with_tir) | set(whole) and all(rescued[n] == low[n] for n in rescued)
        assert list(rest) == [n for n in low if n not in rescued]
        rescued, rest = util.rescue_low_copy("tir", low, 1, str(tmp_path / "work_off"), tandem_masker=same, ctx=ctx, library_dir=libdir)
        assert set(rescued) == set(with_tir)
