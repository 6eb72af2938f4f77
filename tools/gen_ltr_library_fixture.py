#!/usr/bin/env python
"""Writes tests/golden/ltr_library.json.gz: what the REFERENCE's own code of FiLTR's steps 4 to 8 makes of a seeded genome of planted
LTR families (hite_amd/synth.make_ltr_library_genome) and of crafted integer tables -- get_intact_ltr_copies, search_ltr_structure /
is_ltr_has_structure, estimate_insert_time, filter_single_copy_ltr, get_LTR_seq_from_scn (bin/FiLTR-main/src/Util.py) and
assign_label_to_lib (module/Util.py), loaded from the reference tree and run unchanged (the technique of
tools/gen_ltr_scn_fixture.py).  One thing is replaced: get_domain_info, the blastx search inside filter_single_copy_ltr, by a writer
of the recorded tables of two small synthetic protein files.  The copies that go into get_intact_ltr_copies come from the copy
finder's twin and the twin's coverage rule (tests/oracle_lib.find_copies, tests/ltrcopy_twin.cover_ok): the fixture pins the rules
on the copies, not the search (minimap2 is not pinned).  It holds inputs and the reference's outputs, and no program text.  Runs in
the build container only (it needs the reference tree); regenerable byte for byte:
    PYTHONHASHSEED=0 python tools/gen_ltr_library_fixture.py"""
import gzip
import json
import os
import shutil
import sys
import tempfile
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SEED = 20251021
MIU = 1.3e-8
PROTEINS = {"LTRPeps.lib": {"RT_copia": "M" * 200, "INT_gypsy": "K" * 120}, "OtherPeps.lib": {"TPase_hAT": "L" * 150}}


def domain_rows(names):
    """recorded tables: by position among the single-copy elements -- an intact LTR protein (>= 95 % of it), a fragment of one, an intact
    other protein beside an intact LTR protein"""
    ltr, other = [], []
    for k, n in enumerate(names):
        if k % 3 == 0:
            ltr.append((n, "RT_copia", 10, 610, 1, 191))          # 190 / 200 = 0.95: on the bound
        if k % 3 == 1:
            ltr.append((n, "INT_gypsy", 40, 340, 5, 118))         # 113 / 120 < 0.95
        if k % 4 == 3:
            ltr.append((n, "INT_gypsy", 40, 400, 120, 2))         # minus strand: |2 - 120| / 120 >= 0.95
            other.append((n, "TPase_hAT", 700, 1150, 1, 150))
    return {"LTRPeps.lib": ltr, "OtherPeps.lib": other}


def scn_lines_of(std, names):
    return {k: " ".join(str(x) for x in (s + 1, e, e - s, s + 1, s + 100, 100, e - 99, e, 100, "95.00", k, names[c])) for k, (c, s, e) in enumerate(std)}


def main():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ltrcopy_cases as LC
    import ltrcopy_twin as LT
    import oracle_lib as O
    import ref_harness
    from hite_amd import synth

    U = ref_harness.load_filtr_util()
    HU = ref_harness.load_reference_util()
    quiet = lambda *_a, **_k: None  # noqa: E731
    log = types.SimpleNamespace(logger=types.SimpleNamespace(info=quiet, debug=quiet, error=quiet))
    g = synth.make_ltr_library_genome(seed=SEED)
    names = list(g["contigs"])
    out = {"contigs": g["contigs"], "scn": g["scn"], "truth": g["truth"], "miu": MIU, "proteins": PROTEINS}
    work = tempfile.mkdtemp(prefix="ltr_library_fixture_")
    try:
        ref, scn = os.path.join(work, "ref.fa"), os.path.join(work, "in.scn")
        with open(ref, "w") as f:
            for name, seq in g["contigs"].items():
                f.write(">%s\n%s\n" % (name, seq))
        with open(scn, "w") as f:
            f.write(g["scn"])
        _cand, ltr_lines = U.read_scn(scn, log)
        # ---- the interval rules on crafted integers: contigs of the cases' lengths, records that passed the coverage rule
        crafted = []
        for ci, c in enumerate(LC.crafted()):
            cnames = ["ctg%d" % k for k in range(len(c["contig_len"]))]
            cref = os.path.join(work, "crafted%d.fa" % ci)
            with open(cref, "w") as f:
                for n, ln in zip(cnames, c["contig_len"]):
                    f.write(">%s\n%s\n" % (n, "A" * ln))
            covered = [[r[:3] for r in recs if LT.cover_ok(L, r[3], r[1], r[2], 0.985)] for L, recs in zip(c["el_len"], c["records"])]
            copies = {"el%d" % k: [(cnames[r[0]], r[1], r[2], r[2] - r[1] + 1, "+") for r in recs] for k, recs in enumerate(covered) if recs}
            got = U.get_intact_ltr_copies(copies, scn_lines_of(c["std"], cnames), 0.95, cref)
            crafted.append({"label": c["label"], "contig_len": c["contig_len"], "std": [list(t) for t in c["std"]],
                            "covered": [[list(r) for r in recs] for recs in covered],
                            "intact_ltr_copies": [[n, [[cnames.index(x[0]), x[1], x[2]] for x in v]] for n, v in got.items()]})
        out["crafted"] = crafted
        # ---- step 4 on the genome: the finder's twin on the intact sequences of all lines
        contigs = [g["contigs"][n] for n in names]
        left_names, elements, internal = [], [], {}
        l2c = {}
        for k, line in ltr_lines.items():
            p = line.split(" ")
            nm = "%s-%s-%s" % (p[11], p[3], p[4])
            l2c[nm] = k
            left_names.append(nm)
            elements.append(g["contigs"][p[11]][int(p[3]) - 1:int(p[7])])
            internal[nm] = g["contigs"][p[11]][int(p[4]):int(p[6]) - 1]
        tab = O.find_copies(contigs, elements, clips=True)
        ltr_copies = {}
        for nm, el, rows in zip(left_names, elements, tab):
            rows = [(names[r[0]], r[1], r[2], len(el) - (r[5] & 0xffff) - (r[5] >> 16), "-" if r[3] else "+") for r in rows
                    if LT.cover_ok(len(el), r[5], r[1], r[2], 0.985)]
            if rows:
                ltr_copies[nm] = rows
        out["ltr_copies"] = [[n, [list(r) for r in v]] for n, v in ltr_copies.items()]
        intact = U.get_intact_ltr_copies(ltr_copies, ltr_lines, 0.95, ref)
        out["intact_ltr_copies"] = [[n, [list(r) for r in v]] for n, v in intact.items()]
        # ---- the structure search: every line of the genome, and windows with N, short windows, no common k-mer
        out["structure"] = [[n, list(U.is_ltr_has_structure(n, ltr_lines[l2c[n]], g["contigs"][ltr_lines[l2c[n]].split(" ")[11]]))] for n in left_names]
        windows = [("ACGTACGTTGT", "ACAACGTACGT"), ("AAAAAAAACCC", "GGGTTTTTTTT"), ("ACGTNCGTTGT", "ACANCGTTGTA"), ("TGT", "ACAGGTCA"), ("", ""),
                   ("ACGTTGCATGT", "ACATTGCAAGG"), ("NNNNNNNNNNN", "NNNNNNNNNNN"), ("GATTACAGTGT", "ACATTACAGCC"), ("CCGATCGTGTA", "ACAGATCCCGG")]
        out["windows"] = [[l, r, list(U.search_ltr_structure("w", l, r))] for l, r in windows]
        out["insert_time"] = [[i, MIU, U.estimate_insert_time(i, MIU)] for i in (1.0, 0.985, 0.95, 0.9, 0.8123, 0.5)] + \
            [[0.95, 7e-9, U.estimate_insert_time(0.95, 7e-9)]]
        # ---- the single-copy rule, the protein search replaced by recorded tables
        libs = {}
        for lib, prot in PROTEINS.items():
            libs[lib] = os.path.join(work, lib)
            with open(libs[lib], "w") as f:
                for n, s in prot.items():
                    f.write(">%s\n%s\n" % (n, s))
        singles = [n for n in intact if len(intact[n]) <= 1]
        tables = domain_rows(singles)
        out["domain_tables"] = {k: [list(r) for r in v] for k, v in tables.items()}

        def fake_domain_info(cons, lib, output_table, threads, temp_dir):
            with open(output_table, "w") as f:
                f.write("TE_name\tdomain_name\tTE_start\tTE_end\tdomain_start\tdomain_end\n\n")
                for r in tables[os.path.basename(lib)]:
                    f.write("\t".join(str(x) for x in r) + "\n")

        U.get_domain_info = fake_domain_info
        homo, filtered = os.path.join(work, "intact_LTR_homo.txt"), os.path.join(work, "filtered_single_copy_LTRs.txt")
        U.filter_single_copy_ltr(homo, filtered, os.path.join(work, "single_copy_internal.fa"), intact, internal, libs["LTRPeps.lib"],
                                 libs["OtherPeps.lib"], work, 1, ref, l2c, ltr_lines, log, 0)
        out["intact_LTR_homo"], out["filtered_single_copy_LTRs"] = open(homo).read(), open(filtered).read()
        # ---- step 6 on the whole table (+ a line that its neighbour covers, + a dirty element), then the labels
        lines = [ltr_lines[k] for k in sorted(ltr_lines)]
        p = lines[2].split(" ")
        near = " ".join([str(int(p[0]) + 7), p[1], str(int(p[2]) - 7), str(int(p[3]) + 7)] + p[4:])
        six_scn = os.path.join(work, "six.scn")
        out["six_scn"] = "# step 6\n" + "".join(x + "\n" for x in lines[:3] + [near] + lines[3:])
        with open(six_scn, "w") as f:
            f.write(out["six_scn"])
        dirty = {left_names[1]: 1}
        out["dirty_dicts"] = dirty
        six = {k: os.path.join(work, k) for k in ("confident_ltr.terminal.fa", "confident_ltr.internal.fa", "intact_LTR.fa", "intact_LTR.list")}
        U.get_LTR_seq_from_scn(ref, six_scn, six["confident_ltr.terminal.fa"], six["confident_ltr.internal.fa"], six["intact_LTR.fa"], dirty,
                               six["intact_LTR.list"], MIU)
        out["step6"] = {k: open(v).read() for k, v in six.items()}
        labels = {n: ("LTR/Copia", "LTR/Gypsy", "LTR/Unknown")[k % 3] for k, n in enumerate(HU.read_fasta(six["intact_LTR.fa"])[0])}
        out["labels"] = labels
        cut = os.path.join(work, "confident_ltr_cut.fa")
        with open(cut, "w") as f:
            f.write(out["step6"]["confident_ltr.terminal.fa"] + out["step6"]["confident_ltr.internal.fa"])
        out["labelled"] = {}
        for k, path in (("confident_ltr_cut.fa", cut), ("confident_ltr.terminal.fa", six["confident_ltr.terminal.fa"]),
                        ("confident_ltr.internal.fa", six["confident_ltr.internal.fa"])):
            HU.assign_label_to_lib(path, labels)
            out["labelled"][k] = open(path).read()
    finally:
        shutil.rmtree(work)
    path = os.path.join(ROOT, "tests", "golden", "ltr_library.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps(out, separators=(",", ":"), sort_keys=True).encode())
    print("wrote %s: %d lines, %d elements with copies, %d with a matching copy (%d single), %d with a TSD, homo table %s, %d bytes" %
          (path, len(ltr_lines), len(ltr_copies), len(intact), len(singles), sum(1 for _n, r in out["structure"] if r[1]),
           out["intact_LTR_homo"].split(), os.path.getsize(path)))


if __name__ == "__main__":
    main()
