"""Host-side mirror of the reference's function interface for the dynamic-boundary path
(/root/reference/module/Util.py).  Same names, argument meaning and file contracts; the
arithmetic runs in libhite_gpu.so through `hite_amd._lib` (no CPU fallback).

Third-party tools the reference shells out to: `minimap2` copy finding is replaced by the build's own minimizer-based
finder (get_full_length_copies_minimap2; `all_copies=` / `copy_finder=` of flank_region_align_v5 override it); `itrsearch`
(run_itrsearch, Util.py:216) is an in-tree GPU stage pinned to the tool's own output; `trf` and `cd-hit-est` are called where the
reference calls them when they are installed (the build's own masker / clustering otherwise); the low-copy recall of TIR
candidates by structure (Util.py:8196-8213: short-TIR signatures + terminal inverted repeats) is reproduced, and so is the
decision of the recall by protein domains (:8215-8276) on a blastx domain table.  `blastx` itself is called when it is installed;
the build's own translated search (protein_search_outfmt6: six-frame translation, 4-mer seeds, banded Gotoh on the GPU; the
definition is in include/hite_gpu.h) takes its place with search="gpu" / domain_search="gpu" or HITE_DOMAIN_SEARCH=gpu.
The clustering that stands in for `cd-hit-est` (remove_redundant_sequences) works on chain coverage alone by default; with
identity="gpu" or HITE_CLUSTER_IDENTITY=gpu its -c / -A rest on the pairwise identity of include/hite_gpu.h (Context.pair_identity).
The flank filter of LTR terminal sequences (ltr_flank_filter: step 3 of the vendored FiLTR, bin/FiLTR-main/src/LTR_filter.py:44-170)
runs its three `cd-hit-est` calls per candidate as batched calls of the build's own clustering of frames (Context.frame_cluster).
"""
import itertools
import json
import math
import os
import re
import shutil
import subprocess
import sys
import time

import numpy as np

from ._lib import Context

_CTX = None
_PACKED = {"path": None, "names": None, "lens": None}


def get_ctx(device=0):
    global _CTX
    if _CTX is None or not getattr(_CTX, "h", None):      # none yet, or closed by its previous owner
        _CTX = Context(device)
    return _CTX


# ---- FASTA (Util.py:1650-1670, 1983-1988) ---------------------------------------------------------
def read_fasta(fasta_path):
    """-> (names in file order, {name: sequence}): the name is the header up to the first blank or tab, the sequence upper-case;
    a record without sequence characters is skipped, text before the first header ignored, a missing file gives empty results"""
    names, seqs = [], {}
    if not os.path.exists(fasta_path):
        return names, seqs
    current = ""
    with open(fasta_path, "r") as handle:
        # runs of header lines / of sequence lines: of several headers in a row only the last can own sequence
        for is_header, run in itertools.groupby(handle, key=lambda ln: ln.startswith(">")):
            if is_header:
                for ln in run:
                    current = ln.strip()[1:].split(" ")[0].split("\t")[0]
                continue
            sequence = "".join(ln.strip().upper() for ln in run)
            if current != "" and sequence != "":
                seqs[current] = sequence
                names.append(current)
            # (a second run of sequence lines cannot follow without a header in between: groupby merges neighbours)
    return names, seqs


def store_fasta(contigs, file_path):
    with open(file_path, "w") as f:
        for name, seq in contigs.items():
            f.write(">" + name + "\n" + seq + "\n")


def rename_fasta(input, output, header="N"):
    """Util.py:7500 -- names become <header>_<i>, a '#class' suffix (text after the last '#') is kept"""
    names, contigs = read_fasta(input)
    with open(output, "w") as out:
        for i, old in enumerate(names):
            _head, sep, cls = str(old).rpartition("#")
            out.write(">%s_%d%s\n%s\n" % (header, i, sep + cls if sep else "", contigs[old]))


def rename_reference(input, output, chr_name_map):
    """Util.py:7517 -- contigs renamed chr_<i>; the map file holds 'new\told' lines"""
    names, contigs = read_fasta(input)
    chr_name_dict = {}
    with open(output, "w") as f_save:
        for ref_index, name in enumerate(names):
            new_name = "chr_" + str(ref_index)
            f_save.write(">" + new_name + "\n" + contigs[name] + "\n")
            chr_name_dict[new_name] = name
    with open(chr_name_map, "w") as f_save:
        for new_name, old in chr_name_dict.items():
            f_save.write(new_name + "\t" + old + "\n")


def lib_add_prefix(HiTE_lib, prefix):
    """Util.py:11559 -- every name gets '<prefix>-' in front, in place"""
    lib_names, lib_contigs = read_fasta(HiTE_lib)
    store_fasta({prefix + "-" + name: lib_contigs[name] for name in lib_names}, HiTE_lib)
    return HiTE_lib


def convertToUpperCase_v1(reference):
    """Util.py:1521 -- the genome FASTA is rewritten in place: names cut at the first blank, sequences upper-case on one line"""
    names, contigs = [], {}
    with open(reference, "r") as f_r:
        name, seq = "", []
        for line in f_r:
            if line.startswith(">"):
                if name != "" and seq:
                    contigs[name] = "".join(seq)
                    names.append(name)
                name, seq = line.strip()[1:].split(" ")[0], []
            else:
                seq.append(line.strip().upper())
        contigs[name] = "".join(seq)
        names.append(name)
    with open(reference, "w") as f_save:
        for name in names:
            f_save.write(">" + name + "\n" + contigs[name] + "\n")
    return reference


def genome_segments(reference, chrom_seg_length):
    """multi_line (Util.py:1801) + the naming of split_genome_chunks.py:41-52 without the temporary file: yields
    ('chr$offset', segment, len of the '>chr\\toffset\\tsegment' text line) in genome order"""
    names, contigs = read_fasta(reference)
    for name in names:
        contig = contigs[name]
        for start in range(0, len(contig), chrom_seg_length):
            seg = contig[start:start + chrom_seg_length]
            yield name + "$" + str(start), seg, len(">" + name + "\t" + str(start) + "\t" + seg)


def split_chromosomes(chromosomes_dict, max_length=200_000_000):
    """Util.py:10252 -- sequences longer than max_length become <name>_part<k> pieces"""
    out = {}
    for chrom, sequence in chromosomes_dict.items():
        if len(sequence) <= max_length:
            out[chrom] = sequence
            continue
        out.update(("%s_part%d" % (chrom, k + 1), sequence[o:o + max_length]) for k, o in enumerate(range(0, len(sequence), max_length)))
    return out


def split_dict_into_blocks(chromosomes_dict, threads, chunk_size):
    """Util.py:10276 -- consecutive sequences are grouped until a block holds total / threads bases: on the prefix sums of the
    lengths, a block that starts at sequence `first` ends at the first sequence where the sum since `first` reaches the target"""
    items = list(split_chromosomes(chromosomes_dict, max_length=chunk_size).items())
    ends = np.cumsum([len(seq) for _name, seq in items], dtype=np.int64)
    target = int(ends[-1]) // threads if len(items) else 0
    blocks, first = [], 0
    while first < len(items):
        before = int(ends[first - 1]) if first else 0
        last = int(np.searchsorted(ends, before + target, side="left"))       # first index with ends[last] - before >= target
        last = max(first, min(last, len(items) - 1))
        blocks.append(dict(items[first:last + 1]))
        first = last + 1
    return blocks


def split_genome_chunks(reference, tmp_output_dir, chrom_seg_length, chunk_size_mb):
    """module/split_genome_chunks.py:27-88: genome.cut{i}.fa (chr$offset segments, a new chunk whenever the FASTA-text bytes
    read reach chunk_size) and ref_chr/ref_block_{i}.fa; returns the chunk paths"""
    chunk_size = int(float(chunk_size_mb) * 1024 * 1024)
    tmp_output_dir = os.path.abspath(tmp_output_dir)
    os.makedirs(tmp_output_dir, exist_ok=True)
    convertToUpperCase_v1(reference)
    cut_references, cur, cur_base_num, ref_index = [], {}, 0, 0
    for seg_name, seg, line_len in genome_segments(reference, int(chrom_seg_length)):
        cur[seg_name] = seg
        cur_base_num += line_len
        if cur_base_num >= chunk_size:
            path = os.path.join(tmp_output_dir, "genome.cut%d.fa" % ref_index)
            store_fasta(cur, path)
            cut_references.append(path)
            cur, cur_base_num, ref_index = {}, 0, ref_index + 1
    if cur:
        path = os.path.join(tmp_output_dir, "genome.cut%d.fa" % ref_index)
        store_fasta(cur, path)
        cut_references.append(path)
    _names, ref_contigs = read_fasta(reference)
    split_ref_dir = os.path.join(tmp_output_dir, "ref_chr")
    shutil.rmtree(split_ref_dir, ignore_errors=True)
    os.makedirs(split_ref_dir)
    for i, block in enumerate(split_dict_into_blocks(ref_contigs, 100, chunk_size)):
        chr_path = os.path.join(split_ref_dir, "ref_block_%d.fa" % i)
        store_fasta(block, chr_path)
        if shutil.which("makeblastdb"):     # only the blastn route of the reference reads these databases
            subprocess.run("makeblastdb -in %s -dbtype nucl > /dev/null 2>&1" % chr_path, shell=True, check=False)
    return cut_references


def file_exist(result_path):
    """Util.py:2831 -- the reference's 'did this stage succeed' test: a FASTA with at least one record, any other file with
    a non-comment non-blank line, a non-empty directory"""
    if os.path.isdir(result_path):
        with os.scandir(result_path) as entries:
            return next(entries, None) is not None
    if not os.path.isfile(result_path) or os.path.getsize(result_path) == 0:
        return False
    if result_path.endswith((".fa", ".fasta")):
        return bool(read_fasta(result_path)[1])
    with open(result_path, "r") as handle:
        return any(ln.strip() != "" and not ln.startswith("#") for ln in handle)


def update_prev_TE(prev_TE, cur_file):
    """Util.py:6378 -- append cur_file (+ newline) to prev_TE under a lock file (several stage scripts share prev_TE)"""
    if not os.path.exists(cur_file):
        print("Warning: %s not found, skipping" % cur_file)
        return
    import fcntl

    with open(prev_TE + ".lock", "w") as lock_f:
        fcntl.flock(lock_f, fcntl.LOCK_EX)
        try:
            with open(prev_TE, "a+") as target_f, open(cur_file, "r") as source_f:
                target_f.write(source_f.read() + "\n")
        finally:
            fcntl.flock(lock_f, fcntl.LOCK_UN)


def set_reference(reference, device=0):
    """pack the genome into HBM once per process (replaces the per-stage read_fasta(reference))"""
    ctx = get_ctx(device)
    if _PACKED["path"] != os.path.abspath(reference):
        names, contigs = read_fasta(reference)
        ctx.genome_pack([contigs[n] for n in names])
        ctx.set_contig_order(names)       # length ties between alignment rows fall to the row NAME (tools/ready_for_MSA.sh)
        ctx.release_copy_index()          # the minimizer index belongs to the genome that was packed before
        _PACKED.update(path=os.path.abspath(reference), names={n: i for i, n in enumerate(names)},
                       lens=[len(contigs[n]) for n in names])
    return ctx


def _read_alignment(align_file):
    names, contigs = read_fasta(align_file)
    if not names:
        return names, None
    rows = [contigs[n] for n in names]
    width = len(rows[0])
    if any(len(r) != width for r in rows):
        raise ValueError("alignment rows differ in length: " + align_file)
    return names, np.frombuffer("".join(rows).encode(), dtype=np.uint8).reshape(len(rows), width).copy()


# ---- a-14 .. a-21 ------------------------------------------------------------------------------------
def remove_sparse_col_in_align_file(align_file):
    """Util.py:10344-10405: writes <align_file>.clean.fa and returns its path"""
    names, m = _read_alignment(align_file)
    clean = get_ctx().sparse_cols([m])[0]
    out = align_file + ".clean.fa"
    with open(out, "w") as f:
        for n, r in zip(names, clean):
            f.write(">" + n + "\n" + r.tobytes().decode() + "\n")
    return out


def _judge(te_type, cur_seq, align_file, plant, result_type):
    if result_type != "cons":
        raise NotImplementedError("only result_type='cons' (the only value the reference's callers pass)")
    names, m = _read_alignment(align_file)
    if m is None:
        return False, "nb", "", 0
    r = get_ctx().judge(te_type, [m], [cur_seq], plant=int(plant))[0]
    if r[1] == "EXC":
        raise RuntimeError("the reference raises on this input (empty candidate / no full-length row / index error)")
    return r[0], r[1], r[2], r[3]


def judge_boundary_v5(cur_seq, align_file, debug, TE_type, plant, result_type):
    """Util.py:9145-9480 (TIR)"""
    return _judge("tir", cur_seq, align_file, plant, result_type)


def judge_boundary_v6(cur_seq, align_file, debug, TE_type, plant, result_type):
    """Util.py:9821-10159 (Helitron)"""
    return _judge("helitron", cur_seq, align_file, plant, result_type)


def judge_boundary_v9(cur_seq, align_file, debug, TE_type, plant, result_type):
    """Util.py:9483-9720 (non-LTR)"""
    return _judge("non_ltr", cur_seq, align_file, plant, result_type)


def TSDsearch_v5(raw_align_seq, cur_boundary_start, cur_boundary_end, plant):
    """Util.py:2460-2492"""
    l, r, _k = get_ctx().tsd_search([raw_align_seq], [cur_boundary_start], [cur_boundary_end], int(plant))[0]
    return l, r


def search_boundary_homo_v3(valid_col_threshold, pos, matrix, row_num, col_num, type, homo_threshold, debug,
                            int_sliding_window_size, out_sliding_window_size):
    """Util.py:8887-9143; `matrix` = list of rows (lists/strings of single characters)"""
    m = np.frombuffer("".join("".join(r) for r in matrix).encode(), dtype=np.uint8).reshape(row_num, col_num).copy()
    b, _ = get_ctx().boundary_search([m], [pos], [type], [homo_threshold], variant=3, win_in=int_sliding_window_size,
                                     win_out=out_sliding_window_size)
    return int(b[0])


def search_boundary_homo_v4(valid_col_threshold, pos, matrix, row_num, col_num, type, homo_threshold, int_homo_threshold,
                            out_homo_threshold, debug, int_sliding_window_size, out_sliding_window_size):
    """Util.py:8556-8824"""
    m = np.frombuffer("".join("".join(r) for r in matrix).encode(), dtype=np.uint8).reshape(row_num, col_num).copy()
    b, v = get_ctx().boundary_search([m], [pos], [type], [homo_threshold], variant=4, int_thr=[int_homo_threshold],
                                     out_thr=[out_homo_threshold], win_in=int_sliding_window_size,
                                     win_out=out_sliding_window_size)
    return bool(v[0]), int(b[0])


# ---- a-6 ---------------------------------------------------------------------------------------------
def _read_matrix(matrix_file, column):
    rows = []
    with open(matrix_file) as f:
        for line in f:
            rows.append(line.replace("\n", "").split("\t")[column])
    return rows


def get_both_ends_frame(query_name, cur_seq, align_file, output_dir, full_length_output_dir, flanking_len, debug, device=0):
    """bin/FiLTR-main/src/Util.py:1401 -- aligned copies of one LTR terminal -> <output_dir>/<query>.matrix
    ('left_frame\\tright_frame' per copy) and <full_length_output_dir>/<query>.matrix; (None, None) without a boundary"""
    align_names, align_contigs = read_fasta(align_file)
    if not align_names:
        return None, None
    res = get_ctx(device).ltr_both_ends([[align_contigs[n] for n in align_names]], [cur_seq], flanking_len)[0]
    if res is None:
        return None, None
    frames, full, _ns, _ne = res
    start_align_file = os.path.join(output_dir, query_name + ".matrix")
    with open(start_align_file, "w") as f_save:
        for left, right in frames:
            f_save.write(left + "\t" + right + "\n")
    full_length_align_file = os.path.join(full_length_output_dir, query_name + ".matrix")
    with open(full_length_align_file, "w") as f_save:
        for row in full:
            f_save.write(row + "\n")
    return start_align_file, full_length_align_file


def judge_left_frame_LTR(matrix_file, flanking_len, sliding_window_size=20):
    """bin/FiLTR-main/src/Util.py:9327: (is_ltr, new_boundary_start) from the left frames of the '.matrix' file"""
    rows = _read_matrix(matrix_file, 0)
    return (True, -1) if len(rows) <= 1 else get_ctx().ltr_frame([rows], flanking_len, sliding_window_size, "left")[0]


def judge_right_frame_LTR(matrix_file, flanking_len, sliding_window_size=20):
    """bin/FiLTR-main/src/Util.py:9175: (is_ltr, new_boundary_end) from the right frames of the '.matrix' file"""
    rows = _read_matrix(matrix_file, 1)
    return (True, -1) if len(rows) <= 1 else get_ctx().ltr_frame([rows], flanking_len, sliding_window_size, "right")[0]


_COMP = {"A": "T", "T": "A", "C": "G", "G": "C"}


def getReverseSequence(sequence):
    """reverse complement, every non-ACGT symbol -> N (Util.py:1635)"""
    return "".join(_COMP.get(b, "N") for b in reversed(sequence))


def get_short_tir_contigs(cur_itr_contigs, plant):
    """terminal-structure shortcuts of Util.py:7297-7334: variants whose first 5 bases equal the reverse complement of
    their last 5 are kept without itrsearch when the TSD length in the name says hAT (8, < 4 kb), Mutator (9-11) or --
    plants, CACTA/CACTG start -- CACTA (3); so are variants framed by CCC ... GGG."""
    keep = {}
    for name, seq in cur_itr_contigs.items():
        tsd_len = len(name.split("-tsd_")[1].split("-")[0]) if "-tsd_" in name else 0
        head5, tail5 = seq[:5], getReverseSequence(seq[len(seq) - 5:])
        head3, tail3 = seq[:3], getReverseSequence(seq[len(seq) - 3:])
        if head5 == tail5:
            if (tsd_len == 8 and len(seq) < 4000) or 9 <= tsd_len <= 11 or \
                    (plant == 1 and tsd_len == 3 and head5 in ("CACTA", "CACTG")):
                keep[name] = seq
        elif head3 == tail3 == "CCC":
            keep[name] = seq
    return keep


def filter_dup_itr_v3(cur_copies_out_contigs, TIR_len_dict):
    """Util.py:2791-2812: of the variants of one query keep the one with the smallest '-distance_' (first wins ties),
    renamed '<query>-tir_<len>-tsd_<seq>'; >= 30 kb is dropped."""
    best, best_d = "", 100000
    for name in cur_copies_out_contigs:
        d = int(name.split("-distance_")[1])
        if d < best_d:
            best, best_d = name, d
    if not best:
        return {}
    query, rest = best.split("-C_")[0], best.split("-C_")[1]
    tsd = rest.split("-tsd_")[1].split("-")[0]
    seq = cur_copies_out_contigs[best]
    return {"%s-tir_%d-tsd_%s" % (query, TIR_len_dict.get(best, 0), tsd): seq} if len(seq) < 30000 else {}


def run_itrsearch(contigs, end_len=40, device=0, ctx=None):
    """run_itrsearch (Util.py:216-224: `tools/itrsearch -i 0.7 -l 7 <fasta>`) on {name: sequence}: the in-tree stage
    (hite_itr_search; defined by oracle/hite_oracle_itr.c, pinned to the tool's own output).  end_len = 40: the records are the
    first 40 + last 40 bases (Util.py:6564, 6577); end_len = 0: whole sequences (remove_no_tirs, Util.py:13907).
    -> (names the tool writes to <input>.itr, in input order; {name: the "Length itr=" of its header})."""
    names = list(contigs.keys())
    res = (ctx or get_ctx(device)).itr_search([contigs[n] for n in names], end_len=end_len, min_identity=0.7, min_len=7)
    found = [n for n, r in zip(names, res) if r[5]]
    return found, {n: int(r[6]) for n, r in zip(names, res) if r[5]}


def tir_variants_with_structure(names, contigs, flanking_len, plant, device=0, ctx=None):
    """the first two thirds of search_confident_tir_batch_v1 (Util.py:6533-6604): k-mer TSD variants on the GPU
    (search_confident_tir_v4, names '<q>-C_<i>-tsd_<kmer>-distance_<d>' in the canonical order (distance, start, end, k)), the
    terminal-structure shortcuts (get_short_tir_contigs), the terminal-inverted-repeat filter for the rest (a variant itrsearch
    does not report is dropped, Util.py:6598-6600)  -> ({variant: sequence} that stay, {variant: TIR length})."""
    ctx = ctx or get_ctx(device)
    names = [n for n in names if "NNNNNNNNNN" not in contigs[n]]
    recs = ctx.tsd_kmer([contigs[n] for n in names], flank=flanking_len, plant=plant)
    variants = {}
    for n, rr in zip(names, recs):
        seq = contigs[n]
        for i, (k, ts, te, d) in enumerate(rr):
            variants["%s-C_%d-tsd_%s-distance_%d" % (n, i, seq[ts - k:ts], d)] = seq[ts:te + 1]
    short = get_short_tir_contigs(variants, plant)
    rest = {n: s for n, s in variants.items() if n not in short}
    tir_len = {}
    _f, lens = run_itrsearch(short, 40, ctx=ctx) if short else ([], {})
    found, lens_rest = run_itrsearch(rest, 40, ctx=ctx) if rest else ([], {})
    kept = {n: rest[n] for n in found}
    tir_len.update(lens_rest)
    tir_len.update(lens)        # (the reference reads the short set's lengths last, Util.py:6593-6596)
    kept.update(short)
    return kept, tir_len


def search_confident_tir_batch_v1(names, contigs, flanking_len, plant, work_dir=None, device=0, ctx=None):
    """search_confident_tir_batch_v1 (Util.py:6533-6628) for one batch: the variants that keep a terminal structure
    (tir_variants_with_structure), then one variant per query (filter_dup_itr_v3: the smallest '-distance_')."""
    kept, tir_len = tir_variants_with_structure(names, contigs, flanking_len, plant, device, ctx)
    groups = {}
    for n, s in kept.items():
        groups.setdefault(n.split("-C_")[0], {})[n] = s
    out = {}
    for q in groups:
        out.update(filter_dup_itr_v3(groups[q], tir_len))
    return out


def remove_no_tirs(tir_contigs, plant, device=0, ctx=None):
    """remove_no_tirs (Util.py:13897-13920) on {name: sequence}: sequences with a short-TIR signature stay, the rest is
    searched whole for a terminal inverted repeat (itrsearch -i 0.7 -l 7)  -> ({with a TIR}, {without}); the first in the
    reference's order (the tool's output order, then the short-TIR set)."""
    short = get_short_tir_contigs(tir_contigs, plant)
    rest = {n: s for n, s in tir_contigs.items() if n not in short}
    found, _lens = run_itrsearch(rest, 0, device, ctx) if rest else ([], {})
    with_tir = {n: rest[n] for n in found}
    with_tir.update(short)
    return with_tir, {n: s for n, s in tir_contigs.items() if n not in with_tir}


def search_polyA_TSD_batch(seqs, flanking_len=50, end_5_window_size=25, device=0):
    """search_polyA_TSD (Util.py:10915) for a batch of flanked repeats -> [(found_TSD, TSD_seq, non_ltr_seq)]"""
    res = get_ctx(device).nonltr_prep(seqs, flanking_len, end_5_window_size)
    out = []
    for s, (found, direct, ts, tn, lo, hi) in zip(seqs, res):
        nl = s[lo:hi] if direct else ""
        if direct == 2:
            nl = getReverseSequence(nl)
        out.append((bool(found), s[ts:ts + tn] if found else "", nl))
    return out


def get_candidate_non_LTR(longest_repeats_flanked_path, flanking_len=50, device=0):
    """get_candidate_non_LTR (Util.py:11009-11045): flanked repeats of 100-700 bp (SINE) / 700-8000 bp (LINE) with a polyA/T
    or tandem tail and a TSD -> ({name\tTSD:seq: element}, {...}); the element must fall into the same length class."""
    names, contigs = read_fasta(longest_repeats_flanked_path)
    sine = [n for n in names if 100 <= len(contigs[n]) - 2 * flanking_len <= 700]
    line = [n for n in names if 700 < len(contigs[n]) - 2 * flanking_len <= 8000]
    res = search_polyA_TSD_batch([contigs[n] for n in sine + line], flanking_len, 25, device)
    cand_sine, cand_line = {}, {}
    for i, n in enumerate(sine + line):
        found, tsd, seq = res[i]
        if not found:
            continue
        if i < len(sine) and 100 <= len(seq) <= 700:
            cand_sine[n + "\tTSD:" + tsd] = seq
        elif i >= len(sine) and 700 < len(seq) <= 8000:
            cand_line[n + "\tTSD:" + tsd] = seq
    return cand_sine, cand_line


def get_query_copies(cur_segments, query_contigs, subject_path, query_coverage, subject_coverage, query_fixed_extend_base_threshold=200,
                     subject_fixed_extend_base_threshold=200, max_copy_num=100, device=0, ctx=None):
    """Util.py:6828 -- cur_segments = [(query_name, {subject_name: [(q_start, q_end, s_start, s_end, identity)]})] ->
    {query_name: [(subject_name, start, end, chain_len, '+'/'-')]}.  One device call for all queries."""
    subject_contigs = read_fasta(subject_path)[1] if subject_coverage > 0 else {}
    qnames, snames, sidx = [], [], {}
    qid, sid, qs, qe, ss, se, ident = [], [], [], [], [], [], []
    for query_name, subject_dict in cur_segments:
        q = len(qnames)
        qnames.append(query_name)
        for subject_name, subject_pos in subject_dict.items():
            s = sidx.setdefault(subject_name, len(snames))
            if s == len(snames):
                snames.append(subject_name)
            for (a, b, c, d, idt) in subject_pos:
                qid.append(q); sid.append(s); qs.append(a); qe.append(b); ss.append(c); se.append(d); ident.append(idt)
    all_copies = {}
    if not qnames:
        return all_copies
    qlen = [len(query_contigs[name]) for name in qnames]
    slen = [len(subject_contigs[name]) for name in snames] if subject_coverage > 0 else None
    res = (ctx or get_ctx(device)).query_copies(qid, sid, qs, qe, ss, se, ident, qlen, slen, ns=max(1, len(snames)), qcov=query_coverage,
                                       scov=subject_coverage, qthr=query_fixed_extend_base_threshold,
                                       sthr=subject_fixed_extend_base_threshold, max_copy=max_copy_num)
    for q, name in enumerate(qnames):
        all_copies[name] = [(snames[c[0]], c[1], c[2], c[3], c[4]) for c in res[q]]
    return all_copies


def get_copies_v1(blastnResults_path, query_path, subject_path, query_coverage=0.95, subject_coverage=0, device=0, ctx=None):
    """Util.py:7032 -- blast6 table -> {query: copies}; lines with query == subject name are skipped"""
    query_records = {}
    with open(blastnResults_path) as f_r:
        for line in f_r:
            parts = line.split("\t")
            if len(parts) < 10 or parts[0] == parts[1]:
                continue
            query_records.setdefault(parts[0], {}).setdefault(parts[1], []).append(
                (int(parts[6]), int(parts[7]), int(parts[8]), int(parts[9]), float(parts[2])))
    _names, query_contigs = read_fasta(query_path)
    return get_query_copies(list(query_records.items()), query_contigs, subject_path, query_coverage, subject_coverage, device=device, ctx=ctx)


def _chain_all_by_name(query_records, gap_of, ctx):
    """query_records: {query: {subject: [(q_start, q_end, s_start, s_end), ...]}} in the reference's insertion order;
    gap_of(query) -> its skip_gap (real).  -> {query: [(q_start, q_end, length, s_start, s_end, |s span|, subject, extend_num)]}:
    the reference's longest_queries tuples, per query, in its order (hite_chain_all)"""
    import math

    qnames = list(query_records.keys())
    snames, sidx = [], {}
    qid, sid, qs, qe, ss, se = [], [], [], [], [], []
    for qi, q in enumerate(qnames):
        for sname, frags in query_records[q].items():
            si = sidx.setdefault(sname, len(sidx))
            if si == len(snames):
                snames.append(sname)
            for f in frags:
                qid.append(qi); sid.append(si); qs.append(f[0]); qe.append(f[1]); ss.append(f[2]); se.append(f[3])
    out = {q: [] for q in qnames}
    if not qid:
        return out
    # an integer distance is below the real skip_gap exactly when it is below its ceiling
    gaps = [int(math.ceil(gap_of(q))) for q in qnames]
    chains = ctx.chain_all(qid, sid, qs, qe, ss, se, len(qnames), len(snames), gaps)
    for q, lst in zip(qnames, chains):
        for (si, a, b, c, d, nx) in lst:
            out[q].append((a, b, (b - a) if nx else abs(b - a), c, d, abs(d - c), snames[si], nx))
    return out


def FMEA(blastn2Results_path, fixed_extend_base_threshold, device=0, ctx=None):
    """FMEA (Util.py:10452-10645), same arguments: blast6 table -> {query_name: [(query_name, q_start - 1, q_end, subject_name,
    s_start - 1, s_end), ...]} -- every chain of get_longest_repeats_v4's chaining core with a fixed skip_gap, no
    de-duplication (deredundant_for_LTR, Util.py:10750).  A zero-length HSP raises ZeroDivisionError (the reference divides
    by the fragment lengths, :10550-10554, wherever such a fragment meets another one; here: always)."""
    query_records = {}
    with open(blastn2Results_path) as f_r:
        for line in f_r:
            parts = line.split("\t")
            query_name, subject_name = parts[0], parts[1]
            float(parts[2]); int(parts[3])                     # (identity, alignment length: parsed, unused -- a malformed line raises as in the reference)
            q_start, q_end, s_start, s_end = int(parts[6]), int(parts[7]), int(parts[8]), int(parts[9])
            if query_name == subject_name and q_start == s_start and q_end == s_end:
                continue
            if q_start == q_end or s_start == s_end:
                raise ZeroDivisionError("zero-length HSP")
            query_records.setdefault(query_name, {}).setdefault(subject_name, []).append((q_start, q_end, s_start, s_end))
    if ctx is None:
        ctx = get_ctx(device)
    chains = _chain_all_by_name(query_records, lambda _q: fixed_extend_base_threshold, ctx)
    return {q: [(q, r[0] - 1, r[1], r[6], r[3] - 1, r[4]) for r in lst] for q, lst in chains.items()}


def get_full_length_copies_from_blastn_v1(TE_lib, reference, blastn_out, tmp_output_dir, threads, divergence_threshold,
                                          full_length_threshold, search_struct, tools_dir, device=0, ctx=None):
    """get_full_length_copies_from_blastn_v1 (Util.py:5907-6135), same arguments: blast6 table of a TE library against a genome
    -> ({query: {'chr:start-end': sequence | '1'}}, the same with flanks): the chains (skip_gap = len(query) * threshold) that
    cover >= threshold of their query; names lose their '#class' suffix; with search_struct the sequences (flank 5 for
    'Helitron' names, else 50) come from `reference`, else '1' as in the reference."""
    ref_names, ref_contigs = read_fasta(reference) if search_struct else ([], {})
    query_names, query_contigs = read_fasta(TE_lib)
    query_contigs = {name.split("#")[0]: query_contigs[name] for name in query_names}
    query_records = {}
    with open(blastn_out) as f_r:
        for line in f_r:
            if line.startswith("#"):
                continue
            info_parts = line.split("\t")
            query_name = info_parts[0].split("#")[0]
            query_records.setdefault(query_name, {}).setdefault(info_parts[1], []).append(
                (int(info_parts[6]), int(info_parts[7]), int(info_parts[8]), int(info_parts[9])))
    known = {q: v for q, v in query_records.items() if q in query_contigs}       # (`continue` at :5943: no entry in the results)
    if ctx is None:
        ctx = get_ctx(device)
    chains = _chain_all_by_name(known, lambda q: len(query_contigs[q]) * full_length_threshold, ctx)
    full_length_copies, flank_full_length_copies = {}, {}
    for query_name in query_records.keys():
        if query_name not in query_contigs:
            continue
        query_len = len(query_contigs[query_name])
        flanking_len = 5 if "Helitron" in str(query_name) else 50
        query_copies, flank_query_copies = {}, {}
        for repeat in chains[query_name]:
            if repeat[2] < full_length_threshold * query_len:
                continue
            subject_name = repeat[6]
            if repeat[3] > repeat[4]:
                start, end = repeat[4] - 1, repeat[3]
            else:
                start, end = repeat[3] - 1, repeat[4]
            subject_pos = subject_name + ":" + str(start) + "-" + str(end)
            if search_struct:
                subject_seq = ref_contigs[subject_name][start:end]
                flank_subject_seq = ref_contigs[subject_name][start - flanking_len:end + flanking_len]
            else:
                subject_seq = flank_subject_seq = "1"
            if float(repeat[2]) / query_len >= full_length_threshold:
                query_copies[subject_pos] = subject_seq
                flank_query_copies[subject_pos] = flank_subject_seq
        full_length_copies[query_name] = query_copies
        flank_full_length_copies[query_name] = flank_query_copies
    return full_length_copies, flank_full_length_copies


def generate_full_length_out_v1(BlastnOut, TE_lib, reference, tmp_output_dir, tools_dir, full_length_threshold, category, debug=0,
                                device=0, ctx=None):
    """generate_full_length_out_v1 (Util.py:6288-6316), same arguments: the full-length copies of every library sequence as
    pickled sets of (query_name, chr_name, chr_start, chr_end) (1-based, inclusive), one file per batch of 500 queries --
    what mask_genome_intactTE (:6406-6417) reads.  category 'Total' keeps every line of the table, another value those
    whose query class (after '#') contains it (filter_out_by_category :5014).  The structure search of the reference's
    get_structure_info_v1 is switched off in this call there as well (search_struct = False)."""
    import pickle

    os.makedirs(tmp_output_dir, exist_ok=True)
    filter_tmp_out = os.path.join(tmp_output_dir, "tmp.out")
    shutil.copy(BlastnOut, filter_tmp_out)
    if category != "Total":
        kept = [line for line in open(filter_tmp_out) if category in line.split("\t")[0].split("#")[1]]
        filter_tmp_out = os.path.join(tmp_output_dir, "tmp.filter.out")
        with open(filter_tmp_out, "w") as f_save:
            f_save.writelines(kept)
    if os.path.exists(BlastnOut) and debug != 1:
        os.remove(BlastnOut)
    full_length_copies, _flank = get_full_length_copies_from_blastn_v1(TE_lib, reference, filter_tmp_out, tmp_output_dir, 1, 20,
                                                                       full_length_threshold, False, tools_dir, device=device, ctx=ctx)
    if os.path.exists(filter_tmp_out) and debug != 1:
        os.remove(filter_tmp_out)
    cluster_dir = os.path.join(tmp_output_dir, "cluster")
    shutil.rmtree(cluster_dir, ignore_errors=True)
    os.makedirs(cluster_dir)
    all_query_names = list(full_length_copies.keys())
    output_files = []
    for batch_start in range(0, len(all_query_names), 500):
        lines = set()
        for query_name in all_query_names[batch_start:batch_start + 500]:
            for chr_pos in full_length_copies[query_name].keys():
                chr_name, span = chr_pos.split(":")[0], chr_pos.split(":")[1].split("-")
                lines.add((str(query_name), chr_name, int(span[0]) + 1, int(span[1])))
        output_file = os.path.join(cluster_dir, "result_%d.pkl" % batch_start)
        with open(output_file, "wb") as f:
            pickle.dump(lines, f)
        output_files.append(output_file)
    return output_files


def multiple_alignment_blast_and_get_copies_v1(repeats_path, align_fn=None, device=0, ctx=None):
    """multiple_alignment_blast_and_get_copies_v1 (Util.py:7179-7210), same argument (query FASTA, directory of per-chromosome
    '.fa' databases, scratch blast6 path): the chromosomes are searched one after the other (os.listdir order), the copies of
    every query accumulate (get_copies_v1), a query that has reached 100 copies leaves the query file.  align_fn(chr_path,
    query_path, out_path) writes the blast6 table of one chromosome: by default `blastn -evalue 1e-20 -outfmt 6` as in the
    reference when it is installed (it is external), else the build's copy finder, one line per copy."""
    split_repeats_path, split_ref_dir, blastn2Results_path = repeats_path[0], repeats_path[1], repeats_path[2]
    if os.path.exists(blastn2Results_path):
        os.remove(blastn2Results_path)
    if align_fn is None:
        align_fn = _blastn_one_chromosome if shutil.which("blastn") else (lambda c, q, o: _copies_as_blast6(c, q, o, device))
    all_copies = {}
    repeat_names, repeat_contigs = read_fasta(split_repeats_path)
    remain_contigs = repeat_contigs
    for chr_name in os.listdir(split_ref_dir):
        if len(remain_contigs) > 0:
            if not str(chr_name).endswith(".fa"):
                continue
            align_fn(split_ref_dir + "/" + chr_name, split_repeats_path, blastn2Results_path)
            cur_all_copies = get_copies_v1(blastn2Results_path, split_repeats_path, "", device=device, ctx=ctx)
            for query_name in cur_all_copies.keys():
                update_copy_list = all_copies.get(query_name, []) + cur_all_copies[query_name]
                all_copies[query_name] = update_copy_list
                if len(update_copy_list) >= 100:
                    del repeat_contigs[query_name]
            remain_contigs = repeat_contigs
            store_fasta(remain_contigs, split_repeats_path)
    return all_copies


def _blastn_one_chromosome(chr_path, query_path, out_path):
    subprocess.run("blastn -db %s -num_threads 1 -query %s -evalue 1e-20 -outfmt 6 > %s" % (chr_path, query_path, out_path), shell=True, check=False)


def _copies_as_blast6(chr_path, query_path, out_path, device=0):
    """the build's stand-in for one blastn run: the copies hite_find_copies reports for the queries in the sequences of
    chr_path, one blast6 line per copy (the whole query against the copy's interval)"""
    names, contigs = read_fasta(chr_path)
    qnames, queries = read_fasta(query_path)
    ctx = get_ctx(device)
    ctx.genome_pack([contigs[n].upper() for n in names])
    ctx.release_copy_index()
    _PACKED["path"] = None
    # (the index of this chunk serves this one query set -- the caller masks the chunk next: built for these queries only)
    tab = ctx.find_copies([queries[q].upper() for q in qnames], restricted=True) if qnames and names else []
    with open(out_path, "w") as f:
        for q, copies in zip(qnames, tab):
            L = len(queries[q])
            for (c, s1, e1, minus, _anch) in copies:
                a, b = (e1, s1) if minus else (s1, e1)
                f.write("%s\t%s\t%.3f\t%d\t0\t0\t1\t%d\t%d\t%d\t1e-50\t%.1f\n" % (q, names[c], 95.0, L, L, a, b, 2.0 * L))


def lib_longest_repeats(blastnResults_path, redundant_ltr, coverage_threshold, chunk_size=5_000_000, device=0):
    """process_blast_results_in_chunks + FMEA_new1_parallel_large (Util.py:12146, 12006) in one device call ->
    [{query_name: [(query_name, q_start-1, q_end, subject_name, s_start-1, s_end)]}] one dict per chunk, in chunk order"""
    names, contigs = read_fasta(redundant_ltr)
    idx = {name: i for i, name in enumerate(names)}
    qid, sid, qs, qe, ss, se = [], [], [], [], [], []
    with open(blastnResults_path) as f_r:
        for line in f_r:
            parts = line.rstrip("\n").split("\t")
            qid.append(idx[parts[0]]); sid.append(idx[parts[1]])
            qs.append(int(parts[6])); qe.append(int(parts[7])); ss.append(int(parts[8])); se.append(int(parts[9]))
    lens = [len(contigs[name]) for name in names]
    recs = get_ctx(device).lib_chain(qid, sid, qs, qe, ss, se, lens, coverage_threshold, chunk_size)
    chunks = []
    for (ch, q, a, b, s, c, d) in recs:
        while len(chunks) <= ch:
            chunks.append({})
        chunks[ch].setdefault(names[q], []).append((names[q], a, b, names[s], c, d))
    return chunks


def cluster_sequences_from_chunks(longest_repeats_chunks, contigs, coverage_threshold, device=0):
    """Util.py:12067 -- chunks as lib_longest_repeats returns them (the reference reads the same dicts from JSON files) ->
    list of clusters; each cluster is a list (query first) where the reference builds a set"""
    names = list(contigs.keys())
    idx = {name: i for i, name in enumerate(names)}
    recs = []
    for ch, chunk in enumerate(longest_repeats_chunks):
        for query_name, lst in chunk.items():
            for r in lst:
                recs.append((ch, idx[query_name], r[1], r[2], idx[r[3]], r[4], r[5]))
    lens = [len(contigs[name]) for name in names]
    return [[names[i] for i in cl] for cl in get_ctx(device).lib_cluster(recs, lens, coverage_threshold)]


def cons_from_mafft_v1(align_file, device=0):
    """Util.py:12515 -- strict-majority consensus of an aligned FASTA (None for an empty file)"""
    align_names, align_contigs = read_fasta(align_file)
    if len(align_names) <= 0:
        return None
    return get_ctx(device).msa_consensus([[align_contigs[name] for name in align_names]])[0]


def split_internal_out(merge_te_file, output_dir):
    """Util.py:14577 -- LTR internal sequences ('-int#' in the name) and the rest of a merged library go to two files"""
    names, contigs = read_fasta(merge_te_file)
    other_path, internal_path = os.path.join(output_dir, "merged_other.fa"), os.path.join(output_dir, "merged_internal.fa")
    store_fasta({n: contigs[n] for n in names if "-int#" not in n}, other_path)
    store_fasta({n: contigs[n] for n in names if "-int#" in n}, internal_path)
    return other_path, internal_path


def read_Ninja_clusters(cluster_file):
    """Util.py:12500 -- '<cluster id>\t<sequence name>' per line -> {cluster id: [names in file order]}"""
    clusters = {}
    with open(cluster_file) as f_r:
        for line in f_r:
            parts = line.rstrip("\n").split("\t")
            if len(parts) < 2:
                continue
            clusters.setdefault(int(parts[0]), []).append(parts[1])
    return clusters


CLUSTER_CLEAN_THRESHOLD = 10000   # "mafft cannot take too many rows": clusters are kept within this size (Util.py:12254)
NINJA_CUTOFF = 0.2        # generate_cons_v1 runs `Ninja --cluster_cutoff 0.2` (Util.py:12470)
STAR_MAX_LEN = 32767      # longest window the star aligner takes (include/hite_gpu.h)
SEED_MAX_SEGMENTS = 65000  # sequences per all-vs-all call (the seeding stage addresses < 65535 segments)


def ninja_stand_in(rows):
    """The build's stand-in for Ninja's re-clustering of an aligned cluster (Util.py:12468-12474; Ninja is an external tool,
    absent: PARITY UNPINNED).  Leader clustering on the aligned rows: a row joins the first earlier leader it differs from
    in <= 20 % of the columns where either has a base (a base against a gap is a difference; Ninja cuts its
    neighbour-joining tree at distance 0.2), else it becomes a leader.  rows: 2-D uint8 alignment -> list of lists of row indices (sub-clusters in order of their leaders)."""
    rows = np.asarray(rows)
    R, C = rows.shape if rows.ndim == 2 else (0, 0)
    base = rows != 45
    lead_rows = np.empty((0, C), dtype=rows.dtype)     # the leaders' rows, grown in blocks: one vectorised compare per row
    lead_base = np.empty((0, C), dtype=bool)
    n_lead, members = 0, []
    for r in range(R):
        k = -1
        if n_lead:
            # a base against a gap counts like a base against another base (the star alignment threads a short unrelated
            # member through the centre with gaps wherever that makes bases agree: its aligned bases alone look similar)
            either = lead_base[:n_lead] | base[r]
            n = either.sum(axis=1)
            diff = ((lead_rows[:n_lead] != rows[r]) & either).sum(axis=1)
            ok = np.nonzero((n > 0) & (diff <= NINJA_CUTOFF * n))[0]
            if len(ok):
                k = int(ok[0])
        if k >= 0:
            members[k].append(r)
            continue
        if n_lead == len(lead_rows):
            grow = max(16, n_lead)
            lead_rows = np.concatenate([lead_rows, np.empty((grow, C), dtype=rows.dtype)])
            lead_base = np.concatenate([lead_base, np.zeros((grow, C), dtype=bool)])
        lead_rows[n_lead], lead_base[n_lead] = rows[r], base[r]
        n_lead += 1
        members.append([r])
    return members


def _star_align_clusters(ctx, clusters):
    """clusters: list of lists of (name, sequence).  Every cluster is aligned as a star around its LONGEST member (ties: the
    first), rows returned in the cluster's own order -- the stand-in for `mafft --preservecase` (Util.py:12464, 12490; mafft
    compares case-insensitively: sequences are upper-cased first).  -> per cluster (rows: {name: aligned row}, dropped: [names
    the aligner could not place (shorter than half the centre, or an insertion / deletion beyond its widest band)])."""
    groups, orders = [], []
    for cl in clusters:
        seqs = [sq.upper() for _n, sq in cl]
        centre = max(range(len(seqs)), key=lambda i: (len(seqs[i]), -i))
        order = [centre] + [i for i in range(len(seqs)) if i != centre]
        orders.append(order)
        groups.append([seqs[i] for i in order])
    aligned, info = ctx.star_msa(groups, info=True) if groups else ([], [])
    out = []
    for cl, order, m, inf in zip(clusters, orders, aligned, info):
        rows, dropped = {}, []
        if m is None:
            out.append(({}, [n for n, _s in cl]))
            continue
        k = 0
        by_member = {}
        for pos, i in enumerate(order):
            if pos == 0 or int(inf[pos][2]) == 0:
                by_member[i] = bytes(m[k]).decode()
                k += 1
            else:
                dropped.append(cl[i][0])
        for i in range(len(cl)):               # back to the cluster's own order
            if i in by_member:
                rows[cl[i][0]] = by_member[i]
        out.append((rows, dropped))
    return out


def _subcluster_on(subcluster):
    """the switch of the sub-clustering route of _generate_cons_batch: the argument, then $HITE_SUBCLUSTER; "gpu" is on"""
    mode = subcluster if subcluster is not None else os.environ.get("HITE_SUBCLUSTER")
    return mode == "gpu"


def _generate_cons_batch(ctx, clusters, ninja=None, subcluster=None, seconds=None):
    """generate_cons_v1 (Util.py:12457-12498) for a batch of clusters, each a list of (name, sequence) in file order:
    alignment -> sub-clusters (Ninja in the reference, ninja_stand_in here; `ninja` = per cluster {id: [names]} overrides it,
    which is how the goldens pin everything around the external tool) -> alignment of every sub-cluster -> strict-majority
    consensus (cons_from_mafft_v1) named after the sub-cluster's LAST member.  A cluster that yields no consensus returns
    its sequences unchanged; members the aligner dropped pass unchanged as well.  -> per cluster {name: sequence}.
    subcluster="gpu" (or HITE_SUBCLUSTER=gpu when the argument is None; anything else is off) takes the sub-clusters of ALL first
    alignments from one Context.msa_subcluster call (hite_msa_subcluster: the same leader clustering on the device) instead of
    ninja_stand_in cluster by cluster; the result is the same.  seconds: a dict that receives the wall seconds of the steps
    (align_first, subcluster, align_second, consensus)."""
    clock = time.perf_counter
    t0 = clock()
    need_first = [ci for ci in range(len(clusters)) if ninja is None or ninja[ci] is None]
    first = dict(zip(need_first, _star_align_clusters(ctx, [clusters[ci] for ci in need_first])))
    t1 = clock()
    kept_names, mats = {}, {}
    for ci in need_first:
        rows = first[ci][0]
        names = [n for n, _s in clusters[ci] if n in rows]
        if names:
            kept_names[ci] = names
            mats[ci] = np.frombuffer("".join(rows[n] for n in names).encode(), dtype=np.uint8).reshape(len(names), -1)
    order = sorted(mats)
    if _subcluster_on(subcluster):
        groups = dict(zip(order, ctx.msa_subcluster([mats[ci] for ci in order], NINJA_CUTOFF))) if order else {}
    else:
        groups = {ci: ninja_stand_in(mats[ci]) for ci in order}
    t2 = clock()
    subs, owner = [], []
    passed = [dict() for _ in clusters]
    for ci, cl in enumerate(clusters):
        seq_of = dict(cl)
        if ci in first:
            for n in first[ci][1]:           # not placed in the cluster's alignment: passes unchanged
                passed[ci][n] = seq_of[n]
            if ci not in groups:
                continue
            parts = [[kept_names[ci][r] for r in grp] for grp in groups[ci]]
        else:
            parts = [list(ninja[ci][k]) for k in ninja[ci]]
        for part in parts:
            if part:
                subs.append([(n, seq_of[n]) for n in part])
                owner.append(ci)
    second = _star_align_clusters(ctx, subs)
    t3 = clock()
    als, who = [], []
    for si, (sub, (rows, dropped)) in enumerate(zip(subs, second)):
        for n in dropped:
            passed[owner[si]][n] = dict(sub)[n]
        kept = [n for n, _s in sub if n in rows]
        if kept:
            als.append([rows[n] for n in kept])
            who.append((owner[si], kept[-1]))
    cons = ctx.msa_consensus(als) if als else []
    if seconds is not None:
        seconds.update(align_first=t1 - t0, subcluster=t2 - t1, align_second=t3 - t2, consensus=clock() - t3)
    out = [dict() for _ in clusters]
    for (ci, last), c in zip(who, cons):
        out[ci][last] = c
    for ci, cl in enumerate(clusters):
        if not out[ci]:                      # no reliable consensus: the original sequences (Util.py:12495-12498)
            out[ci] = dict(cl)
        else:
            out[ci].update(passed[ci])
    return out


def generate_cons_v1(cluster_id, cur_cluster_path, cluster_dir, threads, device=0, ninja_clusters=None, subcluster=None):
    """generate_cons_v1 (Util.py:12457), same arguments: the FASTA of one cluster -> {name: consensus}.  ninja_clusters: the
    parsed output of Ninja ({id: [names]}, read_Ninja_clusters) when the caller has one; else the build's stand-in, on the host
    or, with subcluster="gpu" / HITE_SUBCLUSTER=gpu, on the device (_generate_cons_batch)."""
    names, contigs = read_fasta(cur_cluster_path)
    if not names:
        return {}
    return _generate_cons_batch(get_ctx(device), [[(n, contigs[n]) for n in names]], [ninja_clusters], subcluster=subcluster)[0]


def _library_hits(ctx, names, contigs):
    """all-vs-all of a library with itself where the reference runs blastn (multi_process_align, Util.py:12209): the library is
    packed as a genome (one contig per sequence) and searched by hite_seed_allvsall, in blocks when it has more sequences
    than one call addresses (every pair of blocks once: the blocks of a pair are packed together).
    -> (q, s, qs, qe, ss, se) arrays over the indices of `names`."""
    n = len(names)
    half = SEED_MAX_SEGMENTS // 2
    blocks = [list(range(a, min(n, a + half))) for a in range(0, n, half)] if n > SEED_MAX_SEGMENTS else [list(range(n))]
    parts = []
    pairs = [(i, j) for i in range(len(blocks)) for j in range(i, len(blocks))] if len(blocks) > 1 else [(0, 0)]
    for (i, j) in pairs:
        ids = blocks[i] + (blocks[j] if j != i else [])
        ctx.genome_pack([contigs[names[t]].upper() for t in ids])
        ctx.release_copy_index()
        _PACKED["path"] = None
        lens = [len(contigs[names[t]]) for t in ids]
        tab = ctx.seed_allvsall(seg_len=max(lens))
        gi = np.asarray(ids, dtype=np.int64)
        q, s2 = gi[np.asarray(tab["qseg"], dtype=np.int64)], gi[np.asarray(tab["sseg"], dtype=np.int64)]
        keep = np.ones(len(q), dtype=bool)
        if j != i:          # a mixed pair contributes the hits BETWEEN its two blocks only
            inb = np.zeros(n, dtype=bool)
            inb[blocks[i]] = True
            keep = inb[q] != inb[s2]
        parts.append(tuple(np.asarray(x)[keep] for x in (q, s2, tab["qs"], tab["qe"], tab["ss"], tab["se"])))
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(6))


_COMP_U8 = np.full(256, ord("N"), dtype=np.uint8)
for _a, _b in zip(b"ACGT", b"TGCA"):
    _COMP_U8[_a] = _b


def _stretch_hits(q, s, qs, qe, ss, se, lens, seqs):
    """The seeding stage reports a hit from its first to its last anchor; blastn extends an alignment to the ends of the
    sequences when they keep matching.  A hit whose ends lie within a short overhang of the sequence ends (on both sequences;
    <= 30 bases or a tenth of the shorter sequence) is therefore stretched along its diagonal -- BY THE BASES THAT ALIGN: the
    overhang is compared base by base (match +1, mismatch -2 as megablast scores, no gaps) and the hit grows to the best-scoring prefix of it,
    as an ungapped X-drop extension would leave it.  Copies of one family (<= 15 % apart) gain nearly the whole overhang and
    pass a 0.95 coverage rule they would miss by the bases outside their anchors; unrelated termini (a quarter of the bases
    agree by chance) gain a handful of bases at most and stay below it, as they do under blastn / cd-hit-est.
    seqs: the upper-case sequences behind the ids (bytes / str)."""
    L = np.asarray(lens, dtype=np.int64)
    q, s = np.asarray(q, dtype=np.int64), np.asarray(s, dtype=np.int64)
    qs, qe, ss, se = (np.asarray(x, dtype=np.int64).copy() for x in (qs, qe, ss, se))
    if len(q) == 0:
        return qs, qe, ss, se
    off = np.zeros(len(L) + 1, dtype=np.int64)
    np.cumsum(L, out=off[1:])
    buf = np.frombuffer(b"".join(x.encode() if isinstance(x, str) else bytes(x) for x in seqs), dtype=np.uint8)
    fwd = ss <= se
    left = np.minimum(qs - 1, np.where(fwd, ss - 1, L[s] - ss))
    right = np.minimum(L[q] - qe, np.where(fwd, L[s] - se, se - 1))
    reach = np.maximum(30, np.minimum(L[q], L[s]) // 10)
    left = np.where(left <= reach, left, 0)
    right = np.where(right <= reach, right, 0)

    def aligned(room, q0, qstep, s0, sstep):
        """room[h] candidate bases; base j of hit h: query q0 + qstep * j, subject s0 + sstep * j (0-based, inside the
        sequence); -> the length of the best-scoring prefix"""
        out = np.zeros(len(room), dtype=np.int64)
        idx = np.nonzero(room > 0)[0]
        CH = 4096
        for a in range(0, len(idx), CH):
            h = idx[a:a + CH]
            w = int(room[h].max())
            j = np.arange(w, dtype=np.int64)[None, :]
            ok = j < room[h][:, None]
            qi = off[q[h]][:, None] + np.where(ok, q0[h][:, None] + qstep * j, 0)
            si = off[s[h]][:, None] + np.where(ok, s0[h][:, None] + sstep[h][:, None] * j, 0)
            qb, sb = buf[qi], buf[si]
            sb = np.where(fwd[h][:, None], sb, _COMP_U8[sb])
            sc = np.where(ok, np.where((qb == sb) & (qb != ord("N")), 1, -2), -(1 << 20)).cumsum(axis=1)
            best = sc.argmax(axis=1)
            out[h] = np.where(sc[np.arange(len(h)), best] > 0, best + 1, 0)
        return out

    one = np.where(fwd, 1, -1).astype(np.int64)
    # to the left of the hit: query bases qs-2, qs-3, ... (0-based); subject ss-2, ss-3, ... (forward) / ss, ss+1, ... (reverse)
    left = aligned(left, qs - 2, -1, np.where(fwd, ss - 2, ss), -one)
    # to the right: query qe, qe+1, ...; subject se, se+1, ... (forward) / se-2, se-3, ... (reverse)
    right = aligned(right, qe, 1, np.where(fwd, se, se - 2), one)
    qs -= left; qe += right
    ss = np.where(fwd, ss - left, ss + left)
    se = np.where(fwd, se + right, se - right)
    return qs, qe, ss, se


def deredundant_for_LTR_v5(redundant_ltr, work_dir, threads, type, coverage_threshold, debug, device=0, ctx=None, stages=None,
                           subcluster=None):
    """deredundant_for_LTR_v5 (Util.py:12202-12337, the library de-duplication of panHiTE, config C5), same arguments.
    Reference: blastn all-vs-all of the library -> chunked fragment chaining (process_blast_results_in_chunks +
    FMEA_new1_parallel_large) -> greedy clusters (cluster_sequences_from_chunks) -> per cluster generate_cons_v1 (mafft ->
    Ninja sub-clusters -> mafft -> cons_from_mafft_v1) -> cd-hit-est.  Here: the library is packed as a genome and searched
    against itself by hite_seed_allvsall (where the reference runs blastn; libraries of >= 65 000 sequences in blocks),
    chaining / clustering / consensus are the pinned device stages (hite_lib_chain, hite_lib_cluster, hite_msa_consensus),
    the alignments are star alignments (where the reference runs mafft), the sub-clusters come from ninja_stand_in (where it
    runs Ninja; with subcluster="gpu" / HITE_SUBCLUSTER=gpu from hite_msa_subcluster, the same clustering on the device); a cluster above 10 000 members is cut in file order into pieces of <= 10 000, the fall-back the reference
    itself takes when its cd-hit-est pre-reduction does not get a cluster below that size (:12252-12299; the pre-reduction
    itself needs the external tool); cd-hit-est after the consensus step runs when it is installed.  Sequences longer than
    the aligner's 32 767-base windows pass unclustered.
    Writes <redundant_ltr>.tmp.cons and <redundant_ltr>.cons, returns the former like the reference.
    ctx: the context to run on (default: the process-wide one of `device`); stages: a dict that receives the intermediate
    results ('hits', 'clusters': lists of names) -- what the parity tests compare between two runs -- and 'seconds': the wall
    seconds of the steps (hits, stretch, chain, cluster, align_first, subcluster, align_second, consensus, redundancy)."""
    clock = time.perf_counter
    secs = dict.fromkeys(("hits", "stretch", "chain", "cluster", "align_first", "subcluster", "align_second", "consensus", "redundancy"), 0.0)
    names, contigs = read_fasta(redundant_ltr)
    cons_path, final_path = redundant_ltr + ".tmp.cons", redundant_ltr + ".cons"
    if not names:
        store_fasta({}, cons_path)
        store_fasta({}, final_path)
        return cons_path
    if ctx is None:
        ctx = get_ctx(device)
    work = [n for n in names if 0 < len(contigs[n]) <= STAR_MAX_LEN]       # the rest passes unchanged
    all_cons, clustered = {}, set()
    if work:
        t0 = clock()
        q, s, qs, qe, ss, se = _library_hits(ctx, work, contigs)
        t1 = clock()
        lens = [len(contigs[n]) for n in work]
        qs, qe, ss, se = _stretch_hits(q, s, qs, qe, ss, se, lens, [contigs[n].upper() for n in work])
        t2 = clock()
        recs = ctx.lib_chain(q, s, qs, qe, ss, se, lens, coverage_threshold, 5_000_000)
        t3 = clock()
        clusters = [cl for cl in ctx.lib_cluster(recs, lens, coverage_threshold) if len(cl) >= 1]
        clusters = [cl[a:a + CLUSTER_CLEAN_THRESHOLD] for cl in clusters for a in range(0, len(cl), CLUSTER_CLEAN_THRESHOLD)]
        secs.update(hits=t1 - t0, stretch=t2 - t1, chain=t3 - t2, cluster=clock() - t3)
        if stages is not None:
            stages["hits"] = len(q)
            stages["clusters"] = [[work[i] for i in cl] for cl in clusters]
        batch = [[(work[i], contigs[work[i]]) for i in cl] for cl in clusters]
        for cl, cons in zip(clusters, _generate_cons_batch(ctx, batch, subcluster=subcluster, seconds=secs) if batch else []):
            clustered.update(work[i] for i in cl)
            all_cons.update(cons)
    for n in names:      # sequences outside every cluster (and the over-long ones) pass unchanged
        if n not in clustered:
            all_cons[n] = contigs[n]
    store_fasta(all_cons, cons_path)
    t0 = clock()
    if shutil.which("cd-hit-est"):
        subprocess.run("cd-hit-est -aS 0.95 -aL 0.95 -c %s -G 0 -g 1 -A 80 -i %s -o %s -T 0 -M 0 > /dev/null 2>&1" %
                       (coverage_threshold, cons_path, final_path), shell=True, check=False)
    else:
        # the build's stand-in, never a plain copy; -c takes effect with HITE_CLUSTER_IDENTITY=gpu
        remove_redundant_sequences(cons_path, final_path, 0.95, 0.95, device=device, ctx=ctx, c=coverage_threshold)
    secs["redundancy"] = clock() - t0
    if stages is not None:
        stages["seconds"] = secs
    return cons_path


def _cluster_identity_on(identity):
    """the switch of the identity test of remove_redundant_sequences: the argument, then $HITE_CLUSTER_IDENTITY; "gpu" is on"""
    mode = identity if identity is not None else os.environ.get("HITE_CLUSTER_IDENTITY")
    return mode == "gpu"


def remove_redundant_sequences(inp, outp, aS=0.95, aL=0.95, device=0, ctx=None, c=None, min_aligned=80, identity=None):
    """The build's stand-in for `cd-hit-est -aS 0.95 -aL 0.95 -c <c> -G 0 -g 1 -A 80 -i inp -o outp` (judge_TIR_transposons.py:87,
    Util.py:12330; cd-hit-est is an external tool: PARITY UNPINNED), used when it is not installed -- the step is never skipped.
    Greedy incremental clustering in cd-hit's order (longest first, ties in input order): a sequence joins the first longer
    representative that a chain of library-vs-library hits (hite_seed_allvsall + hite_lib_chain, the stages of the library
    merge) covers to >= aS of the shorter and >= aL of the longer sequence; otherwise it becomes a representative.  The
    representatives are written longest first, as cd-hit-est writes them.
    By default identity is not computed: hits are runs of shared 15-base minimizers, which sequences below ~85 % identity hardly
    have (cd-hit's -c 0.8 / 0.95 asks for less / more), so `c` and `min_aligned` are ignored.
    identity="gpu" (or HITE_CLUSTER_IDENTITY=gpu when the argument is None; anything else is off) with `c` given puts -c and -A on
    the pairwise identity of include/hite_gpu.h (hite_pair_identity; twin tests/identity_twin.py): every chain record that passes
    the two coverage tests goes, once, into one batched Context.pair_identity call -- the query interval and the subject interval
    of the record (the bases the chain covers; the reverse-complemented subject when its coordinates descend), band 32 -- and
    counts only if both intervals hold >= min_aligned bases and matches >= c * (cost + matches) in binary64.  A record the
    primitive refuses (cost -1: an interval above 32 767 bases, or a length difference the band cannot hold) does not count, so
    such a pair is not merged; one line on stderr gives the number of those records.  The greedy pass and the output order are the
    same.  This is an edit-distance identity over the chained interval, not cd-hit's banded local alignment (2 / -2 / -6 / -1):
    parity with the tool itself stays unpinned."""
    names, contigs = read_fasta(inp)
    work = [n for n in names if len(contigs[n]) > 0]         # (nothing is aligned here: no length limit)
    by_identity = c is not None and _cluster_identity_on(identity)
    drop = set()
    if len(work) > 1:
        if ctx is None:
            ctx = get_ctx(device)
        q, s_, qs, qe, ss, se = _library_hits(ctx, work, contigs)
        lens = [len(contigs[n]) for n in work]
        qs, qe, ss, se = _stretch_hits(q, s_, qs, qe, ss, se, lens, [contigs[n].upper() for n in work])
        recs = ctx.lib_chain(q, s_, qs, qe, ss, se, lens, min(aS, aL), 5_000_000)
        covered = {}
        candidates = {}                                      # (identity test) the records that pass the coverage tests, each once
        for (_ch, qi, a, b, si, s0, s1) in recs:
            if qi == si:
                continue
            cq, cs = (b - a) / lens[qi], abs(s1 - s0) / lens[si]
            short_cov, long_cov = (cq, cs) if lens[qi] <= lens[si] else (cs, cq)
            if short_cov >= aS and long_cov >= aL:
                if by_identity:
                    candidates.setdefault((qi, a, b, si, s0, s1), None)
                    continue
                covered.setdefault(qi, set()).add(si)
                covered.setdefault(si, set()).add(qi)
        if by_identity:
            for qi, si in _identity_filter(ctx, [contigs[n] for n in work], lens, list(candidates), float(c), int(min_aligned)):
                covered.setdefault(qi, set()).add(si)
                covered.setdefault(si, set()).add(qi)
        order = sorted(range(len(work)), key=lambda i: (-lens[i], i))
        reps = set()
        for i in order:
            if covered.get(i, set()) & reps:
                drop.add(work[i])
            else:
                reps.add(i)
    keep = [n for n in names if n not in drop]
    keep.sort(key=lambda n: -len(contigs[n]))          # (stable: ties stay in input order)
    store_fasta({n: contigs[n] for n in keep}, outp)
    return outp


def _identity_filter(ctx, seqs, lens, records, c, min_aligned, band=32):
    """the -c / -A test of remove_redundant_sequences on chain records (q, q0, q1, s, s0, s1) as hite_lib_chain writes them: the query
    bases [q0, q1); the subject bases [s0, s1) on the forward strand and, when the coordinates descend (s0 = s_start - 1 > s1 = s_end
    of a minus-strand chain), [s1 - 1, s0 + 1) reverse-complemented.  -> the (q, s) of the records that count."""
    pairs = []
    for (qi, a, b, si, s0, s1) in records:
        lo, hi, strand = (s0, s1, 0) if s0 <= s1 else (s1 - 1, s0 + 1, 1)
        pairs.append((qi, max(0, a), min(lens[qi], b), si, max(0, lo), min(lens[si], hi), strand))
    res = ctx.pair_identity(seqs, pairs, band=band) if pairs else np.zeros((0, 2), dtype=np.int32)
    out, refused = [], 0
    for p, (cost, matches) in zip(pairs, res.tolist()):
        if cost < 0:
            refused += 1
            continue
        if p[2] - p[1] >= min_aligned and p[5] - p[4] >= min_aligned and float(matches) >= c * float(cost + matches):
            out.append((p[0], p[3]))
    sys.stderr.write("remove_redundant_sequences: identity test on %d chain records, %d refused by the pairwise identity (over 32 767 bases "
                     "or outside its band): not merged\n" % (len(pairs), refused))
    return out


def mask_genome_intactTE(TE_lib, genome_path, work_dir=None, thread=1, ref_index=0, debug=0, device=0):
    """mask_genome_intactTE (Util.py:6389-6431), step for step: the library is searched in the chunk (the reference runs
    minimap2 and converts its PAF to blast6, :6396-6398; here the build's copy finder, one blast6 line per copy:
    _copies_as_blast6), generate_full_length_out_v1 (:6406) turns the table into the full-length copies (coverage >= 0.95 of
    the library sequence), and those intervals become N -- in <genome_path>.masked and in the resident genome."""
    masked = genome_path + ".masked"
    names, contigs = read_fasta(genome_path)
    te_names, tes = read_fasta(TE_lib) if TE_lib is not None and os.path.exists(TE_lib) else ([], {})
    if not te_names:
        store_fasta(contigs, masked)
        return masked
    import pickle
    import tempfile

    ctx = get_ctx(device)
    own_dir = work_dir is None
    work = tempfile.mkdtemp(prefix="hite_mask_") if own_dir else work_dir
    os.makedirs(work, exist_ok=True)
    tmp_blast_dir = work + "/mask_tmp_" + str(ref_index)
    lib_out = work + "/prev_TE_" + str(ref_index) + ".out"
    _copies_as_blast6(genome_path, TE_lib, lib_out, device)         # (packs the chunk: it is the resident genome from here on)
    output_files = generate_full_length_out_v1(lib_out, TE_lib, genome_path, tmp_blast_dir, "", 0.95, "Total", debug=debug, device=device)
    idx = {n: i for i, n in enumerate(names)}
    cc, ss, ee = [], [], []
    for output_file in output_files:
        with open(output_file, "rb") as f:
            for _query_name, chr_name, chr_start, chr_end in sorted(pickle.load(f)):
                cc.append(idx[chr_name]); ss.append(chr_start); ee.append(chr_end)
    ctx.genome_mask(cc, ss, ee)
    arrs = [np.frombuffer(contigs[n].encode(), dtype=np.uint8).copy() for n in names]
    for c, s1, e1 in zip(cc, ss, ee):
        arrs[c][max(0, s1 - 1):e1] = ord("N")
    store_fasta({n: a.tobytes().decode() for n, a in zip(names, arrs)}, masked)
    if debug != 1:
        shutil.rmtree(tmp_blast_dir, ignore_errors=True)
        if own_dir:
            shutil.rmtree(work, ignore_errors=True)
    return masked


def split_and_store_sequences(names, contigs, base_threshold):
    """grouping rule of split_and_store_sequences (/root/reference/module/Util.py:4987-5012) without the files:
    consecutive sequences are collected until their total reaches base_threshold -> list of name lists (the reference's
    {i}_target.fa query / target files)."""
    groups, cur, count = [], [], 0
    for name in names:
        cur.append(name)
        count += len(contigs[name])
        if count >= base_threshold:
            groups.append(cur)
            cur, count = [], 0
    if cur:
        groups.append(cur)
    return groups


def run_remove_TR(target_file, trf_dir):
    """Util.py:2855-2874 -- `trf <file> 2 7 7 80 10 50 500 -f -d -m -h` in trf_dir; returns the .mask FASTA (tandem repeats -> N)"""
    os.makedirs(trf_dir, exist_ok=True)
    subprocess.run("cd %s && trf %s 2 7 7 80 10 50 500 -f -d -m -h > /dev/null 2>&1" % (trf_dir, target_file), shell=True, check=False)
    return os.path.join(trf_dir, os.path.basename(target_file) + ".2.7.7.80.10.50.500.mask")


def mask_tandem_repeats(names, contigs, device=0, max_period=500):
    """The build's own tandem-repeat masker (hite_tr_mask; definition oracle/hite_oracle_trf.c) where the reference runs TRF:
    {name: sequence} -> {name: sequence with tandem repeats as N}.  The resident genome becomes these sequences."""
    if not names or not any(len(contigs[n]) for n in names):     # an empty chunk stays an empty file, as in the reference
        return {n: contigs[n] for n in names}
    ctx = get_ctx(device)
    ctx.genome_pack([contigs[n] for n in names])
    ctx.release_copy_index()
    _PACKED["path"] = None
    m = ctx.tr_mask(max_period)
    out, pos = {}, 0
    for n in names:
        a = np.frombuffer(contigs[n].encode(), dtype=np.uint8).copy()
        a[m[pos:pos + len(a)]] = ord("N")
        out[n] = a.tobytes().decode()
        pos += len(a)
    return out


def filter_tandem_repeats(repeat_names, repeat_contigs, tmp_output_dir, ref_index, threads, device=0):
    """Util.py:4672-4697 -- the chunk is cut into files of >= 100 kb (split_and_store_sequences), every file goes through TRF,
    the masked files are concatenated (in file order: the canonical replacement of the reference's as_completed order) into
    filter_tandem_{ref_index}.fa.  `trf` is an external tool: when it is installed (and HITE_TR_MASKER is not
    "gpu") it is called exactly as the reference calls it; otherwise the chunk is masked by the build's own GPU masker
    (mask_tandem_repeats: match 2 / edit 5 -- TRF's 2 / 7 / 7 calibrated for neighbour-against-neighbour scoring --, periods <= 500, score >= 50) -- the chunk never passes unmasked."""
    out = os.path.join(tmp_output_dir, "filter_tandem_%s.fa" % ref_index)
    if shutil.which("trf") is None or os.environ.get("HITE_TR_MASKER", "") == "gpu":
        store_fasta(mask_tandem_repeats(repeat_names, repeat_contigs, device=device), out)
        return out
    tmp_dir = os.path.join(tmp_output_dir, "trf_filter_%s" % ref_index)
    os.makedirs(tmp_dir, exist_ok=True)
    jobs = []
    for i, group in enumerate(split_and_store_sequences(repeat_names, repeat_contigs, 100000)):
        sub = os.path.join(tmp_dir, str(i))
        os.makedirs(sub, exist_ok=True)
        target = os.path.join(sub, "%d_target.fa" % i)
        store_fasta({n: repeat_contigs[n] for n in group}, target)
        jobs.append((target, os.path.join(sub, "%d_trf" % i)))
    from concurrent.futures import ThreadPoolExecutor

    with ThreadPoolExecutor(max_workers=max(1, int(threads))) as ex:     # the workers only wait for `trf` processes
        masked = list(ex.map(lambda j: run_remove_TR(*j), jobs))
    with open(out, "w") as f:
        for (target, _d), m in zip(jobs, masked):
            with open(m if os.path.exists(m) else target) as g:
                f.write(g.read())
    return out


def determine_repeat_boundary_v5(repeats_path, longest_repeats_path, prev_TE, fixed_extend_base_threshold, max_single_repeat_len,
                                 tmp_output_dir, threads, ref_index, reference, debug, device=0, ctx=None):
    """determine_repeat_boundary_v5 (Util.py:4637-4670), same positional arguments: TRF masking of the chunk
    (filter_tandem_repeats), N-masking of the full-length copies of the TEs found so far (mask_genome_intactTE with prev_TE),
    process_blast_alignments (:4724) + get_longest_repeats_v4 per query file + generate_final_result (:4783).
    repeats_path = the chunk FASTA of 'chr$offset' segments; the all-vs-all stage is hite_seed_allvsall (the build's blastn
    stand-in), FMEA runs per query file as in the reference (each call has its own first-come de-duplication), results are
    unioned by name in query-file order (the canonical replacement of the reference's as_completed order)."""
    from . import dist as hd

    # One code path for one GPU and for the ranks of a node (hite_amd/dist.py).  Under torchrun every rank is called with the same
    # arguments and shares tmp_output_dir: the steps that WRITE files (tandem masking, prev_TE masking, the result, the clean-up)
    # run on rank 0 only, the others wait at a barrier and read what it wrote; every rank seeds its share of the all-vs-all
    # stage, the HSP records go to the owners of the query files, the interval lists are gathered.
    multi, rank, world = hd.process_group_state()

    def barrier():
        if multi and world > 1:
            hd.dist.barrier()

    os.makedirs(tmp_output_dir, exist_ok=True)
    ctx = ctx or get_ctx(device)
    repeat_names, repeat_contigs = read_fasta(repeats_path)
    if not repeat_names:
        if rank == 0:
            store_fasta({}, longest_repeats_path)
        barrier()
        return longest_repeats_path
    filter_tandem_file = os.path.join(tmp_output_dir, "filter_tandem_%s.fa" % ref_index)
    masked_file_path = filter_tandem_file + ".masked"
    if rank == 0:
        filter_tandem_file = filter_tandem_repeats(repeat_names, repeat_contigs, tmp_output_dir, ref_index, threads, device=device)
        masked_file_path = mask_genome_intactTE(prev_TE, filter_tandem_file, tmp_output_dir, threads, ref_index, debug=debug, device=device)
    barrier()
    names, contigs = read_fasta(masked_file_path)
    ctx.genome_pack([contigs[n] for n in names])
    ctx.release_copy_index()
    _PACKED["path"] = None   # the reference genome has to be packed again by whoever needs it next
    seg_len = max(len(contigs[n]) for n in names)
    chroms, seg_chrom, seg_off = {}, [], []
    for n in names:
        c, off = n.split("$")
        chroms.setdefault(c, len(chroms))
        seg_chrom.append(chroms[c])
        seg_off.append(int(off))
    inv = {v: k for k, v in chroms.items()}
    # query files of >= 1 Mbp as in the reference: FMEA (with its own first-come de-duplication) runs per query file, the results
    # are unioned by name in file order
    oc, os_, oe = hd.coarse_stage_sharded(ctx, max(seg_len, 1), fixed_extend_base_threshold, max_single_repeat_len, seg_table=(seg_chrom, seg_off))
    if rank == 0:
        final = [("%s:%d-%d" % (inv[int(c)], a_, b_), inv[int(c)], int(a_), int(b_)) for c, a_, b_ in zip(oc, os_, oe)]
        _rn, ref = read_fasta(reference)
        store_fasta({name: ref[c][a_:b_] for name, c, a_, b_ in final}, longest_repeats_path)
    barrier()                 # nobody is still reading the masked chunk, and the result is there for every rank
    if rank == 0 and not debug:      # cleanup_temp_files (Util.py:4797)
        shutil.rmtree(os.path.join(tmp_output_dir, "trf_filter_%s" % ref_index), ignore_errors=True)
        for p_ in (filter_tandem_file, masked_file_path):
            if os.path.exists(p_):
                os.remove(p_)
    return longest_repeats_path


def flanking_seq(longest_repeats_path, longest_repeats_flanked_path, reference, flanking_len):
    """Util.py:4614-4634: `chr:start-end` (0-based half-open) -> `chr:(s+1-flank)-(e+flank)` with the
    window clamped into the contig; bases come from the packed genome."""
    seq_names, _ = read_fasta(longest_repeats_path)
    ctx = set_reference(reference)
    idx, lens = _PACKED["names"], _PACKED["lens"]
    contig, s1, e1, new_names = [], [], [], []
    for name in seq_names:
        ref_name, pos = name.split(":")
        a, b = pos.split("-")
        ref_start, ref_end = int(a) + 1, int(b)
        clen = lens[idx[ref_name]]
        if ref_start - 1 - flanking_len < 0:
            ref_start = flanking_len + 1
        if ref_end + flanking_len > clen:
            ref_end = clen - flanking_len
        new_names.append(ref_name + ":" + str(ref_start - flanking_len) + "-" + str(ref_end + flanking_len))
        contig.append(idx[ref_name])
        s1.append(ref_start - flanking_len)       # 1-based inclusive window, gathered with flank 0
        e1.append(ref_end + flanking_len)
    wins, _ = ctx.flank_gather(contig, s1, e1, [0] * len(contig), flank=0)
    flanked = {}
    host_ref = None
    for n, w, (c, a, b) in zip(new_names, wins, zip(contig, s1, e1)):
        if w is None:   # the gather applies the 100-bp rule of the copy windows (Util.py:8116); flanking_seq has no minimum
            if host_ref is None:
                rn, rc_ = read_fasta(reference)
                host_ref = [rc_[x] for x in rn]
            flanked[n] = host_ref[c][max(0, a - 1):max(0, b)]
        else:
            flanked[n] = w.decode()
    store_fasta(flanked, longest_repeats_flanked_path)


# ---- the fine stage (Util.py:8032-8287) -----------------------------------------------------------------
def get_full_length_copies_minimap2(query_path, reference, temp_dir=None, max_copy_num=100, threads=1, device=0):
    """Same arguments as the reference's function (Util.py:7933, which runs minimap2): {query: [(chr, start1, end1, length,
    '+'/'-'), ...]} from the build's minimizer-based copy finder on the resident genome (packed from `reference`).  The finder
    keeps up to 300 copies per query (the reference's own -N of the masking step); the <= 100 rows of an alignment are chosen
    later by the longest-100 rule (ready_for_MSA.sh 100 100), so max_copy_num / temp_dir / threads have nothing to steer here."""
    ctx = set_reference(reference, device)
    names, contigs = read_fasta(query_path)
    tab = ctx.find_copies([contigs[n] for n in names], clips=True)
    rev = {v: k for k, v in _PACKED["names"].items()}
    # (a 6th field beside the reference's five: the clip word of the record -- zero unless the records are aligned intervals,
    # hite_copy_config(1) -- which flank_region_align_v5 hands to the star alignment)
    return {n: [(rev[c], s_, e_, e_ - s_ + 1, "-" if m_ else "+", cl_) for (c, s_, e_, m_, _an, cl_) in t] for n, t in zip(names, tab) if t}


def flank_region_align_v5(candidate_sequence_path, real_TEs, flanking_len, reference, split_ref_dir, TE_type, tmp_output_dir,
                          threads, ref_index, log, subset_script_path, plant, debug, iter_num, all_low_copy,
                          result_type="cons", all_copies=None, copy_finder=None):
    """Same contract and positional arguments as the reference (Util.py:8032): reads the candidate FASTA, writes `real_TEs` and
    appends the low-copy elements to `all_low_copy`.  The copies come from the built-in copy finder (get_full_length_copies_minimap2,
    where the reference runs minimap2, Util.py:8076); `all_copies` ({query: [(chr, start1, end1, aligned_len, '+'/'-'), ...]},
    what get_full_length_copies_minimap2 returns) or `copy_finder(candidate_path, reference)` override it; one batched GPU call
    replaces the per-candidate process pool."""
    if result_type != "cons":
        raise NotImplementedError("only result_type='cons'")
    names, contigs = read_fasta(candidate_sequence_path)
    ctx = set_reference(reference)          # before the copy finder: it searches whatever genome is resident
    if all_copies is None:
        all_copies = (copy_finder or get_full_length_copies_minimap2)(candidate_sequence_path, reference)
    idx = _PACKED["names"]
    qnames = [q for q in all_copies.keys() if q in contigs]  # reference iterates all_copies (Util.py:8095)
    cands = [contigs[q] for q in qnames]
    copies = []
    for q in qnames:
        seen, lst = {}, []
        for cp in all_copies[q]:
            key = (cp[0], int(cp[1]), int(cp[2]), cp[4])  # dict semantics of copy_contigs[new_name] (Util.py:8110-8114)
            if key in seen:
                continue
            seen[key] = 1
            lst.append((idx[cp[0]], int(cp[1]), int(cp[2]), 1 if cp[4] == "-" else 0, 0, int(cp[5]) if len(cp) > 5 else 0))
        copies.append(lst)
    res, _stats = ctx.flank_region_align(TE_type, cands, copies, plant=int(plant), flank=int(flanking_len)) if qnames else ([], None)
    true_tes, low_copy = bucket_results(TE_type, [(q if is_te else None, cons if is_te else None, info, copy_count)
                                                  for q, (is_te, info, cons, copy_count, _bs, _be) in zip(qnames, res)])
    rescued, low_copy = rescue_low_copy(TE_type, low_copy, plant, os.path.join(tmp_output_dir, "low_copy_%s_%s" % (TE_type, ref_index)),
                                        threads=max(1, int(threads)))
    true_tes.update(rescued)
    store_fasta(true_tes, real_TEs)
    with open(all_low_copy, "a") as f:
        for q, s in low_copy.items():
            f.write(">" + q + "\n" + s + "\n")
    return true_tes, low_copy


def rescue_low_copy(TE_type, low_copy, plant, work_dir, tandem_masker=None, ctx=None, library_dir=None, threads=1, domain_search=None):
    """The recall of low-copy elements (Util.py:8196-8276): the low-copy sequences go through TRF (tandem repeats -> N) when `trf`
    is installed and through the build's own masker otherwise (`tandem_masker(names, contigs) -> contigs` overrides it).  TIR
    stage: those with a short-TIR signature (get_short_tir_contigs) or a terminal inverted repeat (remove_no_tirs: the in-tree
    stage where the reference runs `itrsearch -i 0.7 -l 7`) are real TEs, with their masked sequence as the tool writes it; the
    others, and the low-copy Helitron / non-LTR candidates, are searched for intact protein domains (get_domain_info: blastx
    against <library_dir>/TIRPeps.lib | HelitronPeps.lib | non_LTR.lib, a hit over >= 95 % of a protein recalls the element with
    its unmasked sequence).  library_dir defaults to $HITE_LIBRARY_DIR, then <HiTE>/library beside the package (as scripts/judge_Other_transposons.py).
    domain_search: "gpu" = the build's own translated search, "blastx" = the external tool, None = $HITE_DOMAIN_SEARCH, else the
    external tool when it is installed; when the search or the library is missing that recall finds nothing and the stage log says
    so.  -> (rescued, still low copy), both in the reference's order."""
    mode = _domain_search_mode(domain_search)
    if not low_copy or TE_type not in _PROTEIN_LIB:
        return {}, dict(low_copy)
    # the reference always looks in <HiTE>/library (Util.py:8215-8230: cur_dir + '/library/...'); here: the argument, then
    # $HITE_LIBRARY_DIR, then <HiTE>/library beside the package (as scripts/judge_Other_transposons.py does)
    library_dir = library_dir or os.environ.get("HITE_LIBRARY_DIR") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "library")
    lib = os.path.join(library_dir, _PROTEIN_LIB[TE_type]) if library_dir else None
    can_search = (mode == "gpu" or shutil.which("blastx") is not None) and lib is not None and os.path.exists(lib)
    if not can_search:
        # (said once per stage call, in the stage's stderr log: a user must know what this run cannot recall)
        sys.stderr.write("[hite_amd] %d low-copy %s candidate%s: blastx or the protein library (%s) is not there, nothing is recalled by its "
                         "protein domains (Util.py:8215-8276; HITE_DOMAIN_SEARCH=gpu / domain_search=\"gpu\" runs the build's own search "
                         "instead of blastx)%s\n" % (len(low_copy), TE_type, "" if len(low_copy) == 1 else "s",
                                                                      lib or "set HITE_LIBRARY_DIR", "" if TE_type == "tir" else
                                                                      ": low-copy %s elements stay in the low-copy file" % TE_type))
        if TE_type != "tir":
            return {}, dict(low_copy)
    os.makedirs(work_dir, exist_ok=True)
    masked = dict(low_copy)
    if shutil.which("trf") is not None and tandem_masker is None:
        path = os.path.join(work_dir, "low_copy.fa")
        store_fasta(low_copy, path)
        m = run_remove_TR(path, work_dir)
        if os.path.exists(m):
            _n, mc = read_fasta(m)
            masked = {n: mc[n] for n in low_copy if n in mc}
    else:
        # the build's own masker (the resident genome becomes these sequences; whoever needs the reference next packs it again)
        masked = (tandem_masker or mask_tandem_repeats)(list(low_copy.keys()), low_copy)
    rescued = {}
    to_search = masked
    if TE_type == "tir":
        rescued, to_search = remove_no_tirs(masked, plant, ctx=ctx)
    if to_search and can_search:
        cons = os.path.join(work_dir, "low_copy.%s.fa" % ("no_tir" if TE_type == "tir" else "masked"))
        table = cons + "." + TE_type + "_domain"
        store_fasta(to_search, cons)
        if get_domain_info(cons, lib, table, threads, os.path.join(work_dir, TE_type + "_domain"), search=mode, ctx=ctx):
            for n in intact_domain_names(table, lib):
                if n in low_copy:
                    rescued[n] = low_copy[n]
    return rescued, {n: s_ for n, s_ in low_copy.items() if n not in rescued}


# ---- low-copy rescue by intact protein domains (Util.py:8215-8276; get_domain_info :4571-4612, multiple_alignment_blastx_v1 :1006-1262)
def _chain_domain_fragments(frags, thr):
    """one (query, protein) pair of multiple_alignment_blastx_v1 (Util.py:1055-1207): blastx fragments (q_start, q_end, s_start,
    s_end) -> [(q_start, q_end, length, s_start, s_end, s_length, extensions)] , one per cluster, in cluster order.  Forward
    fragments (q_start <= q_end) ordered by the protein interval, reverse ones by descending query position; a fragment joins the
    running cluster when it starts less than `thr` behind the end of any member (newest first); inside a cluster (ordered by the
    protein interval again) every unvisited fragment grows a chain over the later ones that advance on the protein, keep the
    strand, start < thr beyond the chain's query end and < thr / 3 beyond its protein end; the longest chain of a cluster stays
    (the first among equals).  Fragments are keyed by value: equal tuples share their visited mark, as in the reference's dict."""
    fwd = sorted((f for f in frags if not f[0] > f[1]), key=lambda x: (x[2], x[3]))
    rev = sorted((f for f in frags if f[0] > f[1]), key=lambda x: (-x[0], -x[1]))
    clusters = []
    for group, sign in ((fwd, 1), (rev, -1)):
        cur = None
        for k, f in enumerate(group):
            if k == 0:
                cur = [f]
                clusters.append(cur)
                continue
            near = any((f[0] - m[1] if sign > 0 else m[1] - f[0]) < thr for m in reversed(cur))
            if near:
                cur.append(f)
            else:
                cur = [f]
                clusters.append(cur)
    out = []
    for cl in clusters:
        cl = sorted(cl, key=lambda x: (x[2], x[3]))
        best, visited = None, set()
        for i, origin in enumerate(cl):
            if origin in visited:
                continue
            qs, qe, ss, se = origin
            length, n_ext = abs(qe - qs), 0
            visited.add(origin)
            for ext in cl[i + 1:]:
                if ext in visited or not ext[3] > se:
                    continue
                if qs < qe and ext[0] < ext[1]:
                    if ext[1] > qe:
                        if ext[0] - qe < thr and ext[2] - se < thr / 3:
                            qe, ss, se = ext[1], min(ss, ext[2]), ext[3]
                            length, n_ext = qe - qs, n_ext + 1
                            visited.add(ext)
                        elif ext[0] - qe >= thr:
                            break
                elif qs > qe and ext[0] > ext[1]:
                    if ext[1] < qe:
                        if qe - ext[0] < thr and ext[2] - se < thr / 3:
                            qe, ss, se = ext[1], min(ss, ext[2]), ext[3]
                            length, n_ext = qs - qe, n_ext + 1
                            visited.add(ext)
                        elif qe - ext[0] >= thr:
                            break
            if best is None or length > best[2]:
                best = (qs, qe, length, ss, se, se - ss, n_ext)
        if best is not None:
            out.append(best)
    return out


def _domain_overlap(pre, cur):
    """the overlap arithmetic of the table writer (Util.py:1226-1246), both intervals put in ascending order first"""
    ps, pe = (pre[0], pre[1]) if pre[0] <= pre[1] else (pre[1], pre[0])
    cs, ce = (cur[0], cur[1]) if cur[0] <= cur[1] else (cur[1], cur[0])
    if ps <= ce <= pe:
        return ce - ps if cs <= ps else ce - cs
    if ce > pe and ps <= cs <= pe:
        return pe - cs
    return 0


def blastx_domain_table(blastx_out, merge_distance=100):
    """the part of multiple_alignment_blastx_v1 (Util.py:1017-1262) behind the blastx call: `-outfmt 6` lines -> the rows of the
    domain table [(TE, protein, TE_start, TE_end, protein_start, protein_end)]: per (TE, protein) the chained fragments, per TE
    the chains by length (longest first), one dropped when more than half of it lies inside a longer one that stayed"""
    records = {}
    with open(blastx_out) as f:
        for line in f:
            parts = line.split("\t")
            if len(parts) < 10:
                continue
            records.setdefault(parts[0], {}).setdefault(parts[1], []).append((int(parts[6]), int(parts[7]), int(parts[8]), int(parts[9])))
    rows = []
    for te, subjects in records.items():
        chains = []
        for protein, frags in subjects.items():
            chains.extend(c + (protein,) for c in _chain_domain_fragments(frags, merge_distance))
        chains.sort(key=lambda x: -x[2])
        kept = []
        for c in chains:
            if all(not float(_domain_overlap(k_, c) / c[2]) > 0.5 for k_ in kept):
                kept.append(c)
        rows.extend((te, c[7], c[0], c[1], c[3], c[4]) for c in kept)
    return rows


def pet_partitions(items, partitions):
    """PET / divided_array (Util.py:1771-1798) on (name, sequence) pairs: longest first (stable), dealt to the partitions in rounds
    that take alternately from the front and from the back of that order"""
    order = sorted(items, key=lambda x: len(x[1]), reverse=True)
    parts = [[] for _ in range(partitions)]
    i, j, k, front = 0, len(order) - 1, 0, True
    while i <= j:
        if front:
            parts[k % partitions].append(order[i])
            i += 1
        else:
            parts[k % partitions].append(order[j])
            j -= 1
        k += 1
        if k % partitions == 0:
            front = not front
    return parts


_DOMAIN_SEARCH_MODES = ("gpu", "blastx")


def _domain_search_mode(search):
    """the switch of the domain search: the argument, then $HITE_DOMAIN_SEARCH, then None (blastx when it is installed)"""
    mode = search if search is not None else (os.environ.get("HITE_DOMAIN_SEARCH") or None)
    if mode is not None and mode not in _DOMAIN_SEARCH_MODES:
        raise ValueError("domain search %r: expected one of %s" % (mode, ", ".join(_DOMAIN_SEARCH_MODES)))
    return mode


def protein_search_outfmt6(query_path, lib_path, out_path, evalue=1e-20, ctx=None, protein_lib=None):
    """The build's own translated search where the reference runs `blastx -db <lib> -evalue 1e-20 -query <query> -outfmt 6`: writes
    the twelve columns qseqid sseqid pident length mismatch gapopen qstart qend sstart send evalue bitscore, one line per HSP (the
    definition: include/hite_gpu.h; minus-strand hits have qstart > qend as the tool prints them).  pident = 100 identical /
    columns; evalue = m n K exp(-lambda S) without length adjustment, bitscore = (lambda S - ln K) / ln 2 with lambda 0.267,
    K 0.041; mismatch and gapopen are written as 0: they are not computed, and neither the reference (Util.py:1025-1033) nor
    blastx_domain_table reads them.  protein_lib: a handle of ctx.protein_lib for this library (built here otherwise).
    -> the number of lines."""
    ctx = ctx or get_ctx()
    qnames, qseqs = read_fasta(query_path)
    pnames, pseqs = read_fasta(lib_path)
    own = protein_lib is None
    plib = ctx.protein_lib([pseqs[n] for n in pnames]) if own else protein_lib
    try:
        rec = ctx.protein_search([qseqs[n] for n in qnames], plib, evalue=evalue)
        n_res = plib.n_res
    finally:
        if own:
            plib.release()
    lam, k = 0.267, 0.041
    with open(out_path, "w") as f:
        for (q, p, _frame, qs, qe, ss, se, sc, idn, cols) in rec.tolist():
            ev = float(len(qseqs[qnames[q]]) // 3) * float(n_res) * k * math.exp(-lam * float(sc))
            f.write("%s\t%s\t%.3f\t%d\t0\t0\t%d\t%d\t%d\t%d\t%.2e\t%.1f\n" % (qnames[q], pnames[p], 100.0 * idn / cols, cols, qs, qe, ss, se, ev,
                                                                                  (lam * sc - math.log(k)) / math.log(2.0)))
    return len(rec)


def get_domain_info(cons, lib, output_table, threads, temp_dir, search=None, ctx=None):
    """get_domain_info (Util.py:4571-4612), same arguments: `blastx -evalue 1e-20 -outfmt 6` of the sequences of `cons`
    (in `threads` partitions dealt as the reference's PET deals them) against the protein library `lib`, the fragments chained per
    protein (blastx_domain_table), written as the reference's table: a header line, an empty line, then
    TE \t protein \t TE_start \t TE_end \t protein_start \t protein_end.  search: "gpu" = the build's own translated search
    (protein_search_outfmt6) writes the partitions' -outfmt 6 files, "blastx" = the external tool (NCBI BLAST+), None =
    $HITE_DOMAIN_SEARCH, else the external tool; without a search the table holds the header only and a warning says so.
    -> True when the search ran."""
    os.makedirs(temp_dir, exist_ok=True)
    names, contigs = read_fasta(cons)
    mode = _domain_search_mode(search)
    ran = False
    rows = []
    have_lib = lib is not None and os.path.exists(lib)
    if names and mode == "gpu" and have_lib:
        ctx = ctx or get_ctx()
        _pn, pseqs = read_fasta(lib)
        plib = ctx.protein_lib([pseqs[n] for n in _pn])
        try:
            for pi, part in enumerate(pet_partitions([(n, contigs[n]) for n in names], max(1, int(threads)))):
                if not part:
                    continue
                query, out = os.path.join(temp_dir, "%d.fa" % pi), os.path.join(temp_dir, "%d.out" % pi)
                store_fasta(dict(part), query)
                protein_search_outfmt6(query, lib, out, 1e-20, ctx=ctx, protein_lib=plib)
                rows.extend(blastx_domain_table(out, 100))
        finally:
            plib.release()
        ran = True
    elif names and mode != "gpu" and shutil.which("blastx") is not None and have_lib:
        if not all(os.path.exists(lib + ext) for ext in (".phr", ".pin", ".psq")) and shutil.which("makeblastdb"):
            subprocess.run("cd %s && makeblastdb -dbtype prot -in %s > /dev/null 2>&1" % (os.path.dirname(lib) or ".", lib), shell=True, check=False)
        for pi, part in enumerate(pet_partitions([(n, contigs[n]) for n in names], max(1, int(threads)))):
            if not part:
                continue
            query, out = os.path.join(temp_dir, "%d.fa" % pi), os.path.join(temp_dir, "%d.out" % pi)
            store_fasta(dict(part), query)
            subprocess.run("blastx -db %s -num_threads 1 -evalue 1e-20 -query %s -outfmt 6 > %s" % (lib, query, out), shell=True, check=False)
            if os.path.exists(out):        # (the reference concatenates the partitions' tables as they complete; here: in partition order)
                rows.extend(blastx_domain_table(out, 100))
        ran = True
    elif names:
        sys.stderr.write("[hite_amd] blastx or the protein library %s not found: no low-copy element is recalled by its protein domains "
                         "(HITE_DOMAIN_SEARCH=gpu / search=\"gpu\" runs the build's own search instead of blastx)\n" % lib)
    with open(output_table, "w") as f:
        f.write("TE_name\tdomain_name\tTE_start\tTE_end\tdomain_start\tdomain_end\n\n")
        for r in rows:
            f.write("\t".join(str(x) for x in r) + "\n")
    return ran


def intact_domain_names(output_table, protein_lib):
    """the decision of the domain recall (Util.py:8221-8234): TEs with a protein hit spanning >= 95 % of the protein"""
    _pn, proteins = read_fasta(protein_lib)
    keep = []
    with open(output_table) as f:
        for i, line in enumerate(f):
            if i < 2:
                continue
            parts = line.split("\t")
            if len(parts) < 6:
                continue
            if float(abs(int(parts[5]) - int(parts[4]))) / len(proteins[parts[1]]) >= 0.95 and parts[0] not in keep:
                keep.append(parts[0])
    return keep


_PROTEIN_LIB = {"tir": "TIRPeps.lib", "helitron": "HelitronPeps.lib", "non_ltr": "non_LTR.lib"}


def bucket_results(TE_type, results):
    """the collection loop of flank_region_align_v5 (Util.py:8159-8194, 8282-8287) on (cur_name, cur_seq, info, copy_count)
    tuples (cur_name None = not a TE): TIR / Helitron / non-LTR consensi that start with TG and end with CA are dropped (LTR
    ends), those with copy_count <= 5 (TIR, non-LTR) or <= 2 (Helitron) go to the low-copy bucket, the rest are real TEs.
    -> (true_tes, low_copy) in result order (the recall of low-copy elements follows in rescue_low_copy)."""
    true_tes, low_copy = {}, {}
    thr = 5 if TE_type in ("tir", "non_ltr") else 2
    for cur_name, cur_seq, _info, copy_count in results:
        if cur_name is None:
            continue
        if TE_type in ("tir", "helitron", "non_ltr"):
            if cur_seq.startswith("TG") and cur_seq.endswith("CA"):
                continue
            if copy_count <= thr:
                low_copy[cur_name] = cur_seq
            else:
                true_tes[cur_name] = cur_seq
        else:
            true_tes[cur_name] = cur_seq
    return true_tes, low_copy


def valid_filename(query_name):
    """Util.py:8127"""
    return re.sub(r'[<>:"/\\|?*]', "-", query_name)


# ---- Helitron candidate scan (multi_process_helitronscanner Util.py:263: HelitronScanner.jar scanHead / scanTail / pairends / draw) ----
_LCV_GAP = r"(?:\.\{(\d+)(?:,(\d+))?\})?"
_LCV_BODY = r"([ACGT](?:[ACGT.]*[ACGT])?)"
_LCV_RE = {"head": re.compile(r"^TC" + _LCV_GAP + _LCV_BODY + r"$"), "tail": re.compile(r"^" + _LCV_BODY + _LCV_GAP + r"CT\[AG\]\{2\}$")}


def parse_lcvs(lines, side):
    """HelitronScanner's LCV lines (TrainingSet/head.lcvs: side "head", tail.lcvs: side "tail") -> LCV_DTYPE records, the compiled
    patterns hite_helitron_scan takes (include/hite_gpu.h).  head: `TC`, an optional gap `.{n}` / `.{a,b}`, a body of letters ACGT and
    single `.` that starts and ends with a letter; tail: a body, an optional gap, `CT[AG]{2}`.  Blank lines and lines that start
    with # are skipped, a repeated line stays (each counts).  A line outside this grammar, a body of more than 32 positions or a gap
    of more than 63 raises ValueError naming the line."""
    from ._lib import HELITRON_MAX_BODY, HELITRON_MAX_GAP, LCV_DTYPE

    if side not in _LCV_RE:
        raise ValueError("parse_lcvs: side is 'head' or 'tail', not %r" % (side,))
    recs = []
    for no, raw in enumerate(lines, 1):
        line = raw.strip()
        if not line or line.startswith("#"):
            continue
        m = _LCV_RE[side].match(line)
        if not m:
            raise ValueError("parse_lcvs: line %d is no %s LCV pattern: %r" % (no, side, line))
        ga, gb, body = (m.group(1), m.group(2), m.group(3)) if side == "head" else (m.group(2), m.group(3), m.group(1))
        gmin = int(ga) if ga is not None else 0
        gmax = int(gb) if gb is not None else gmin
        if gmin > gmax or gmax > HELITRON_MAX_GAP:
            raise ValueError("parse_lcvs: line %d: gap %d..%d is descending or beyond %d: %r" % (no, gmin, gmax, HELITRON_MAX_GAP, line))
        if len(body) > HELITRON_MAX_BODY:
            raise ValueError("parse_lcvs: line %d: body of %d positions, the limit is %d: %r" % (no, len(body), HELITRON_MAX_BODY, line))
        bits = care = 0
        for j, ch in enumerate(body):
            if ch != ".":
                bits |= "ACGT".index(ch) << (2 * j)
                care |= 3 << (2 * j)
        recs.append((bits, care, gmin, gmax, len(body), (0,) * 5))
    return np.array(recs, dtype=LCV_DTYPE) if recs else np.zeros(0, dtype=LCV_DTYPE)


def lcv_line(rec, side):
    """the LCV line of a compiled record (a single gap prints as `.{n}`, none as nothing): parse_lcvs(lcv_line(r)) == r"""
    body = "".join("ACGT"[(int(rec["body"]) >> (2 * j)) & 3] if (int(rec["care"]) >> (2 * j)) & 3 else "." for j in range(int(rec["body_len"])))
    a, b = int(rec["gap_min"]), int(rec["gap_max"])
    gap = "" if a == b == 0 else (".{%d}" % a if a == b else ".{%d,%d}" % (a, b))
    return "TC" + gap + body if side == "head" else body + gap + "CT[AG]{2}"


def helitron_lcv_dir(HSDIR=None):
    """where head.lcvs and tail.lcvs are: --HSDIR, then $HITE_HSDIR, then <HiTE>/bin/HelitronScanner/TrainingSet beside the package (the
    reference's default, judge_Helitron_transposons.py:18).  The lists are HiTE's data; this build does not ship them.  -> the first
    of these directories that holds both files, or None."""
    beside = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bin", "HelitronScanner", "TrainingSet")
    for d in (HSDIR, os.environ.get("HITE_HSDIR"), beside):
        if d and os.path.isfile(os.path.join(d, "head.lcvs")) and os.path.isfile(os.path.join(d, "tail.lcvs")):
            return d
    return None


def multi_process_helitronscanner(candidate_file, output, sh_dir, temp_dir, HSDIR, HSJAR, threads, debug, ctx=None, device=0,
                                  head_threshold=1, tail_threshold=1, len_range=(200, 20000)):
    """multi_process_helitronscanner (Util.py:263-318; the reference runs bin/run_helitron_scanner.sh per 50 kb part: HelitronScanner's
    scanHead, scanTail, pairends and draw -pure_helitron on both strands, 30 minutes per part) as ONE batched call of the in-tree
    stage (Context.helitron_scan; the definition is in include/hite_gpu.h, parity with the tool is unpinned).  The thresholds and the
    length range are the tool's defaults, which the reference leaves alone.  Every record is written as the pure element -- its
    bases, reverse-complemented on the minus strand -- under the name <source name>_<start+1>_<end>_<+|->.  sh_dir, temp_dir, HSJAR,
    threads and debug are the reference's arguments and are not used.  -> the number of records."""
    lcv_dir = helitron_lcv_dir(HSDIR)
    if lcv_dir is None:
        raise FileNotFoundError("multi_process_helitronscanner: head.lcvs / tail.lcvs not found (HSDIR %r, $HITE_HSDIR, "
                                "<HiTE>/bin/HelitronScanner/TrainingSet)" % (HSDIR,))
    with open(os.path.join(lcv_dir, "head.lcvs")) as f:
        head = parse_lcvs(f, "head")
    with open(os.path.join(lcv_dir, "tail.lcvs")) as f:
        tail = parse_lcvs(f, "tail")
    names, contigs = read_fasta(candidate_file)
    rec = np.zeros((0, 6), dtype=np.int32)
    if names:
        rec = (ctx or get_ctx(device)).helitron_scan([contigs[n] for n in names], head, tail, head_threshold, tail_threshold, len_range)
    with open(output, "w") as f:
        for q, start, end, strand, _hs, _ts in rec.tolist():
            seq = contigs[names[q]][start:end]
            f.write(">%s_%d_%d_%s\n%s\n" % (names[q], start + 1, end, "-" if strand else "+", getReverseSequence(seq) if strand else seq))
    return len(rec)


# ---- FiLTR step 3: the flank filter of LTR terminal sequences (bin/FiLTR-main/src/LTR_filter.py:44-170) ---------------------------
# The three `cd-hit-est` calls of the step run as Context.frame_cluster (the definition is in include/hite_gpu.h, "clusters of a
# group of frames"; parity with the tool is unpinned), the copies come from the build's copy finder, the alignment from the star
# alignment, the frames and the frame vote from hite_ltr_both_ends / hite_ltr_frame.  ltr_flank_filter is the batched in-memory
# driver; the functions under the reference's names are wrappers over its parts that keep the `.matrix` directory contract.
LTR_SORT_OPTIONS = dict(ident=0.8, cov_short=0.3, cov_long=0.0, min_cov=20, min_len=10, both_strands=True)        # data_util.py:2883
LTR_JOINED_OPTIONS = dict(ident=0.95, cov_short=0.95, cov_long=0.95, min_cov=50, min_len=10, both_strands=True)   # Util.py:10947


def ltr_sort_rule(frames, left_clusters, right_clusters):
    """generate_sort_matrix (bin/FiLTR-main/utils/data_util.py:2833-2870) after its two clusterings: frames = the (left, right) rows
    of a `.matrix`, left_clusters / right_clusters = the clusters of the gap-free left / right frames (lists of row indices; rows of
    10 bases or fewer are in none).  -> the kept matrix, rewritten in the LEFT side's order (rows of clusters of several rows first,
    then the single rows, each in cluster order), or None when the candidate is dropped: a side with one row or none, or with too
    many homologous rows (0.8 of the rows under 20 rows, else 0.9)."""
    sides = []
    for clusters in (left_clusters, right_clusters):
        homo = [r for cl in clusters if len(cl) > 1 for r in cl]
        total = homo + [cl[0] for cl in clusters if len(cl) == 1]
        sides.append((homo, total, 0.8 if len(total) < 20 else 0.9))
    (lh, lt, l_thr), (rh, rt, r_thr) = sides
    if len(lt) > 1 and len(rt) > 1 and float(len(lh)) / len(lt) < l_thr and float(len(rh)) / len(rt) < r_thr:
        return [frames[r] for r in lt]
    return None


def ltr_flank_cluster_rule(clusters):
    """filter_ltr_by_flanking_cluster_sub (bin/FiLTR-main/src/Util.py:10966-10978) after its clustering of the joined frames: kept
    when fewer rows are in clusters of several rows than alone"""
    homo = sum(len(cl) for cl in clusters if len(cl) > 1)
    return not homo >= sum(1 for cl in clusters if len(cl) == 1)


def _ltr_clusters(cluster, groups, options, what):
    res = cluster(groups, **options)
    if any(r is None for r in res):
        raise ValueError("%s: a matrix beyond the limits of frame_cluster (HITE_FRAMECLUSTER_MAX_ROWS rows of HITE_FRAMECLUSTER_MAX_LEN bases)" % what)
    return res


def _ltr_sort_batch(mats, cluster, seconds=None):
    """the sort rule on a batch of matrices: TWO clustering calls, all left frames and all right frames"""
    t0 = time.perf_counter()
    left = _ltr_clusters(cluster, [[l.replace("-", "") for l, _r in m] for m in mats], LTR_SORT_OPTIONS, "sort_matrix_dir")
    t1 = time.perf_counter()
    right = _ltr_clusters(cluster, [[r.replace("-", "") for _l, r in m] for m in mats], LTR_SORT_OPTIONS, "sort_matrix_dir")
    if seconds is not None:
        seconds["cluster_left"] = t1 - t0
        seconds["cluster_right"] = time.perf_counter() - t1
    return [ltr_sort_rule(m, lc, rc) for m, lc, rc in zip(mats, left, right)]


def _ltr_joined_batch(mats, cluster, seconds=None):
    """the joined-flank rule on a batch of matrices: ONE clustering call"""
    t0 = time.perf_counter()
    res = _ltr_clusters(cluster, [[(l + r).replace("-", "").replace("\t", "") for l, r in m] for m in mats], LTR_JOINED_OPTIONS,
                        "filter_ltr_by_flanking_cluster")
    if seconds is not None:
        seconds["cluster_joined"] = time.perf_counter() - t0
    return [ltr_flank_cluster_rule(cl) for cl in res]


def _ltr_vote_batch(mats, flanking_len, window, frame_vote):
    """judge_both_ends_frame (bin/FiLTR-main/src/Util.py:10696-10709) on a batch: the frame vote on either side, one call per side;
    a matrix of one row or none passes (as judge_left_frame_LTR / judge_right_frame_LTR above)"""
    idx = [k for k, m in enumerate(mats) if len(m) > 1]
    ok = [True] * len(mats)
    for side, col in (("left", 0), ("right", 1)):
        votes = frame_vote([[row[col] for row in mats[k]] for k in idx], flanking_len, window, side) if idx else []
        for k, (is_ltr, _b) in zip(idx, votes):
            ok[k] = ok[k] and bool(is_ltr)
    return ok


# ---- the high-copy vote of FiLTR's hybrid CNN (bin/FiLTR-main/src/Deep_Learning; LTR_filter.py:146-170 runs it on every matrix of more
# than 5 rows, threshold 0.5) -- PINNED to the reference: Context.ltr_deep computes what include/hite_gpu.h defines ("high-copy LTR
# vote"), tests/golden/ltr_deep.json.gz holds the reference's features, logits and decisions.  The trained weights are FiLTR's data and
# are not shipped with the package (as head.lcvs is not): load_ltr_model finds them.  deep= replaces the device stage (the signature of
# Context.ltr_deep; the CPU tests pass the twin with the flat parameter array as the model).
def _ltr_model_spec():
    """(state-dict key, shape) of every parameter in the canonical order of include/hite_gpu.h"""
    bn = lambda key, c: [(key + "." + f, (c,)) for f in ("weight", "bias", "running_mean", "running_var")]  # noqa: E731
    spec = []
    for branch, c0 in (("model", 3), ("model_kmer", 2)):
        for k, (cin, cout) in enumerate(((c0, 8), (8, 16), (16, 32))):
            b = "%s.%d" % (branch, k)
            spec += [(b + ".conv1.weight", (cout, cin, 3, 3))] + bn(b + ".bn1", cout) + [(b + ".conv2.weight", (cout, cout, 3, 3))] + bn(b + ".bn2", cout)
            spec += [(b + ".shortcut.0.weight", (cout, cin, 1, 1))] + bn(b + ".shortcut.1", cout)
    spec += [("fc_layers.0.weight", (16, 64)), ("fc_layers.0.bias", (16,))] + bn("fc_layers.1", 16)
    spec += [("fc_layers.4.weight", (8, 16)), ("fc_layers.4.bias", (8,))] + bn("fc_layers.5", 8)
    spec += [("fc_layers.8.weight", (2, 8)), ("fc_layers.8.bias", (2,))]
    return spec


LTR_MODEL_PARAMS = 40026        # HITE_LTRDEEP_PARAMS


def ltr_model_params(state):
    """the canonical flat float32 array (LTR_MODEL_PARAMS values) from {key: array} with the keys of the reference's state dict (class
    CNNCAT; a `module.` prefix is stripped, the `num_batches_tracked` counters are not used); ValueError for a missing key or a wrong shape"""
    state = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in state.items()}
    parts = []
    for key, shape in _ltr_model_spec():
        if key not in state:
            raise ValueError("ltr_model_params: no %r in the state dict" % key)
        a = np.asarray(state[key], dtype=np.float32)
        if a.shape != shape:
            raise ValueError("ltr_model_params: %r has shape %r, not %r" % (key, a.shape, shape))
        parts.append(a.reshape(-1))
    flat = np.concatenate(parts)
    assert flat.size == LTR_MODEL_PARAMS
    return flat


def ltr_model_state(params):
    """the inverse of ltr_model_params: {key: float32 array} from the flat array"""
    params = np.asarray(params, dtype=np.float32).reshape(-1)
    if params.size != LTR_MODEL_PARAMS:
        raise ValueError("ltr_model_state: %d values, not %d" % (params.size, LTR_MODEL_PARAMS))
    state, at = {}, 0
    for key, shape in _ltr_model_spec():
        n = int(np.prod(shape))
        state[key] = params[at:at + n].reshape(shape)
        at += n
    return state


def _ltr_model_places(path=None):
    places = [path, os.environ.get("HITE_LTR_MODEL")]
    if os.environ.get("HITE_FILTR_DIR"):
        places.append(os.path.join(os.environ["HITE_FILTR_DIR"], "models", "production_model.pth"))
    return [p for p in places if p]


def load_ltr_model(path=None):
    """the flat parameter array of FiLTR's hybrid CNN from the first file that exists of: path, $HITE_LTR_MODEL,
    $HITE_FILTR_DIR/models/production_model.pth; a `.npy` file holds the flat array, anything else is a checkpoint of the reference
    (torch.load(..., weights_only=True)['model_state_dict']; torch is imported only then).  -> None when there is no such file."""
    for p in _ltr_model_places(path):
        if not os.path.isfile(p):
            continue
        if p.endswith(".npy"):
            flat = np.load(p).astype(np.float32).reshape(-1)
            if flat.size != LTR_MODEL_PARAMS:
                raise ValueError("load_ltr_model: %s holds %d values, not %d" % (p, flat.size, LTR_MODEL_PARAMS))
            return flat
        import torch

        ckpt = torch.load(p, map_location="cpu", weights_only=True)
        return ltr_model_params({k: v.numpy() for k, v in ckpt["model_state_dict"].items()})
    return None


def ltr_deep_probs(matrices, model, ctx=None, deep=None):
    """{name: probability of the LTR class} of the scored matrices of {name: rows}: ONE batched call of deep(model, matrices)
    (Context.ltr_deep; model is a handle of Context.ltr_model or the flat parameter array), then 1 / (1 + exp(l0 - l1)) in binary64"""
    names = list(matrices)
    if not names:
        return {}
    own = None
    if deep is None:
        ctx = ctx or get_ctx()
        deep = ctx.ltr_deep
        if isinstance(model, np.ndarray):
            model = own = ctx.ltr_model(model)
    try:
        logits, status = deep(model, [matrices[n] for n in names])
    finally:
        if own is not None:
            own.release()
    return {n: 1.0 / (1.0 + math.exp(float(l[0]) - float(l[1]))) for n, l, s in zip(names, np.asarray(logits, dtype=np.float64), status) if s == 0}


def ltr_deep_votes(matrices, model, threshold=0.5, ctx=None, deep=None):
    """hybridLTR_deep_main.py on {name: rows}: {name: 0 | 1} of the SCORED matrices only (5 .. 100 rows of 200 columns), 1 when the
    probability of the LTR class is above threshold (CNNPredictor.predict_and_save)"""
    return {n: 1 if p > threshold else 0 for n, p in ltr_deep_probs(matrices, model, ctx, deep).items()}


def alter_deep_learning_results(deep_table, homology_table, high_copy_names):
    """bin/FiLTR-main/src/Util.py:10711-10757 on dicts {name: 0 | 1}: both tables empty -> every high-copy name is 1; one empty -> the
    other; else the model's table with 0 written for every name the homology rule answers 0.  A name the homology rule passes and
    the model did not score is ABSENT from the result, as in the reference."""
    if not deep_table and not homology_table:
        return {n: 1 for n in high_copy_names}
    if not deep_table:
        return dict(homology_table)
    if not homology_table:
        return dict(deep_table)
    out = dict(deep_table)
    for n, is_ltr in homology_table.items():
        if not is_ltr:
            out[n] = is_ltr
    return out


def hybrid_ltr_deep(matrix_dir, model_path, output_dir, threshold=0.5, ctx=None, deep=None):
    """the directory contract of hybridLTR_deep_main.py: every `*.matrix` of matrix_dir (its name up to the first '.') is scored in ONE
    batched call; output_dir/is_LTR_deep.txt receives `name<TAB>0|1` and output_dir/deep_probs.csv `name<TAB>probability` of the
    scored matrices, in the order of the names.  -> {name: 0 | 1}"""
    model = load_ltr_model(model_path)
    if model is None:
        raise FileNotFoundError("hybrid_ltr_deep: no model at %r" % (model_path,))
    mats = {}
    for f in sorted(os.listdir(matrix_dir)):
        if f.endswith(".matrix"):
            with open(os.path.join(matrix_dir, f)) as fh:
                mats[f.split(".")[0]] = [line.replace("\t", "").strip() for line in fh]
    probs = ltr_deep_probs(mats, model, ctx, deep)
    os.makedirs(output_dir, exist_ok=True)
    votes = {n: 1 if p > threshold else 0 for n, p in probs.items()}
    with open(os.path.join(output_dir, "is_LTR_deep.txt"), "w") as f:
        for n, v in votes.items():
            f.write("%s\t%d\n" % (n, v))
    with open(os.path.join(output_dir, "deep_probs.csv"), "w") as f:
        for n, p in probs.items():
            f.write("%s\t%r\n" % (n, p))
    return votes


def _ltr_default_model(model):
    """model, or with HITE_LTR_DEEP=gpu what load_ltr_model finds (an error when it finds nothing)"""
    if model is None and os.environ.get("HITE_LTR_DEEP") == "gpu":
        model = load_ltr_model()
        if model is None:
            raise FileNotFoundError("HITE_LTR_DEEP=gpu and no model: searched $HITE_LTR_MODEL (%r) and $HITE_FILTR_DIR/models/production_model.pth "
                                    "($HITE_FILTR_DIR = %r); the path argument was not given" %
                                    (os.environ.get("HITE_LTR_MODEL"), os.environ.get("HITE_FILTR_DIR")))
    return model


def ltr_flank_decide(matrices, flanking_len=100, ctx=None, cluster=None, frame_vote=None, copy_num_threshold=5, sliding_window_size=20,
                     seconds=None, model=None, deep=None, threshold=0.5):
    """The decision rules of FiLTR's step 3 on `.matrix` contents, batched over all candidates: matrices = {name: [(left frame, right
    frame), ...]}.  In the reference's order: the sort rule (sort_matrix_dir), the joined-flank rule (filter_ltr_by_flanking_cluster),
    the split at copy_num_threshold rows (get_low_copy_LTR / get_high_copy_LTR; LTR_filter.py passes 5) and the frame vote on both
    sides (judge_ltr_from_both_ends_frame), merged as alter_deep_learning_results does.  Without a model (model=None and no
    HITE_LTR_DEEP=gpu) there is no deep-learning table: the homology rule alone.  With one (the flat parameter array or a handle of
    Context.ltr_model) the high-copy answers are alter_deep_learning_results(ltr_deep_votes(kept high-copy matrices), frame votes).
    cluster(groups, **options), frame_vote(matrices, flank, window, side) and deep(model, matrices) default to ctx.frame_cluster,
    ctx.ltr_frame and ctx.ltr_deep (the CPU suite passes the twins).
    -> ({name: (is_ltr, "low" | "high" | None, dropped_by)}, {name: kept matrix of every high-copy candidate}); dropped_by is None
    for a true LTR, else "sort", "flank_cluster", "frame_vote", "deep" (the model rejects what the homology rule passes) or
    "deep_missing" (the homology rule passes it and the model did not score it: absent from the reference's merged table)."""
    model = _ltr_default_model(model)
    if cluster is None or frame_vote is None or (model is not None and deep is None):
        ctx = ctx or get_ctx()
    cluster, frame_vote = cluster or ctx.frame_cluster, frame_vote or ctx.ltr_frame
    names = list(matrices)
    table = {}
    kept = _ltr_sort_batch([matrices[n] for n in names], cluster, seconds) if names else []
    table.update((n, (False, None, "sort")) for n, m in zip(names, kept) if m is None)
    names, mats = [n for n, m in zip(names, kept) if m is not None], [m for m in kept if m is not None]
    keep = _ltr_joined_batch(mats, cluster, seconds) if names else []
    table.update((n, (False, None, "flank_cluster")) for n, k in zip(names, keep) if not k)
    names, mats = [n for n, k in zip(names, keep) if k], [m for m, k in zip(mats, keep) if k]
    t0 = time.perf_counter()
    votes = _ltr_vote_batch(mats, flanking_len, sliding_window_size, frame_vote) if names else []
    if seconds is not None:
        seconds["frame_vote"] = time.perf_counter() - t0
    high = {}
    for n, m, ok in zip(names, mats, votes):
        label = "low" if len(m) <= copy_num_threshold else "high"
        table[n] = (bool(ok), label, None if ok else "frame_vote")
        if label == "high":
            high[n] = m
    if model is not None:
        t0 = time.perf_counter()
        homology = {n: int(table[n][0]) for n in high}
        merged = alter_deep_learning_results(ltr_deep_votes(high, model, threshold, ctx, deep), homology, list(high))
        for n in high:
            if n not in merged:
                table[n] = (False, "high", "deep_missing")
            elif homology[n] and not merged[n]:
                table[n] = (False, "high", "deep")
        if seconds is not None:
            seconds["deep"] = time.perf_counter() - t0
    return table, high


def ltr_terminal_frames(terminals, reference, flanking_len=100, max_copy_num=100, ctx=None, seconds=None):
    """generate_both_ends_frame_from_seq_minimap2 (bin/FiLTR-main/src/Util.py:956-1042) in memory, batched: terminals = {name:
    sequence}; the copies of every terminal sequence from the build's copy finder on the resident genome (where the reference runs
    minimap2; ctx, when given, holds `reference` packed in file order), the windows +- flanking_len (:978-1018: a window that leaves
    its contig or has fewer than 100 bases is skipped, the minus strand is reverse-complemented; when a candidate has windows of
    more than 1 000 bases only those are aligned, as their first 500 + last 500 bases), the first 100 members in copy order
    (extract_copies, :1305: the first max_num records of the file, not the longest), ONE star alignment and ONE frame call for all
    candidates; the anchor sequence is the first member without its flanks (generate_msa, :1315-1338).  max_copy_num is the
    reference's argument (its minimap2 -N is three times that; the copy finder keeps up to 300 copies) and steers nothing here.
    -> ({name: [(left frame, right frame), ...]}, {name: full-length rows}) for the candidates whose boundary was found."""
    t = [time.perf_counter()]
    lap = lambda key: (t.append(time.perf_counter()), seconds is not None and seconds.__setitem__(key, t[-1] - t[-2]))  # noqa: E731
    ctx = ctx or set_reference(reference)
    ref_names, ref_contigs = read_fasta(reference)
    names = list(terminals)
    tab = ctx.find_copies([terminals[n] for n in names]) if names else []
    lap("copies")
    q_names, groups, anchors = [], [], []
    for n, copies in zip(names, tab):
        extend, trunc = {}, {}
        for contig, start1, end1, minus, _anchors in copies:
            seq = ref_contigs[ref_names[contig]]
            if start1 - 1 - flanking_len < 0 or end1 + flanking_len > len(seq):
                continue
            win = seq[start1 - 1 - flanking_len:end1 + flanking_len]
            if minus:
                win = getReverseSequence(win)
            if len(win) < 100:
                continue
            key = (contig, start1, end1, bool(minus))
            extend[key] = win
            if len(win) > 1000:
                trunc[key] = win[:500] + win[-500:]
        members = list((trunc or extend).values())[:100]
        if members:
            q_names.append(n)
            groups.append(members)
            anchors.append(members[0][flanking_len:-flanking_len])
    lap("windows")
    msas = ctx.star_msa(groups) if groups else []
    lap("msa")
    ok = [k for k, m in enumerate(msas) if m is not None]
    ends = ctx.ltr_both_ends([[bytes(r) for r in msas[k]] for k in ok], [anchors[k] for k in ok], flanking_len) if ok else []
    lap("both_ends")
    frames, full = {}, {}
    for k, res in zip(ok, ends):
        if res is not None:
            frames[q_names[k]], full[q_names[k]] = res[0], res[1]
    return frames, full


def ltr_flank_filter(terminals, reference, flanking_len=100, max_copy_num=100, ctx=None, cluster=None, frame_vote=None, seconds=None,
                     model=None, deep=None, threshold=0.5):
    """FiLTR's "Step 3: filter out false positive sequences based on the flanking regions of the terminal sequences"
    (bin/FiLTR-main/src/LTR_filter.py:44-170) for a set of LTR terminal sequences (a FASTA path or {name: sequence}) against
    `reference`: ltr_terminal_frames, then ltr_flank_decide (model / deep / threshold: its high-copy vote of the hybrid CNN; without
    a model the homology rule alone).  A true LTR is a candidate whose copies' flanks are mostly not alike.  seconds: a dict that
    receives the wall seconds of every step.
    -> ({name: (is_ltr, "low" | "high" | None, dropped_by)}, {name: kept high-copy matrix}); dropped_by "frames" = no copy window
    or no boundary in the alignment (the reference writes no `.matrix` for such a candidate), else as ltr_flank_decide."""
    if not isinstance(terminals, dict):
        t_names, t_contigs = read_fasta(terminals)
        terminals = {n: t_contigs[n] for n in t_names}
    frames, _full = ltr_terminal_frames(terminals, reference, flanking_len, max_copy_num, ctx, seconds)
    table, high = ltr_flank_decide(frames, flanking_len, ctx or get_ctx(), cluster, frame_vote, seconds=seconds, model=model, deep=deep,
                                   threshold=threshold)
    return {n: table.get(n, (False, None, "frames")) for n in terminals}, high


def _read_matrix_dir(matrix_dir):
    """{name: [(left, right), ...]} of every `.matrix` under matrix_dir (find_files_recursively), by path"""
    out = {}
    for root, _dirs, files in sorted(os.walk(matrix_dir)):
        for f in sorted(files):
            if f.endswith(".matrix"):
                with open(os.path.join(root, f)) as fh:
                    out[f.split(".")[0]] = [tuple((line.replace("\n", "").split("\t") + [""])[:2]) for line in fh]
    return out


def _write_matrix(path, rows):
    with open(path, "w") as f:
        for left, right in rows:
            f.write(left + "\t" + right + "\n")


def generate_both_ends_frame_from_seq_minimap2(candidate_sequence_path, reference, flanking_len, threads, temp_dir, output_dir,
                                               full_length_output_dir, max_copy_num, ctx=None):
    """bin/FiLTR-main/src/Util.py:956: <output_dir>/<name>.matrix and <full_length_output_dir>/<name>.matrix of every terminal
    sequence with a boundary, from ONE batched call (ltr_terminal_frames); threads and temp_dir have nothing to steer here"""
    for d in (output_dir, full_length_output_dir):
        if os.path.exists(d):
            shutil.rmtree(d)
        os.makedirs(d, exist_ok=True)
    names, contigs = read_fasta(candidate_sequence_path)
    frames, full = ltr_terminal_frames({n: contigs[n] for n in names}, reference, flanking_len, max_copy_num, ctx)
    for n, rows in frames.items():
        _write_matrix(os.path.join(output_dir, n + ".matrix"), rows)
        with open(os.path.join(full_length_output_dir, n + ".matrix"), "w") as f:
            for row in full[n]:
                f.write(row + "\n")


def sort_matrix_dir(source_dir, target_dir, temp_dir, threads, ctx=None, cluster=None):
    """bin/FiLTR-main/utils/data_util.py:2792: the kept matrices of source_dir, rewritten, in target_dir -> (input_num, keep_num)"""
    os.makedirs(target_dir, exist_ok=True)
    mats = _read_matrix_dir(source_dir)
    kept = _ltr_sort_batch(list(mats.values()), cluster or (ctx or get_ctx()).frame_cluster) if mats else []
    for n, rows in zip(mats, kept):
        if rows is not None:
            _write_matrix(os.path.join(target_dir, n + ".matrix"), rows)
    return len(mats), sum(1 for rows in kept if rows is not None)


def filter_ltr_by_flanking_cluster(output_dir, target_dir, temp_dir, threads, log, ctx=None, cluster=None):
    """bin/FiLTR-main/src/Util.py:10985: the matrices of output_dir that pass the joined-flank rule are copied to target_dir"""
    shutil.rmtree(target_dir, ignore_errors=True)
    os.makedirs(target_dir, exist_ok=True)
    mats = _read_matrix_dir(output_dir)
    keep = _ltr_joined_batch(list(mats.values()), cluster or (ctx or get_ctx()).frame_cluster) if mats else []
    for (n, rows), k in zip(mats.items(), keep):
        if k:
            _write_matrix(os.path.join(target_dir, n + ".matrix"), rows)
    if log is not None:
        log.logger.debug("Input LTR num: " + str(len(mats)) + ", keep LTR num: " + str(sum(keep)))


def _copy_matrices_by_rows(output_dir, target_dir, want):
    shutil.rmtree(target_dir, ignore_errors=True)
    os.makedirs(target_dir)
    for name in sorted(os.listdir(output_dir)):
        path = os.path.join(output_dir, name)
        with open(path) as f:
            rows = sum(1 for _line in f)
        if want(rows):
            shutil.copy(path, target_dir)


def get_low_copy_LTR(output_dir, low_copy_output_dir, threads, copy_num_threshold=3):
    """bin/FiLTR-main/src/Util.py:10368: the matrices of at most copy_num_threshold rows"""
    _copy_matrices_by_rows(output_dir, low_copy_output_dir, lambda rows: rows <= copy_num_threshold)


def get_high_copy_LTR(output_dir, high_copy_output_dir, threads, copy_num_threshold=3):
    """bin/FiLTR-main/src/Util.py:10406: the matrices of more than copy_num_threshold rows"""
    _copy_matrices_by_rows(output_dir, high_copy_output_dir, lambda rows: rows > copy_num_threshold)


def judge_ltr_from_both_ends_frame(output_dir, output_path, threads, type, flanking_len, log, sliding_window_size=20, ctx=None,
                                   frame_vote=None):
    """bin/FiLTR-main/src/Util.py:10477: 'name\\t0|1' per matrix of output_dir, from two batched frame votes"""
    mats = _read_matrix_dir(output_dir)
    votes = _ltr_vote_batch(list(mats.values()), flanking_len, sliding_window_size, frame_vote or (ctx or get_ctx()).ltr_frame) if mats else []
    if log is not None:
        log.logger.debug(type + " LTR num: " + str(len(mats)) + ", LTR Homo filter LTR num: " + str(len(votes) - sum(votes)) +
                         ", remain LTR num: " + str(sum(votes)))
    with open(output_path, "w") as f_save:
        for n, ok in zip(mats, votes):
            f_save.write(n + "\t" + str(1 if ok else 0) + "\n")


# ---- FiLTR steps 1 and 2: the filters on the lines of the `.scn` candidate table (bin/FiLTR-main/src/LTR_filter.py:542-589) -------
# Where the reference writes two FASTA files and starts one `blastn -query .. -subject .. -outfmt 6` process per candidate line, every
# function here makes ONE batched call of Context.pair_hsps (the definition is in include/hite_gpu.h, "local alignments of pairs of
# intervals"; parity with blastn is unpinned: plus strand only, no e-value, bands of 192 diagonals, no X-drop).  The rules around the
# search are the reference's.  hsps= replaces the search (the signature of Context.pair_hsps; the CPU tests pass the twin).  A pair
# the search refuses (an interval beyond HITE_PAIRHSP_MAX_LEN) is treated as the reference treats a failed blastn process.
def _scn_log(log, level, msg):
    if log is not None:
        getattr(log.logger, level)(msg)


def _py_slice(seq_len, start, stop):
    """the interval seq[start:stop] covers, as Python slices (a negative index counts from the end): (begin, end), end >= begin"""
    a, b, _ = slice(start, stop).indices(seq_len)
    return a, max(a, b)


def _contig_ids(ref_contigs):
    names = list(ref_contigs)
    return [ref_contigs[n] for n in names], {n: k for k, n in enumerate(names)}


def read_scn(scn_file, log, remove_dup=False):
    """bin/FiLTR-main/src/Util.py:182 -> ({index: (chr_name, left_ltr_start, left_ltr_end, right_ltr_start, right_ltr_end)}, {index:
    line}); remove_dup drops a line whose (parts[0], parts[1], chr_name) was seen before"""
    ltr_candidates, ltr_lines = {}, {}
    existing_records = set()
    remove_count = total_lines = candidate_index = 0
    with open(scn_file, "r") as f_r:
        for line in f_r:
            if line.startswith("#") or line.strip() == "":
                continue
            line = line.replace("\n", "")
            parts = line.split(" ")
            chr_name = parts[11]
            total_lines += 1
            if remove_dup:
                cur_record = (int(parts[0]), int(parts[1]), chr_name)
                if cur_record in existing_records:
                    remove_count += 1
                    continue
                existing_records.add(cur_record)
            ltr_candidates[candidate_index] = (chr_name, int(parts[3]), int(parts[4]), int(parts[6]), int(parts[7]))
            ltr_lines[candidate_index] = line
            candidate_index += 1
    if remove_dup:
        _scn_log(log, "debug", "Total LTR num: " + str(total_lines))
        _scn_log(log, "debug", "Remove " + str(remove_count) + " replicate LTR in scn file, remaining LTR num: " + str(len(ltr_candidates)))
    return ltr_candidates, ltr_lines


def store_scn(confident_lines, confident_scn):
    """bin/FiLTR-main/src/Util.py:219"""
    with open(confident_scn, "w") as f_save:
        for line in confident_lines:
            f_save.write(line + "\n")


def get_recombination_ltr(ltr_candidates, ref_contigs, threads, temp_dir, log, ctx=None, hsps=None):
    """FiLTR step 1a (bin/FiLTR-main/src/Util.py:7099, is_recombination :5923): the left terminal against the candidate's own
    internal sequence ref_seq[left_ltr_end : right_ltr_start - 1]; a candidate is recombinant when some HSP covers 95 % of the
    terminal ((q_end - q_start + 1) / query_len >= 0.95).  One batched search; threads and temp_dir are the reference's arguments
    and steer nothing.  -> the recombinant candidate indices, in candidate order (the reference's order is that of its processes)"""
    _scn_log(log, "info", "Start get recombination ltr")
    seqs, ids = _contig_ids(ref_contigs)
    jobs, pairs = [], []
    for candidate_index, (chr_name, left_ltr_start, left_ltr_end, right_ltr_start, _right_ltr_end) in ltr_candidates.items():
        if chr_name not in ref_contigs:
            raise ValueError("Chromosome names in the SCN file do not match the input genome names: " + chr_name)
        n = len(ref_contigs[chr_name])
        q0, q1 = _py_slice(n, left_ltr_start - 1, left_ltr_end)
        s0, s1 = _py_slice(n, left_ltr_end, right_ltr_start - 1)
        if q1 > q0 and s1 > s0:
            jobs.append((candidate_index, q1 - q0))
            pairs.append((ids[chr_name], q0, q1, ids[chr_name], s0, s1))
    res = (hsps or (ctx or get_ctx()).pair_hsps)(seqs, pairs) if pairs else []
    refused = sum(r is None for r in res)
    if refused:
        _scn_log(log, "debug", "get_recombination_ltr: " + str(refused) + " pairs beyond the limits of the search, taken as not recombinant")
    return [ci for (ci, query_len), r in zip(jobs, res) if r is not None and any((abs(h[1] - h[0]) + 1) / query_len >= 0.95 for h in r)]


def blast6_identity(matches, columns):
    """the third column of a blast6 line as the reference parses it: percent identity with three decimals"""
    return float("%.3f" % (100.0 * matches / columns))


def ltr_lines_from_hsps(line, lLTR_end, chr_name, seq_id, hsp_list):
    """get_ltr_from_line (bin/FiLTR-main/src/Util.py:11170-11223) after its search: the candidate's line and one new line per direct
    repeat inside its internal sequence (identity > 95, both sides > 300 bases, more than 500 apart), then the redundancy pass"""
    new_lines = [line.split(" ")]
    for q_start, q_end, s_start, s_end, _score, matches, columns in hsp_list:
        q_len, s_len = abs(q_end - q_start), abs(s_end - s_start)
        identity = blast6_identity(matches, columns)
        if identity > 95 and q_len > 300 and s_len > 300 and q_end > q_start and s_end > s_start and s_start - q_end > 500:
            new_lLTR_start, new_lLTR_end = lLTR_end + q_start, lLTR_end + q_end
            new_rLTR_start, new_rLTR_end = lLTR_end + s_start, lLTR_end + s_end
            new_lines.append([new_lLTR_start, new_rLTR_end, new_rLTR_end - new_lLTR_start + 1,
                              new_lLTR_start, new_lLTR_end, new_lLTR_end - new_lLTR_start + 1,
                              new_rLTR_start, new_rLTR_end, new_rLTR_end - new_rLTR_start + 1, identity, seq_id, chr_name])
    new_lines.sort(key=lambda x: (int(x[0]), -int(x[1])))
    filtered_new_lines = []
    for i in range(len(new_lines) - 1, -1, -1):
        cur_item = new_lines[i]
        cur_lLTR_start, cur_rLTR_end, cur_LTR_len = int(cur_item[0]), int(cur_item[1]), int(cur_item[2])
        is_redundant = False
        for j in range(i - 1, -1, -1):
            next_item = new_lines[j]
            overlap_length = min(cur_rLTR_end, int(next_item[1])) - max(cur_lLTR_start, int(next_item[0])) + 1
            if overlap_length >= 0.95 * cur_LTR_len and overlap_length >= 0.95 * int(next_item[2]):
                is_redundant = True
                break
        if not is_redundant:
            filtered_new_lines.append(cur_item)
    return [" ".join(map(str, x)) for x in reversed(filtered_new_lines)]


def get_all_potential_ltr_lines(confident_lines, reference, threads, temp_path, temp_dir, log, ctx=None, hsps=None):
    """FiLTR step 1b (bin/FiLTR-main/src/Util.py:11227, get_ltr_from_line :11149): the internal sequence ref_seq[lLTR_end :
    rLTR_start] of every line against itself (diag_min = 500: only what lies more than 500 diagonals off the main one can pass the
    reference's `s_start - q_end > 500`); direct repeats inside it become further candidate lines.  reference: a FASTA path or
    {name: sequence}.  A line with an empty internal sequence, or whose search is refused, gives no line at all (the reference has no
    entry for it).  Writes the JSON side file temp_path as the reference does.  -> the lines, in line order"""
    _scn_log(log, "info", "Start get all potential ltr lines")
    ref_contigs = reference if isinstance(reference, dict) else read_fasta(reference)[1]
    seqs, ids = _contig_ids(ref_contigs)
    jobs, pairs = [], []
    for cur_line in confident_lines:
        parts = cur_line.split(" ")
        chr_name, seq_id, lLTR_end, rLTR_start = parts[11], parts[10], int(parts[4]), int(parts[6])
        s0, s1 = _py_slice(len(ref_contigs[chr_name]), lLTR_end, rLTR_start)
        if s1 > s0:
            jobs.append((lLTR_end, chr_name, seq_id, cur_line))
            pairs.append((ids[chr_name], s0, s1, ids[chr_name], s0, s1))
    res = (hsps or (ctx or get_ctx()).pair_hsps)(seqs, pairs, diag_min=500) if pairs else []
    refused = sum(r is None for r in res)
    if refused:
        _scn_log(log, "debug", "get_all_potential_ltr_lines: " + str(refused) + " internal sequences beyond the limits of the search, their lines are dropped")
    all_lines = {}
    for candidate_index, ((lLTR_end, chr_name, seq_id, cur_line), r) in enumerate(zip(jobs, res)):
        if r is not None:
            all_lines[candidate_index] = ltr_lines_from_hsps(cur_line, lLTR_end, chr_name, seq_id, r)
    temp_lines = {ci: lines for ci, lines in all_lines.items() if len(lines) > 1}
    with open(temp_path, "w", encoding="utf-8") as f:
        json.dump(temp_lines, f, ensure_ascii=False, indent=4)
    new_confident_lines = [cur_line for lines in all_lines.values() for cur_line in lines]
    _scn_log(log, "info", "Find all potential LTR, raw ltr num:" + str(len(confident_lines)) + ", current ltr num:" + str(len(new_confident_lines)))
    return new_confident_lines


def remove_dirty_LTR(confident_lines, log):
    """bin/FiLTR-main/src/Util.py:7140 (host only): {chr-start-end: 1} of the lines whose internal sequence holds a whole later
    candidate of the same chromosome (both its left start and its right end strictly inside)"""
    _scn_log(log, "info", "Start remove dirty LTR")
    dirty_dicts = {}
    rows = []
    for cur_line in confident_lines:
        parts = cur_line.split(" ")
        rows.append((parts[11], int(parts[3]), int(parts[4]), int(parts[6]), int(parts[7])))
    for i, (cur_chr, cur_ls, cur_le, cur_rs, cur_re) in enumerate(rows):
        for next_chr, next_ls, _next_le, _next_rs, next_re in rows[i + 1:]:
            if cur_chr != next_chr:
                break
            if cur_le < next_ls < cur_rs and cur_le < next_re < cur_rs:
                dirty_dicts[cur_chr + "-" + str(cur_ls) + "-" + str(cur_le)] = 1
                break
            if next_ls > cur_re:
                break
    return dirty_dicts


def merge_intervals(intervals):
    """bin/FiLTR-main/src/Util.py:4181: sorts `intervals` in place by start and joins those that touch or overlap"""
    if not intervals:
        return []
    intervals.sort(key=lambda x: x[0])
    merged = [intervals[0]]
    for current in intervals:
        last = merged[-1]
        if current[0] <= last[1]:
            merged[-1] = (last[0], max(last[1], current[1]))
        else:
            merged.append(current)
    return merged


def judge_flank_hsps(hsp_list, lLTR_len, rLTR_len, lLTR_start, lLTR_end, rLTR_start, rLTR_end, extend_len=50, error_region_len=10):
    """judge_scn_line_by_flank_seq_v2 (bin/FiLTR-main/src/Util.py:10783-10836) after its search of the left terminal +- extend_len
    against the right one: an alignment that begins within error_region_len of both left boundaries, or ends within it of both right
    boundaries, is a boundary alignment; the candidate is an LTR when the merged boundary alignments cover 90 % of the left terminal.
    -> (is_ltr, None or the adjusted (lLTR_start, lLTR_end, rLTR_start, rLTR_end))"""
    q_start_offset = q_end_offset = s_start_offset = s_end_offset = 0
    precise_boundary_alignments = []
    for q_start, q_end, s_start, s_end in (h[:4] for h in hsp_list):
        if ((extend_len - error_region_len) <= q_start <= (extend_len + error_region_len)
                and q_end <= (extend_len + lLTR_len + error_region_len)
                and (extend_len - error_region_len) <= s_start <= (extend_len + error_region_len)
                and s_end <= (extend_len + rLTR_len + error_region_len)):
            q_start_offset = q_start - extend_len
            s_start_offset = s_start - extend_len
            precise_boundary_alignments.append((q_start, q_end))
        if ((extend_len - error_region_len) <= q_start
                and (extend_len + lLTR_len - error_region_len) <= q_end <= (extend_len + lLTR_len + error_region_len)
                and (extend_len - error_region_len) <= s_start
                and (extend_len + rLTR_len - error_region_len) <= s_end <= (extend_len + rLTR_len + error_region_len)):
            q_end_offset = q_end + 1 - (lLTR_len + extend_len)
            s_end_offset = s_end + 1 - (rLTR_len + extend_len)
            precise_boundary_alignments.append((q_start, q_end))
    cover_len = sum(end - start for start, end in merge_intervals(precise_boundary_alignments))
    if float(cover_len) / lLTR_len >= 0.9:
        adjusted = (lLTR_start + q_start_offset, lLTR_end + q_end_offset, rLTR_start + s_start_offset, rLTR_end + s_end_offset)
        moved = q_start_offset != 0 or q_end_offset != 0 or s_start_offset != 0 or s_end_offset != 0
        return 1, adjusted if moved else None
    return 0, None


def filter_ltr_by_flank_seq_v2(scn_file, filter_scn, reference, threads, temp_dir, log, ctx=None, hsps=None):
    """FiLTR step 2 (bin/FiLTR-main/src/Util.py:10839): the left terminal +- 50 bases of every line of scn_file against the right
    one; judge_flank_hsps decides, and a line whose boundary moved is followed by its adjusted copy.  reference: a FASTA path or
    {name: sequence}.  A line whose windows are empty, or whose search is refused, has no result and is not kept.  Writes
    filter_scn; -> its lines"""
    ref_contigs = reference if isinstance(reference, dict) else read_fasta(reference)[1]
    _ltr_candidates, ltr_lines = read_scn(scn_file, log)
    seqs, ids = _contig_ids(ref_contigs)
    extend_len = 50
    jobs, pairs = [], []
    for candidate_index, line in ltr_lines.items():
        parts = line.split(" ")
        chr_name = parts[11]
        n = len(ref_contigs[chr_name])
        lLTR_start, lLTR_end, lLTR_len = int(parts[3]), int(parts[4]), int(parts[5])
        rLTR_start, rLTR_end, rLTR_len = int(parts[6]), int(parts[7]), int(parts[8])
        q0, q1 = _py_slice(n, lLTR_start - extend_len, lLTR_end + extend_len)
        s0, s1 = _py_slice(n, rLTR_start - extend_len, rLTR_end + extend_len)
        if q1 > q0 and s1 > s0:
            jobs.append((candidate_index, lLTR_len, rLTR_len, lLTR_start, lLTR_end, rLTR_start, rLTR_end))
            pairs.append((ids[chr_name], q0, q1, ids[chr_name], s0, s1))
    res = (hsps or (ctx or get_ctx()).pair_hsps)(seqs, pairs) if pairs else []
    refused = sum(r is None for r in res)
    if refused:
        _scn_log(log, "debug", "filter_ltr_by_flank_seq_v2: " + str(refused) + " pairs beyond the limits of the search, their lines are not kept")
    confident_lines = []
    fp_count = 0
    for job, r in zip(jobs, res):
        if r is None:
            continue
        is_ltr, adjust_boundary = judge_flank_hsps(r, *job[1:])
        if is_ltr == 0:
            fp_count += 1
            continue
        line = ltr_lines[job[0]]
        confident_lines.append(line)
        if adjust_boundary is not None:
            parts = line.split(" ")
            parts[3], parts[4] = str(adjust_boundary[0]), str(adjust_boundary[1])
            parts[5] = str(adjust_boundary[1] - adjust_boundary[0] + 1)
            parts[6], parts[7] = str(adjust_boundary[2]), str(adjust_boundary[3])
            parts[8] = str(adjust_boundary[3] - adjust_boundary[2] + 1)
            confident_lines.append(" ".join(parts))
    store_scn(confident_lines, filter_scn)
    _scn_log(log, "debug", "Remove False Positive LTR terminal: " + str(fp_count) + ", remaining LTR num: " + str(len(confident_lines)))
    return confident_lines


def left_ltr_terminals(scn_file, ref_contigs, log=None):
    """bin/FiLTR-main/src/LTR_filter.py:594-615: {chr-start-end: left terminal sequence} of the lines of scn_file (a name seen before
    gets -rep1, -rep2, ...; a terminal of N only is left out) and {name: candidate index}"""
    ltr_candidates, _ltr_lines = read_scn(scn_file, log)
    left_LTR_contigs, leftLtr2Candidates = {}, {}
    for candidate_index, (chr_name, left_ltr_start, left_ltr_end, _rs, _re) in ltr_candidates.items():
        if chr_name not in ref_contigs:
            raise ValueError("Chromosome names in the SCN file do not match the input genome names: " + chr_name)
        left_ltr_name = original_name = chr_name + "-" + str(left_ltr_start) + "-" + str(left_ltr_end)
        left_ltr_seq = ref_contigs[chr_name][left_ltr_start - 1: left_ltr_end]
        if all(char == "N" for char in left_ltr_seq):
            continue
        counter = 1
        while left_ltr_name in left_LTR_contigs:
            left_ltr_name = "%s-rep%d" % (original_name, counter)
            counter += 1
        left_LTR_contigs[left_ltr_name] = left_ltr_seq
        leftLtr2Candidates[left_ltr_name] = candidate_index
    return left_LTR_contigs, leftLtr2Candidates


def ltr_scn_filter(scn_file, reference, out_dir, ctx=None, hsps=None, seconds=None, log=None):
    """FiLTR from the `.scn` candidate table to the left terminal sequences (bin/FiLTR-main/src/LTR_filter.py:542-615): step 1
    (get_recombination_ltr, get_all_potential_ltr_lines, remove_dirty_LTR -> out_dir/remove_recomb.scn) and step 2
    (filter_ltr_by_flank_seq_v2 -> out_dir/filter_terminal_align.scn), three batched searches in all.  seconds: a dict that receives
    the wall seconds of `recombination`, `potential_lines`, `flank_align`.
    -> (path of the final scn, dirty_dicts, {chr-start-end: left terminal sequence}); the third value is what ltr_flank_filter takes"""
    t = [time.perf_counter()]
    lap = lambda key: (t.append(time.perf_counter()), seconds is not None and seconds.__setitem__(key, t[-1] - t[-2]))  # noqa: E731
    os.makedirs(out_dir, exist_ok=True)
    hsps = hsps or (ctx or get_ctx()).pair_hsps
    _ref_names, ref_contigs = read_fasta(reference)
    ltr_candidates, ltr_lines = read_scn(scn_file, log, remove_dup=True)
    lap("read")
    recombination_candidates = set(get_recombination_ltr(ltr_candidates, ref_contigs, 1, out_dir, log, hsps=hsps))
    confident_lines = [ltr_lines[ci] for ci in ltr_candidates if ci not in recombination_candidates]
    lap("recombination")
    confident_lines = get_all_potential_ltr_lines(confident_lines, ref_contigs, 1, os.path.join(out_dir, "all_potential_ltr.json"), out_dir, log,
                                                  hsps=hsps)
    dirty_dicts = remove_dirty_LTR(confident_lines, log)
    remove_recomb_scn = os.path.join(out_dir, "remove_recomb.scn")
    store_scn(confident_lines, remove_recomb_scn)
    lap("potential_lines")
    filter_terminal_align_scn = os.path.join(out_dir, "filter_terminal_align.scn")
    filter_ltr_by_flank_seq_v2(remove_recomb_scn, filter_terminal_align_scn, ref_contigs, 1, out_dir, log, hsps=hsps)
    lap("flank_align")
    left_LTR_contigs, _map = left_ltr_terminals(filter_terminal_align_scn, ref_contigs, log)
    return filter_terminal_align_scn, dirty_dicts, left_LTR_contigs


# ---- the LTR candidate table itself (where FiLTR runs LtrDetector: main.py:135-156; HiTE's other branch gt ltrharvest + LTR_FINDER) --
# In-tree stage, PARITY UNPINNED against the three tools: what is computed is the "LTR candidate scan" of include/hite_gpu.h
# (Context.ltr_scan), held to its CPU twin.  scan= replaces the scan (the signature of Context.ltr_scan; the CPU tests pass the twin).
def ltr_scn_lines(records, names):
    """the candidate lines of scan records (seq, ls, le, rs, re, score, matches, columns; 0-based, half-open): the twelve
    space-separated fields the reference's convert_LtrDetector_scn writes (bin/FiLTR-main/src/Util.py:9131) -- start, end and length
    of the element, of the left and of the right terminal (1-based, inclusive), the identity of the terminals (100 * matches /
    columns, two decimals), `NA` as seq_id, the chromosome name"""
    lines = []
    for seq, ls, le, rs, re_, _score, matches, columns in records:
        fields = (ls + 1, re_, re_ - ls, ls + 1, le, le - ls, rs + 1, re_, re_ - rs, "%.2f" % (100.0 * matches / columns), "NA", names[seq])
        lines.append(" ".join(str(x) for x in fields))
    return lines


def ltr_candidate_scan(reference, scn_file, ctx=None, scan=None, **limits):
    """genome in, `.scn` candidate table out: reference is a FASTA path or {name: sequence}; the scan (Context.ltr_scan, or scan=) runs
    on all sequences in one call with LtrDetector's default limits unless given (min_len, max_len, min_ltr, max_ltr, identity; also
    stats=, cap=); scn_file receives a `#` header line and one line per record (ltr_scn_lines), in the order of the records: by
    chromosome in the order of the reference, then by start.  -> the lines"""
    if isinstance(reference, dict):
        names, contigs = list(reference), reference
    else:
        names, contigs = read_fasta(reference)
    scan = scan or (ctx or get_ctx()).ltr_scan
    records = scan([contigs[n] for n in names], **limits)
    lines = ltr_scn_lines([[int(v) for v in r] for r in records], names)
    with open(scn_file, "w") as f_save:
        f_save.write("# hite_ltr_scan: start end len lLTR_start lLTR_end lLTR_len rLTR_start rLTR_end rLTR_len similarity seq_id chr\n")
        for line in lines:
            f_save.write(line + "\n")
    return lines


def ltr_detect(reference, out_dir, flanking_len=100, max_copy_num=100, ctx=None, scan=None, hsps=None, cluster=None, frame_vote=None,
               seconds=None, model=None, deep=None, threshold=0.5):
    """FiLTR from the genome to the is_LTR table, in-tree: ltr_candidate_scan -> out_dir/total.scn, ltr_scn_filter (steps 1 and 2) ->
    out_dir/filter_terminal_align.scn and the left terminals, ltr_flank_filter (step 3) -> the is_LTR table;
    out_dir/confident_ltr.scn receives the lines of filter_terminal_align.scn whose left terminal step 3 kept.  reference is a FASTA
    path.  The reference is NOT cut into pieces of 10 Mb as FiLTR cuts it for LtrDetector: the scan has no such limit, so an element
    that lies across such a cut is found.  scan / hsps / cluster / frame_vote replace the device stages (the signatures of
    Context.ltr_scan, .pair_hsps, .frame_cluster, .ltr_frame); model / deep / threshold: the high-copy vote of the hybrid CNN in step 3
    (ltr_flank_decide; without a model the homology rule alone); seconds: a dict that receives the wall seconds of every step.
    -> (path of confident_ltr.scn, {chr-start-end of a left terminal: (is_ltr, "low" | "high" | None, dropped_by)})"""
    os.makedirs(out_dir, exist_ok=True)
    t0 = time.perf_counter()
    total_scn = os.path.join(out_dir, "total.scn")
    ltr_candidate_scan(reference, total_scn, ctx=ctx, scan=scan)
    if seconds is not None:
        seconds["scan"] = time.perf_counter() - t0
    final_scn, _dirty, terminals = ltr_scn_filter(total_scn, reference, out_dir, ctx=ctx, hsps=hsps, seconds=seconds)
    model = _ltr_default_model(model)
    vote = dict(model=model, deep=deep, threshold=threshold) if model is not None else {}          # without a model the call of before
    table, _high = ltr_flank_filter(terminals, reference, flanking_len, max_copy_num, ctx=ctx, cluster=cluster, frame_vote=frame_vote,
                                    seconds=seconds, **vote)
    _ref_names, ref_contigs = read_fasta(reference)
    _terminals, candidate_of = left_ltr_terminals(final_scn, ref_contigs)
    _candidates, lines = read_scn(final_scn, None)
    confident_scn = os.path.join(out_dir, "confident_ltr.scn")
    store_scn([lines[candidate_of[name]] for name in candidate_of if table.get(name, (False,))[0]], confident_scn)
    return confident_scn, table


# ---- FiLTR's steps 4 to 8: from the is_LTR table to the LTR library (bin/FiLTR-main/src/LTR_filter.py:702-813) ---------------------
# Step 4 asks how many full-length copies every confident intact element has.  Where the reference runs minimap2 and filters its SAM
# records (filter_ltr_by_copy_num_minimap, get_copies_minimap2) and then get_intact_ltr_copies, filter_ltr_by_copy_num makes ONE call
# of Context.ltr_copy_support ("full-length copy support" in include/hite_gpu.h: the copy finder and the reference's rules on its
# records, on the device; parity with minimap2 itself is unpinned).  support= replaces it (the signature of Context.ltr_copy_support;
# the CPU tests pass tests/ltrcopy_twin.support).  Everything around the search is the reference's, restated.
def _scn_std(ltr_lines, contig_id):
    """(contig, lLTR_start - 1, rLTR_end) of every candidate line, in the order of ltr_lines"""
    std = []
    for candidate_index in ltr_lines:
        parts = ltr_lines[candidate_index].split(" ")
        std.append((contig_id[parts[11]], int(parts[3]) - 1, int(parts[7])))
    return std


def get_intact_ltr_copies(ltr_copies, ltr_lines, full_length_threshold, reference):
    """bin/FiLTR-main/src/Util.py:11022-11147 on its own dicts: ltr_copies {name: [(chr_name, start1, end1, ...)]} -> {name:
    [(chr_name, start1, end1)]}: the copies that coincide with a candidate line (same segment of 100 000 bases, overlap >=
    full_length_threshold of both), the shorter of two that overlap by 95 % on one chromosome removed, ascending by length"""
    ref_names, ref_contigs = reference if isinstance(reference, tuple) else read_fasta(reference)
    segment_len = 100000
    n_segments = {n: len(ref_contigs[n]) // segment_len + (len(ref_contigs[n]) % segment_len != 0) for n in ref_names}

    def overlaps(prev, start, end):
        overlap_len = max(min(prev[1], end) - max(prev[0], start), 0)
        return overlap_len / abs(prev[1] - prev[0]) >= full_length_threshold and overlap_len / abs(end - start) >= full_length_threshold

    def segment(start, end):
        a, b = start // segment_len, end // segment_len
        return a if a == b or not abs(b * segment_len - start) < abs(end - b * segment_len) else b

    chr_segments = {}
    for candidate_index in ltr_lines:
        parts = ltr_lines[candidate_index].split(" ")
        chr_name, start, end = parts[11], int(parts[3]) - 1, int(parts[7])
        seg = segment(start, end)
        if seg >= n_segments[chr_name]:
            raise KeyError(seg)
        frags = chr_segments.setdefault((chr_name, seg), [])
        if not any(overlaps(p, start, end) for p in frags):
            frags.append((start, end))
    test_fragments = {}
    for ltr_name in ltr_copies:
        for copy in ltr_copies[ltr_name]:
            test_fragments.setdefault(copy[0], []).append((copy[1], copy[2], ltr_name))
    intact_ltr_copies = {}
    for chr_name, fragments in test_fragments.items():
        for start, end, ltr_name in fragments:
            seg = segment(start, end)
            if seg >= n_segments[chr_name]:
                raise KeyError(seg)
            if any(overlaps(p, start, end) for p in chr_segments.get((chr_name, seg), ())):
                intact_ltr_copies.setdefault(ltr_name, []).append((chr_name, start, end))
    for ltr_name, copies in intact_ltr_copies.items():
        copies.sort(key=lambda x: (x[2] - x[1]))
        kept = []
        for i, (chr_i, start_i, end_i) in enumerate(copies):
            if not any(chr_j == chr_i and min(end_i, end_j) - max(start_i, start_j) + 1 >= 0.95 * (end_i - start_i + 1)
                       for chr_j, start_j, end_j in copies[i + 1:]):
                kept.append((chr_i, start_i, end_i))
        intact_ltr_copies[ltr_name] = kept
    return intact_ltr_copies


def filter_ltr_by_copy_num(output_path, leftLtr2Candidates, ltr_lines, reference, tmp_output_dir, split_ref_dir, threads, full_length_threshold,
                           debug, ctx=None, support=None):
    """bin/FiLTR-main/src/Util.py:6119, same arguments: the intact sequences of the candidates whose left terminal output_path marks 1,
    their full-length copies at coverage 0.985 that coincide with a candidate line (full_length_threshold) -> ({name: [(chr_name,
    start1, end1)]}, {name: internal sequence}).  One call of Context.ltr_copy_support (support=) for all elements, in batches of
    Context.FIND_COPIES_BATCH; the genome must be the packed one (set_reference).  Like the reference's, the first dict holds the
    elements with at least one such copy; its keys are in the order of the elements (the reference's follow the order in which it
    walks the copies chromosome by chromosome: the same entries, another order of the lines written from them)."""
    true_ltrs = set()
    with open(output_path, "r") as f_r:
        for line in f_r:
            parts = line.replace("\n", "").split("\t")
            if int(parts[1]):
                true_ltrs.add(parts[0])
    ref_names, ref_contigs = read_fasta(reference)
    contig_id = {n: k for k, n in enumerate(ref_names)}
    internal_ltrs, intact_ltrs = {}, {}
    for name in leftLtr2Candidates:
        if name not in true_ltrs:
            continue
        parts = ltr_lines[leftLtr2Candidates[name]].split(" ")
        ref_seq = ref_contigs[parts[11]]
        intact_ltr_seq = ref_seq[int(parts[3]) - 1: int(parts[7])]
        internal_ltrs[name] = ref_seq[int(parts[4]): int(parts[6]) - 1]
        if len(intact_ltr_seq) > 0:
            intact_ltrs[name] = intact_ltr_seq
    names = list(intact_ltrs)
    if support is None:
        support = (ctx or get_ctx()).ltr_copy_support
    kept = support([intact_ltrs[n] for n in names], _scn_std(ltr_lines, contig_id), 0.985, full_length_threshold) if names else []
    intact_ltr_copies = {n: [(ref_names[c], s, e) for c, s, e in rows] for n, rows in zip(names, kept) if rows}
    return intact_ltr_copies, internal_ltrs


def search_ltr_structure(ltr_name, left_seq, right_seq):
    """bin/FiLTR-main/src/Util.py:9803: a target-site duplication of 6, 5 or 4 bases -- the first k-mer of right_seq without N, longest k
    first, that left_seq holds -> (ltr_name, has_tsd, tsd_seq)"""
    tsd_lens = [6, 5, 4]
    exist_tsd = set()
    for k_num in tsd_lens:
        for i in range(len(left_seq) - k_num + 1):
            left_kmer = left_seq[i: i + k_num]
            if "N" not in left_kmer:
                exist_tsd.add(left_kmer)
    for k_num in tsd_lens:
        for i in range(len(right_seq) - k_num + 1):
            right_kmer = right_seq[i: i + k_num]
            if "N" not in right_kmer and right_kmer in exist_tsd:
                return ltr_name, True, right_kmer
    return ltr_name, False, ""


def is_ltr_has_structure(ltr_name, line, ref_seq):
    """bin/FiLTR-main/src/Util.py:9956: search_ltr_structure on the 8 bases outside and the 3 bases inside both ends of the element of
    a candidate line, clamped at the ends of the chromosome"""
    left_size, internal_size = 8, 3
    parts = line.split(" ")
    lLTR_start, rLTR_end = int(parts[3]), int(parts[7])
    left_seq = ref_seq[max(lLTR_start - 1 - left_size, 0): min(lLTR_start + internal_size - 1, len(ref_seq))]
    right_seq = ref_seq[max(rLTR_end - internal_size, 0): min(rLTR_end + left_size, len(ref_seq))]
    return search_ltr_structure(ltr_name, left_seq, right_seq)


def estimate_insert_time(identity, miu):
    """bin/FiLTR-main/src/Util.py:4174: the Jukes-Cantor distance of the two terminals over twice the mutation rate"""
    d = 1 - identity
    K = -3 / 4 * math.log(1 - d * 4 / 3)
    T = K / (2 * miu)
    return T


def filtr_protein_libs():
    """(LTRPeps.lib, OtherPeps.lib) of FiLTR's databases directory ($HITE_FILTR_DIR/databases): FiLTR's data, not part of this build"""
    lib_dir = os.path.join(os.environ.get("HITE_FILTR_DIR", ""), "databases")
    return os.path.join(lib_dir, "LTRPeps.lib"), os.path.join(lib_dir, "OtherPeps.lib")


def _intact_protein_names(cons, protein_db, output_table, threads, temp_dir, log, debug, search, ctx):
    """one half of the protein test of filter_single_copy_ltr (:6022-6042): the sequences of cons with a hit that spans >= 95 % of a
    protein of protein_db; a missing library is said in the log and gives the empty table blastx gives when it finds nothing"""
    names = {}
    if not os.path.exists(protein_db):
        _scn_log(log, "info", "protein library " + protein_db + " not found (set HITE_FILTR_DIR): the single-copy rule runs with an empty domain table")
        return names
    get_domain_info(cons, protein_db, output_table, threads, temp_dir, search=search, ctx=ctx)
    _protein_names, protein_contigs = read_fasta(protein_db)
    with open(output_table, "r") as f_r:
        for i, line in enumerate(f_r):
            if i < 2:
                continue
            parts = line.split("\t")
            if float(abs(int(parts[5]) - int(parts[4]))) / len(protein_contigs[parts[1]]) >= 0.95:
                names[parts[0]] = True
    if not debug:
        shutil.rmtree(temp_dir, ignore_errors=True)
        if os.path.exists(output_table):
            os.remove(output_table)
    return names


def filter_single_copy_ltr(output_path, filtered_output_path, single_copy_internals_file, ltr_copies, internal_ltrs, ltr_protein_db,
                           other_protein_db, tmp_output_dir, threads, reference, leftLtr2Candidates, ltr_lines, log, debug, search=None, ctx=None):
    """bin/FiLTR-main/src/Util.py:6005, same arguments: an element of ltr_copies with two or more copies is an LTR; one with at most
    one copy only when its internal sequence holds an intact LTR protein and no intact other protein and the element has a
    target-site duplication.  output_path receives name \\t 0 | 1 per element, filtered_output_path the reason of every 0.  search:
    the mode of get_domain_info."""
    single_copy_internals = {name: internal_ltrs[name] for name in ltr_copies if len(ltr_copies[name]) <= 1}
    store_fasta(single_copy_internals, single_copy_internals_file)
    has_protein = _intact_protein_names(single_copy_internals_file, ltr_protein_db, single_copy_internals_file + ".ltr_domain", threads,
                                        tmp_output_dir + "/ltr_domain", log, debug, search, ctx)
    has_other = _intact_protein_names(single_copy_internals_file, other_protein_db, single_copy_internals_file + ".other_domain", threads,
                                      tmp_output_dir + "/other_domain", log, debug, search, ctx)
    has_structure = {}
    _ref_names, ref_contigs = reference if isinstance(reference, tuple) else read_fasta(reference)
    for ltr_name in single_copy_internals:
        line = ltr_lines[leftLtr2Candidates[ltr_name]]
        has_structure[ltr_name] = is_ltr_has_structure(ltr_name, line, ref_contigs[line.split(" ")[11]])[1]
    no_structure = sum(1 for v in has_structure.values() if not v)
    _scn_log(log, "info", "Filter the number of no structure single copy LTR: " + str(no_structure) + ", remaining single copy LTR num: " +
             str(len(single_copy_internals) - no_structure))
    remain_intact_count = filtered_intact_count = 0
    with open(output_path, "w") as f_save, open(filtered_output_path, "w") as f_filtered:
        for name in ltr_copies:
            if len(ltr_copies[name]) >= 2:
                cur_is_ltr = 1
            elif has_other.get(name):
                cur_is_ltr = 0
                f_filtered.write(name + "\t" + "has_intact_other_protein" + "\n")
            elif has_protein.get(name) and has_structure.get(name):
                cur_is_ltr = 1
            else:
                cur_is_ltr = 0
                filter_reason = [why for why, ok in (("no_intact_protein", has_protein.get(name)), ("no_structure", has_structure.get(name))) if not ok]
                f_filtered.write(name + "\t" + ("|".join(filter_reason) if filter_reason else "other") + "\n")
            remain_intact_count += cur_is_ltr
            filtered_intact_count += 1 - cur_is_ltr
            f_save.write(name + "\t" + str(cur_is_ltr) + "\n")
    _scn_log(log, "info", "Filter the number of non-intact LTR: " + str(filtered_intact_count) + ", remaining LTR num: " + str(remain_intact_count))
    if not debug and os.path.exists(single_copy_internals_file):
        os.remove(single_copy_internals_file)


def get_LTR_seq_from_scn(genome, scn_path, ltr_terminal, ltr_internal, ltr_intact, dirty_dicts, ltr_intact_list, miu, coverage_threshold=0.95):
    """bin/FiLTR-main/src/Util.py:4071, same arguments: the lines of scn_path without those that the line before covers (runs of
    neighbours that overlap by coverage_threshold of both), their terminals (<chr>:<start>..<end>-lLTR#LTR, -rLTR#LTR), internal
    sequences (-int#LTR; not of a dirty element) and whole elements as FASTA -- an element with an empty part or a run of ten N is
    left out --, and the list in the layout of LTR_retriever's pass list: motif, TSD, internal interval, identity, insertion time"""
    _ref_names, ref_contigs = read_fasta(genome)
    with open(scn_path, "r") as f_r:
        ltr_lines = [line.replace("\n", "") for line in f_r if not line.startswith("#")]

    def frag(line):
        parts = line.split(" ")
        return parts[11], int(parts[3]) - 1, int(parts[7])

    deredundant_lines, redundant_index = [], set()
    for i in range(len(ltr_lines) - 1):          # (like the reference, the last line is never taken)
        if i in redundant_index:
            continue
        chr_name, chr_start, chr_end = frag(ltr_lines[i])
        for j in range(i + 1, len(ltr_lines)):
            next_chr_name, next_start, next_end = frag(ltr_lines[j])
            overlap_len = max(min(next_end, chr_end) - max(next_start, chr_start), 0)
            if (next_chr_name == chr_name and overlap_len / abs(next_end - next_start) >= coverage_threshold
                    and overlap_len / abs(chr_end - chr_start) >= coverage_threshold):
                redundant_index.add(j)
            else:
                break
        deredundant_lines.append(ltr_lines[i])
    LTR_terminals, LTR_ints, LTR_intacts = {}, {}, {}
    for line in deredundant_lines:
        parts = line.split(" ")
        LTR_start, LTR_end, chr_name = int(parts[0]), int(parts[1]), parts[11]
        lLTR_start, lLTR_end, rLTR_start, rLTR_end = int(parts[3]), int(parts[4]), int(parts[6]), int(parts[7])
        ref_seq = ref_contigs[chr_name]
        lLTR_seq, rLTR_seq = ref_seq[lLTR_start - 1: lLTR_end], ref_seq[rLTR_start - 1: rLTR_end]
        LTR_int_seq, intact_seq = ref_seq[lLTR_end: rLTR_start - 1], ref_seq[lLTR_start - 1: rLTR_end]
        if (len(lLTR_seq) > 0 and len(rLTR_seq) > 0 and len(LTR_int_seq) > 0
                and "NNNNNNNNNN" not in lLTR_seq and "NNNNNNNNNN" not in rLTR_seq and "NNNNNNNNNN" not in LTR_int_seq):
            intact_name = chr_name + ":" + str(LTR_start) + ".." + str(LTR_end)
            LTR_terminals[intact_name + "-lLTR" + "#LTR"] = lLTR_seq
            LTR_terminals[intact_name + "-rLTR" + "#LTR"] = rLTR_seq
            LTR_intacts[intact_name] = intact_seq
            if chr_name + "-" + str(lLTR_start) + "-" + str(lLTR_end) not in dirty_dicts:
                LTR_ints[intact_name + "-int" + "#LTR"] = LTR_int_seq
    store_fasta(LTR_ints, ltr_internal)
    store_fasta(LTR_terminals, ltr_terminal)
    store_fasta(LTR_intacts, ltr_intact)
    with open(ltr_intact_list, "w") as f_save:
        for line in deredundant_lines:
            parts = line.split(" ")
            chr_name = parts[11]
            ref_seq = ref_contigs[chr_name]
            lLTR_start, lLTR_end, rLTR_start, rLTR_end = int(parts[3]), int(parts[4]), int(parts[6]), int(parts[7])
            identity = float(parts[9]) / 100
            insertion_time = int(estimate_insert_time(identity, float(miu)))
            ltr_name, _has_structure, tsd_seq = is_ltr_has_structure(chr_name + ":" + str(int(parts[0])) + ".." + str(int(parts[1])), line, ref_seq)
            motif = ref_seq[lLTR_start - 1: lLTR_start - 1 + 2] + ref_seq[rLTR_end - 2: rLTR_end]
            if tsd_seq == "":
                tsd_seq = "NA"
            f_save.write(ltr_name + "\t" + "pass" + "\t" + "motif:" + motif + "\t" + "TSD:" + tsd_seq + "\t" + "NA..NA\tNA..NA\t" + "IN:" +
                         str(lLTR_end) + ".." + str(rLTR_start - 1) + "\t" + str(identity) + "\t.\tNA\tNA" + "\t" + str(insertion_time) + "\n")


def assign_label_to_lib(lib, intact_LTR_labels):
    """module/Util.py:13859, in place: the entries of lib get the names LTR_<i><type>#<label>, <type> the last four characters of the
    old name (-lLTR and -rLTR both read -LTR: the two terminals of an element become two entries, both with the second's sequence) and <label> that of the element
    <chr>:<start>..<end>.  An entry shares the index of its partner _LTR / _INT (the names of the LTR_retriever branch); FiLTR's
    names end in -LTR / -int, so there every entry has an index of its own -- as in the reference."""
    ltr_names, ltr_contigs = read_fasta(lib)
    no_label_ltr_names, no_label_ltr_contigs = [], {}
    for name in ltr_names:
        seq = ltr_contigs[name]
        name = name.split("#")[0].replace("-lLTR", "-LTR").replace("-rLTR", "-LTR")
        no_label_ltr_names.append(name)
        no_label_ltr_contigs[name] = seq
    ltr_index = 0
    stored_names = set()
    confident_ltr_cut_contigs = {}
    for name in no_label_ltr_names:
        if name in stored_names:
            continue
        intact_ltr_name, ltr_type = name[:-4], name[-4:]
        label = intact_LTR_labels[intact_ltr_name]
        confident_ltr_cut_contigs["LTR_" + str(ltr_index) + ltr_type + "#" + label] = no_label_ltr_contigs[name]
        other_ltr_type = "_INT" if ltr_type == "_LTR" else "_LTR"
        other_name = intact_ltr_name + other_ltr_type
        if other_name in no_label_ltr_contigs:
            confident_ltr_cut_contigs["LTR_" + str(ltr_index) + other_ltr_type + "#" + label] = no_label_ltr_contigs[other_name]
            stored_names.add(other_name)
        ltr_index += 1
    store_fasta(confident_ltr_cut_contigs, lib)


LTR_LIBRARY_FILES = ("intact_LTR.list", "intact_LTR.fa", "confident_ltr.terminal.fa", "confident_ltr.internal.fa", "confident_ltr.fa",
                     "filtered_single_copy_LTRs.txt")


def ltr_library(reference, out_dir, miu=1.3e-8, is_output_lib=1, flanking_len=100, max_copy_num=100, coverage_threshold=0.95, threads=1, debug=0,
                ctx=None, scan=None, hsps=None, cluster=None, frame_vote=None, support=None, dedup=None, model=None, deep=None, threshold=0.5,
                domain_search=None, log=None, seconds=None):
    """FiLTR from the genome to its LTR library, in-tree (bin/FiLTR-main/src/LTR_filter.py:542-813 with is_filter_single and
    is_deredundant on, its defaults): ltr_detect (steps 1 to 3), then
      step 4  filter_ltr_by_copy_num + filter_single_copy_ltr -> out_dir/intact_LTR_homo.txt, filtered_single_copy_LTRs.txt;
      step 5  out_dir/confident_ltr.scn: the lines whose element step 4 kept (the file ltr_detect wrote is replaced);
      step 6  get_LTR_seq_from_scn -> confident_ltr.terminal.fa, confident_ltr.internal.fa, intact_LTR.fa, intact_LTR.list;
      steps 7 and 8 (is_output_lib)  deredundant_for_LTR_v5 on the terminals at 0.95 and on the internal sequences at 0.8, their
              .cons files joined -> confident_ltr.fa.
    The contamination filters of step 3's chunks (filter_tir, filter_helitron, filter_sine), the tandem-repeat filter of the terminals
    and clean_LTR_internal.py are not part of this build.  reference is a FASTA path; it is packed on ctx (set_reference) unless
    support= is given.  scan / hsps / cluster / frame_vote / model / deep / threshold: see ltr_detect; support: see
    filter_ltr_by_copy_num; dedup: replaces deredundant_for_LTR_v5 (same arguments); domain_search: the mode of get_domain_info;
    seconds: a dict that receives the wall seconds of every step.  The de-duplication packs the library on the context where the
    genome was (deredundant_for_LTR_v5): set_reference packs the genome again.  -> {file name: path} of LTR_LIBRARY_FILES"""
    os.makedirs(out_dir, exist_ok=True)
    t = [time.perf_counter()]
    lap = lambda key: (t.append(time.perf_counter()), seconds is not None and seconds.__setitem__(key, t[-1] - t[-2]))  # noqa: E731
    _conf, table = ltr_detect(reference, out_dir, flanking_len, max_copy_num, ctx=ctx, scan=scan, hsps=hsps, cluster=cluster, frame_vote=frame_vote,
                              seconds=seconds, model=model, deep=deep, threshold=threshold)
    t.append(time.perf_counter())
    final_scn = os.path.join(out_dir, "filter_terminal_align.scn")
    ref_names, ref_contigs = read_fasta(reference)
    _terminals, leftLtr2Candidates = left_ltr_terminals(final_scn, ref_contigs, log)
    _candidates, ltr_lines = read_scn(final_scn, log)
    with open(os.path.join(out_dir, "remove_recomb.scn")) as f:
        dirty_dicts = remove_dirty_LTR([line.replace("\n", "") for line in f if line.strip() and not line.startswith("#")], log)
    msa_flank = os.path.join(out_dir, "msa_flank.txt")
    with open(msa_flank, "w") as f_save:
        for name in leftLtr2Candidates:
            f_save.write(name + "\t" + str(int(bool(table.get(name, (False,))[0]))) + "\n")
    # step 4
    if support is None:
        ctx = ctx or set_reference(reference)
    ltr_copies, internal_ltrs = filter_ltr_by_copy_num(msa_flank, leftLtr2Candidates, ltr_lines, reference, out_dir, None, threads, coverage_threshold,
                                                       debug, ctx=ctx, support=support)
    lap("copy_support")
    if debug:
        with open(os.path.join(out_dir, "ltr_copies.json"), "w", encoding="utf-8") as f:
            json.dump(ltr_copies, f, ensure_ascii=False, indent=4)
    intact_output_path = os.path.join(out_dir, "intact_LTR_homo.txt")
    ltr_protein_db, other_protein_db = filtr_protein_libs()
    filter_single_copy_ltr(intact_output_path, os.path.join(out_dir, "filtered_single_copy_LTRs.txt"), os.path.join(out_dir, "single_copy_internal.fa"),
                           ltr_copies, internal_ltrs, ltr_protein_db, other_protein_db, out_dir, threads, (ref_names, ref_contigs),
                           leftLtr2Candidates, ltr_lines, log, debug, search=domain_search, ctx=ctx)
    lap("single_copy")
    # step 5
    true_ltrs = set()
    with open(intact_output_path, "r") as f_r:
        for line in f_r:
            parts = line.replace("\n", "").split("\t")
            if int(parts[1]):
                true_ltrs.add(parts[0])
    confident_scn = os.path.join(out_dir, "confident_ltr.scn")
    store_scn([ltr_lines[leftLtr2Candidates[name]] for name in leftLtr2Candidates if name in true_ltrs], confident_scn)
    # step 6
    paths = {name: os.path.join(out_dir, name) for name in LTR_LIBRARY_FILES}
    get_LTR_seq_from_scn(reference, confident_scn, paths["confident_ltr.terminal.fa"], paths["confident_ltr.internal.fa"], paths["intact_LTR.fa"],
                         dirty_dicts, paths["intact_LTR.list"], miu)
    lap("sequences")
    # steps 7 and 8
    if is_output_lib:
        dedup = dedup or (lambda *a: deredundant_for_LTR_v5(*a, ctx=ctx))
        dedup(paths["confident_ltr.terminal.fa"], out_dir, threads, "terminal", 0.95, debug)
        dedup(paths["confident_ltr.internal.fa"], out_dir, threads, "internal", 0.8, debug)
        with open(paths["confident_ltr.fa"], "w") as out:
            for part in (paths["confident_ltr.terminal.fa"], paths["confident_ltr.internal.fa"]):
                with open(part + ".cons") as f:
                    shutil.copyfileobj(f, out)
        lap("library")
    return paths


# ---- the annotation of the genome with the library (where HiTE ends with RepeatMasker: annotate_genome.py:17, pan_annotate_genome.py:27)
# In-tree stage, PARITY UNPINNED against RepeatMasker: what is computed is the "genome annotation" of include/hite_gpu.h
# (Context.annotate), held to its CPU twin.  annot= replaces the device stage (the signature of Context.annotate; the CPU tests pass the
# twin).  The files are written in RepeatMasker's layouts because the reference reads them back (get_full_length_copies_from_gff_v1).
def annotation_columns(rec, g_len=None, q_len=None):
    """(mismatches, gaps in the library row, gaps in the genome row) of an annotation record (seq, g_start, g_end, lib, strand, q_start,
    q_end, score, matches, columns), from the arithmetic of the alignment alone: a column is a match (+2), a mismatch (-4) or a gap (-5),
    so G = 6 matches - 4 columns - score columns are gaps, X = columns - matches - G are mismatches, the genome interval holds
    matches + X + (gaps in the library row) bases and the library interval matches + X + (gaps in the genome row)."""
    g_len = rec[2] - rec[1] if g_len is None else g_len
    q_len = rec[6] - rec[5] if q_len is None else q_len
    score, matches, columns = int(rec[7]), int(rec[8]), int(rec[9])
    gaps = 6 * matches - 4 * columns - score
    mism = columns - matches - gaps
    return mism, int(g_len) - matches - mism, int(q_len) - matches - mism


def _lib_name_class(header):
    name, _, cls = header.partition("#")
    return name, cls or "Unknown"


def _publish(path, lines):
    """a temporary name first, then the rename: a file that exists is complete"""
    tmp = path + ".tmp"
    with open(tmp, "w") as f_save:
        f_save.writelines(lines)
    os.replace(tmp, path)


def _pct(part, whole):
    return "%.1f" % (100.0 * part / whole if whole else 0.0)


def repeatmasker_out_lines(records, ref_names, ref_lens, lib_names, lib_lens):
    """the lines of write_repeatmasker_out, the three header lines first"""
    lines = ["   SW   perc perc perc  query     position in query    matching  repeat       position in repeat\n",
             "score   div. del. ins.  sequence  begin end   (left)   repeat    class/family begin  end    (left)  ID\n", "\n"]
    for k, rec in enumerate(records):
        rec = [int(v) for v in rec]
        seq, gs, ge, lib, strand, qs, qe = rec[:7]
        mism, gap_lib, gap_genome = annotation_columns(rec)
        name, cls = _lib_name_class(lib_names[lib])
        left = "(%d)" % (lib_lens[lib] - qe)
        repeat = (left, qe, qs + 1) if strand else (qs + 1, qe, left)
        lines.append("%6d %5s %4s %4s  %s %8d %8d %s %s %s %s %6s %6s %6s %5d\n" % (
            rec[7], _pct(mism, rec[8] + mism), _pct(gap_genome, ge - gs), _pct(gap_lib, ge - gs), ref_names[seq], gs + 1, ge,
            "(%d)" % (ref_lens[seq] - ge), "C" if strand else "+", name, cls, repeat[0], repeat[1], repeat[2], k + 1))
    return lines


def write_repeatmasker_out(records, ref_names, ref_lens, lib_names, lib_lens, path):
    """the 15 columns of a RepeatMasker `.out` under its three header lines, one line per record in the order given: SW score (the
    record's score: 2 / -4 / -5, not a matrix score), percentage divergence 100 X / (M + X), percentage deletions (library bases without
    a genome base) and insertions (genome bases without a library base), both of the genome interval, all to one decimal; the
    sequence, begin, end (1-based, inclusive) and (left); + or C; the name (the library header before #) and class/family (after #, or
    Unknown); begin, end, (left) in the entry -- (left), end, begin for C; a running ID."""
    _publish(path, repeatmasker_out_lines(records, ref_names, ref_lens, lib_names, lib_lens))


def repeatmasker_gff_lines(records, ref_names, lib_names):
    lines = ["##gff-version 2\n"]
    for rec in records:
        rec = [int(v) for v in rec]
        mism = annotation_columns(rec)[0]
        lines.append("%s\tRepeatMasker\tdispersed_repeat\t%d\t%d\t%s\t%s\t.\tTarget \"Motif:%s\" %d %d\n" % (
            ref_names[rec[0]], rec[1] + 1, rec[2], _pct(mism, rec[8] + mism), "-" if rec[4] else "+", _lib_name_class(lib_names[rec[3]])[0],
            rec[5] + 1, rec[6]))
    return lines


def write_repeatmasker_gff(records, ref_names, lib_names, path):
    """one line per record in the form `RepeatMasker -gff` writes and the reference's reader splits (Util.py:13689-13708): sequence,
    RepeatMasker, dispersed_repeat, start, end (1-based, inclusive), the divergence, + or -, ., Target "Motif:NAME" and the interval in
    the entry (1-based, inclusive, ascending on either strand)"""
    _publish(path, repeatmasker_gff_lines(records, ref_names, lib_names))


def repeatmasker_tbl_rows(records, ref_lens, lib_names):
    """[(class, elements, bases covered)] by class name and the total row ("total", ...): the bases are the union of the genome
    intervals of the class (of all records for the total)"""
    by_class = {}
    for rec in records:
        by_class.setdefault(_lib_name_class(lib_names[int(rec[3])])[1], []).append((int(rec[0]), int(rec[1]), int(rec[2])))

    def union(ivs):
        total, cur = 0, None
        for seq, a, b in sorted(ivs):
            if cur is not None and cur[0] == seq and a <= cur[2]:
                cur[2] = max(cur[2], b)
            else:
                total += cur[2] - cur[1] if cur else 0
                cur = [seq, a, b]
        return total + (cur[2] - cur[1] if cur else 0)

    rows = [(cls, len(ivs), union(ivs)) for cls, ivs in sorted(by_class.items())]
    return rows + [("total", sum(r[1] for r in rows), union([iv for ivs in by_class.values() for iv in ivs]))]


def write_repeatmasker_tbl(records, ref_names, ref_lens, lib_names, path):
    """a summary in the spirit of RepeatMasker's `.tbl`, NOT byte-compatible with it: the number of sequences and bases, then per
    class/family the number of elements, the bases covered (the union on the genome) and their percentage of the genome, and a total"""
    total = sum(ref_lens)
    lines = ["sequences: %d\n" % len(ref_names), "total length: %d bp\n" % total, "%-28s %10s %14s %8s\n" % ("class", "elements", "bases", "percent")]
    for cls, n, bases in repeatmasker_tbl_rows(records, ref_lens, lib_names):
        lines.append("%-28s %10d %14d %7s%%\n" % (cls, n, bases, "%.2f" % (100.0 * bases / total if total else 0.0)))
    _publish(path, lines)


def _log_info(log, msg):
    if log is not None:
        (log.logger if hasattr(log, "logger") else log).info(msg)


def annotate_to_files(lib_path, reference, out_path, gff_path, tbl_path, ctx=None, annot=None, log=None):
    """the in-tree annotation of `reference` (a FASTA path) with the library `lib_path`: the three files -> the records"""
    ref_names, ref_contigs = read_fasta(reference)
    lib_names, lib_contigs = read_fasta(lib_path)
    annot = annot or (ctx or get_ctx()).annotate
    stats = {}
    records, status = annot([ref_contigs[n] for n in ref_names], [lib_contigs[n] for n in lib_names], stats=stats)
    for e, s in enumerate(status):
        if s:
            _log_info(log, "annotate: %s is longer than the annotation's limit for an entry and was not searched" % lib_names[e])
    _log_info(log, "annotate: %d records (%s)" % (len(records), ", ".join("%s %d" % kv for kv in stats.items())))
    ref_lens, lib_lens = [len(ref_contigs[n]) for n in ref_names], [len(lib_contigs[n]) for n in lib_names]
    write_repeatmasker_out(records, ref_names, ref_lens, lib_names, lib_lens, out_path)
    write_repeatmasker_gff(records, ref_names, lib_names, gff_path)
    write_repeatmasker_tbl(records, ref_names, ref_lens, lib_names, tbl_path)
    return records


def annotate_genome(tmp_output_dir, classified_TE_consensus, reference, annotate, threads, log, ctx=None, annot=None):
    """annotate_genome.py:14 with its positional arguments: HiTE.out, HiTE.gff and HiTE.tbl in tmp_output_dir when annotate is 1.
    RepeatMasker runs when it is installed, unless HITE_ANNOTATOR=gpu or annot= is given; otherwise the in-tree stage
    (annotate_to_files).  The in-tree stage writes no HiTE.cat.gz (the alignments themselves are not kept)."""
    if annotate is None or int(annotate) != 1:
        return
    if annot is None and os.environ.get("HITE_ANNOTATOR", "") != "gpu" and shutil.which("RepeatMasker") is not None:
        cmd = "cd %s && RepeatMasker -e ncbi -pa %s -gff -lib %s -cutoff 225 %s" % (tmp_output_dir, threads, classified_TE_consensus, reference)
        _log_info(log, "Running command: " + cmd)
        subprocess.run(cmd, shell=True, check=False)
        for suffix, name in ((".out", "HiTE.out"), (".tbl", "HiTE.tbl"), (".out.gff", "HiTE.gff"), (".cat.gz", "HiTE.cat.gz")):
            if os.path.exists(reference + suffix):
                shutil.move(reference + suffix, os.path.join(tmp_output_dir, name))
        return
    _log_info(log, "annotate: the in-tree annotation (hite_annotate) stands in for RepeatMasker; no HiTE.cat.gz is written")
    annotate_to_files(classified_TE_consensus, reference, os.path.join(tmp_output_dir, "HiTE.out"), os.path.join(tmp_output_dir, "HiTE.gff"),
                      os.path.join(tmp_output_dir, "HiTE.tbl"), ctx=ctx, annot=annot, log=log)


def _fmea_new_chain(frags, skip_gap, subject_name, minus):
    """the chaining of FMEA_new (Util.py:12340) on the fragments (q_start, q_end, s_start, s_end) of one entry, one sequence and one
    direction, in its order: a fragment extends EVERY earlier chain it fits (latest first, until one lies skip_gap or more before it),
    and starts a chain of its own only when it extended none"""
    chains = []
    for qs, qe, ss, se in frags:
        extended = False
        for k in range(len(chains) - 1, -1, -1):
            pqs, pqe, pss, pse, _name = chains[k]
            dist = pse - ss if minus else ss - pse
            if dist >= skip_gap:
                break
            if (se < pse if minus else se > pse) and qs - pqe < skip_gap and qe > pqe:
                if minus:
                    chains[k] = (pqs, qe, max(pss, ss), se, subject_name)
                else:
                    chains[k] = (min(pqs, qs), qe, min(pss, ss), se, subject_name)
                extended = True
        if not extended:
            chains.append((qs, qe, ss, se, subject_name))
    return chains


def FMEA_new(query_contigs, query_records, full_length_threshold):
    """Util.py:12340 restated: {entry: [(entry, q_start, q_end, sequence, s_start, s_end)]}, starts 0-based.  Entries in the order of
    query_records, sequences in the order met, the plus fragments (s_start <= s_end, by (s_start, s_end)) before the minus ones (by
    descending (s_start, s_end)); an entry that is not in query_contigs is left out."""
    longest_repeats = {}
    for query_name, subject_dict in query_records.items():
        if query_name not in query_contigs:
            continue
        skip_gap = len(query_contigs[query_name]) * (1 - full_length_threshold)
        chains = []
        for subject_name, frags in subject_dict.items():
            plus = sorted((f for f in frags if not f[2] > f[3]), key=lambda x: (x[2], x[3]))
            minus = sorted((f for f in frags if f[2] > f[3]), key=lambda x: (-x[2], -x[3]))
            chains += _fmea_new_chain(plus, skip_gap, subject_name, False) + _fmea_new_chain(minus, skip_gap, subject_name, True)
        longest_repeats[query_name] = [(query_name, c[0] - 1, c[1], c[4], c[2] - 1, c[3]) for c in chains]
    return longest_repeats


def read_repeatmasker_gff(gff_path):
    """-> ({entry: {sequence: [(q_start, q_end, s_start, s_end)]}}, the entry of the last line) as Util.py:13689-13708 reads the file"""
    query_records, last = {}, None
    with open(gff_path) as f_r:
        for line in f_r:
            if line.startswith("#"):
                continue
            parts = line.split("\t")
            info = parts[8].split(" ")
            last = info[1].replace('"', "").split(":")[1]
            query_records.setdefault(last, {}).setdefault(parts[0], []).append((int(info[2]), int(info[3]), int(parts[3]), int(parts[4])))
    return query_records, last


def get_full_length_copies_from_gff_v1(TE_lib, reference, gff_path, full_length_threshold, te_classes):
    """Util.py:13679 restated: the chains of FMEA_new over the GFF's records that span at least full_length_threshold of their entry
    -> (full_length_copies {entry: {"seq:start-end": bases}}, the same with flanks, full_length_annotations {entry: [(class, sequence,
    start (0-based), end, direction)]}).  As there: the flank is 5 bases when the entry of the LAST line of the GFF has Helitron in
    its name and 50 otherwise, for every entry; a flank that would begin before the sequence gives what Python's slice gives; a GFF's
    start is never above its end, so every copy is '+' whatever its strand column says.  A GFF without records gives three empty
    dictionaries (the reference fails there)."""
    _ref_names, ref_contigs = read_fasta(reference)
    query_names, contigs = read_fasta(TE_lib)
    query_contigs = {name.split("#")[0]: contigs[name] for name in query_names}
    query_records, last = read_repeatmasker_gff(gff_path)
    if last is None:
        return {}, {}, {}
    longest_repeats = FMEA_new(query_contigs, query_records, full_length_threshold)
    flanking_len = 5 if "Helitron" in str(last) else 50
    full_length_copies, flank_full_length_copies, full_length_annotations = {}, {}, {}
    for query_name, repeats in longest_repeats.items():
        query_len = len(query_contigs[query_name])
        annotations, query_copies, flank_query_copies = [], {}, {}
        for _name, q_start, q_end, subject_name, s_start, s_end in repeats:
            if abs(q_end - q_start) < full_length_threshold * query_len:
                continue
            direct = "-" if s_start > s_end else "+"
            lo, hi = (s_end, s_start) if s_start > s_end else (s_start, s_end)
            subject_pos = "%s:%d-%d" % (subject_name, lo, hi)
            query_copies[subject_pos] = ref_contigs[subject_name][lo:hi]
            flank_query_copies[subject_pos] = ref_contigs[subject_name][lo - flanking_len:hi + flanking_len]
            annotations.append((te_classes[query_name], subject_name, lo, hi, direct))
        full_length_copies[query_name] = query_copies
        flank_full_length_copies[query_name] = flank_query_copies
        full_length_annotations[query_name] = annotations
    return full_length_copies, flank_full_length_copies, full_length_annotations


def get_TE_class(panTE_lib):
    """Util.py:13421: ({name before #: class after #}, {name before #: sequence})"""
    te_names, te_contigs = read_fasta(panTE_lib)
    return {n.split("#")[0]: n.split("#")[1] for n in te_names}, {n.split("#")[0]: te_contigs[n] for n in te_names}


def full_length_gff_lines(full_length_annotations):
    """the lines of <genome>.full_length.gff as pan_annotate_genome.py:50-66 makes them: numbered in the order of the annotations, then
    ordered as `sort -k1,1 -k4n` orders them in the C locale (by sequence name, then by start, ties by the whole line)"""
    lines, n = [], 0
    for query_name, annotations in full_length_annotations.items():
        for cls, chr_name, start, end, direct in annotations:
            n += 1
            lines.append("%s\tHiTE\t%s\t%d\t%d\t.\t%s\t.\tid=te_intact_%d;name=%s;classification=%s\n" % (chr_name, cls, start + 1, end, direct, n, query_name, cls))
    return sorted(lines, key=lambda ln: (ln.split("\t")[0].encode(), int(ln.split("\t")[3]), ln.encode()))
