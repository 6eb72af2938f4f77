"""Synthetic workload generator for bench.py and the full-size tests: a random
genome (GC 0.42, 50 Mbp chromosomes) with TIR and LTR families planted as diverged, partly
truncated copies with target-site duplications, plus the candidate file and the copy table that
the fine stage consumes.  Bench/test tooling only -- not part of the product path.

Everything random derives from numpy PCG64 / torch Philox seeds, so a (config, seed) pair names
the workload.  The background genome is generated on the GPU when one is given, the planted
copies with numpy on the host.
"""
import numpy as np

ASCII = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = np.array([3, 2, 1, 0], dtype=np.uint8)  # on codes


def _rand_codes(rng, n, gc=0.42):
    p = np.array([(1 - gc) / 2, gc / 2, gc / 2, (1 - gc) / 2])
    return rng.choice(4, size=n, p=p).astype(np.uint8)


def _mutate_copy(rng, cons, div, indel_rate):
    s = cons.copy()
    L = len(s)
    m = rng.random(L) < div
    k = int(m.sum())
    if k:
        s[m] = (s[m] + rng.integers(1, 4, size=k).astype(np.uint8)) & 3
    n_ind = rng.binomial(max(L - 40, 1), indel_rate)
    if n_ind:
        pos = np.sort(rng.integers(20, L - 20, size=n_ind))
        is_del = rng.random(n_ind) < 0.5
        dpos = pos[is_del]
        ipos = pos[~is_del]
        if len(ipos):
            s = np.insert(s, ipos, rng.integers(0, 4, size=len(ipos)).astype(np.uint8))
            # deletion positions shift by the insertions before them
            dpos = dpos + np.searchsorted(ipos, dpos, side="right")
        if len(dpos):
            s = np.delete(s, np.unique(dpos))
    return s


def make_families(rng, n_tir, n_ltr, max_copies=300):
    fams = []
    for f in range(n_tir + n_ltr):
        is_ltr = f >= n_tir
        if not is_ltr:
            L = int(rng.integers(150, 3001))
            tl = int(rng.integers(10, 41))
            tir = _rand_codes(rng, tl)
            if tir[0] == 3 and tir[1] == 2:  # avoid TG...CA
                tir[0] = 1
            body = _rand_codes(rng, max(L - 2 * tl, 20))
            right = COMP[tir[::-1]].copy()
            dv = rng.random(tl) < 0.05  # TIR arms at <= 10 % divergence
            right[dv] = (right[dv] + 1) & 3
            cons = np.concatenate([tir, body, right])
            tsd = int(rng.choice([2, 3, 4, 5, 6, 8, 9, 10, 11]))
        else:
            ltr = _rand_codes(rng, int(rng.integers(100, 1501)))
            ltr[0], ltr[1], ltr[-2], ltr[-1] = 3, 2, 1, 0  # TG ... CA
            internal = _rand_codes(rng, int(rng.integers(1000, 8001)))
            cons = np.concatenate([ltr, internal, ltr])
            tsd = 5
        ncopy = int(min(max_copies, 2 + rng.geometric(0.05)))
        fams.append(dict(cons=cons, tsd=tsd, ncopy=ncopy, ltr=is_ltr))
    return fams


def make_workload(genome_bp=100_000_000, n_tir=500, n_ltr=0, cands_per_family=10, seed=20250927, chrom_bp=50_000_000,
                  device=None, flank=50, cand_seed=None, family_seed=None, family_keep=1.0):
    """-> dict(genome (uint8 ASCII, torch tensor on `device` or numpy), contig_off, cands (uint8 array),
    cand_off, copy_first, contig, start1, end1, minus, family, n_families, planted)"""
    rng = np.random.default_rng(seed)
    if family_seed is None:
        fams = make_families(rng, n_tir, n_ltr)
    else:
        # population genomes (config C5): the families come from a seed all genomes share, each genome carries a random
        # family_keep fraction of them (its own copies, positions and divergences)
        fams = make_families(np.random.default_rng(family_seed), n_tir, n_ltr)
        for f_, keep_ in zip(fams, rng.random(len(fams)) < family_keep):
            if not keep_:
                f_["ncopy"] = 0
    n_chr = max(1, int(np.ceil(genome_bp / chrom_bp)))
    contig_off = np.minimum(np.arange(n_chr + 1, dtype=np.int64) * chrom_bp, genome_bp)
    # ---- planted copies ------------------------------------------------------------------------
    seqs, meta, divs = [], [], []  # meta: (family, strand, full_len_flag, tsd_len)
    for fi, fam in enumerate(fams):
        cons = fam["cons"]
        for k in range(fam["ncopy"]):
            div = float(rng.random() * 0.15) if k else 0.0
            s = _mutate_copy(rng, cons, div, 0.01 if k else 0.0)
            full = True
            if k and rng.random() < 0.2:  # 5' / 3' truncation
                cut = int(rng.integers(1, max(2, len(s) // 2)))
                full = cut < 0.05 * len(cons)
                s = s[cut:] if rng.random() < 0.5 else s[:-cut]
            minus = bool(rng.integers(0, 2))
            if minus:
                s = COMP[s[::-1]]
            seqs.append(s)
            meta.append((fi, minus, full, fam["tsd"]))
            divs.append(div)
    n_copies = len(seqs)
    lens = np.array([len(s) for s in seqs], dtype=np.int64)
    pad = 2 * flank + 40
    need = int((lens + pad).sum())
    if need > 0.8 * genome_bp:
        raise ValueError("planted copies (%d bp) do not fit the genome (%d bp)" % (need, genome_bp))
    order = rng.permutation(n_copies)
    free = genome_bp - need
    gaps = np.sort(rng.integers(0, free + 1, size=n_copies))
    starts = gaps + np.concatenate([[0], np.cumsum((lens + pad)[order])[:-1]]) + pad // 2
    pos = np.zeros(n_copies, dtype=np.int64)
    pos[order] = starts
    # drop copies that would cross a chromosome border (+- flank)
    chrom = np.searchsorted(contig_off, pos, side="right") - 1
    ok = (pos - pad // 2 >= contig_off[chrom]) & (pos + lens + pad // 2 <= contig_off[chrom + 1])
    # ---- background genome ---------------------------------------------------------------------
    if device is not None:
        import torch

        gen = torch.Generator(device=device)
        gen.manual_seed(int(seed))
        g = torch.empty(genome_bp + 64, dtype=torch.uint8, device=device)
        lut = torch.tensor([65, 67, 71, 84], dtype=torch.uint8, device=device)
        thr = torch.tensor([0.29, 0.50, 0.71], device=device)
        step = 1 << 26
        for a in range(0, genome_bp, step):
            b = min(genome_bp, a + step)
            u = torch.rand(b - a, device=device, generator=gen)
            g[a:b] = lut[torch.bucketize(u, thr)]
        g[genome_bp:] = 65
        # overwrite with the planted copies (+ TSDs)
        buf = np.concatenate([ASCII[s] for s, o in zip(seqs, ok) if o]) if ok.any() else np.zeros(0, np.uint8)
        dst = np.concatenate([np.arange(p, p + l, dtype=np.int64) for p, l, o in zip(pos, lens, ok) if o]) if ok.any() else np.zeros(0, np.int64)
        tb = torch.from_numpy(buf).to(device)
        td = torch.from_numpy(dst).to(device)
        g[td] = tb
        del tb, td
        tsd_src, tsd_dst = [], []
        for p, l, o, m in zip(pos, lens, ok, meta):
            if o:
                t = m[3]
                tsd_src.append(np.arange(p - t, p, dtype=np.int64))
                tsd_dst.append(np.arange(p + l, p + l + t, dtype=np.int64))
        if tsd_src:
            ts = torch.from_numpy(np.concatenate(tsd_src)).to(device)
            tdd = torch.from_numpy(np.concatenate(tsd_dst)).to(device)
            g[tdd] = g[ts]
        genome = g

        def slice_bytes(a, b):
            return genome[a:b].cpu().numpy()
    else:
        gnp = ASCII[_rand_codes(rng, genome_bp)]
        gnp = np.concatenate([gnp, np.full(64, 65, np.uint8)])
        for s, p, l, o, m in zip(seqs, pos, lens, ok, meta):
            if o:
                gnp[p:p + l] = ASCII[s]
                t = m[3]
                gnp[p + l:p + l + t] = gnp[p - t:p]
        genome = gnp

        def slice_bytes(a, b):
            return genome[a:b]
    # ---- candidates + copy table ---------------------------------------------------------------
    crng = np.random.default_rng(seed + 7919 if cand_seed is None else cand_seed)
    by_fam = {}
    for i, (fi, minus, full, _t) in enumerate(meta):
        if ok[i] and full:
            by_fam.setdefault(fi, []).append(i)
    cand_chunks, cand_len, copy_first = [], [], [0]
    c_contig, c_s1, c_e1, c_minus, c_fam, c_div = [], [], [], [], [], []
    rc_lut = np.zeros(256, dtype=np.uint8)
    rc_lut[:] = ord("N")
    for a, b in zip(b"ACGT", b"TGCA"):
        rc_lut[a] = b
    for fi in sorted(by_fam):
        members = by_fam[fi]
        for v in range(cands_per_family):
            i = members[int(crng.integers(0, len(members)))]
            dl, dr = int(crng.integers(-30, 31)), int(crng.integers(-30, 31))
            a = int(pos[i]) - dl if not meta[i][1] else int(pos[i]) - dr
            b = int(pos[i] + lens[i]) + dr if not meta[i][1] else int(pos[i] + lens[i]) + dl
            a = max(a, int(contig_off[chrom[i]]))
            b = min(b, int(contig_off[chrom[i] + 1]))
            if b - a < 60:
                a, b = int(pos[i]), int(pos[i] + lens[i])
            sq = np.asarray(slice_bytes(a, b))
            if meta[i][1]:
                sq = rc_lut[sq[::-1]]
            cand_chunks.append(np.ascontiguousarray(sq))
            cand_len.append(len(sq))
            for j in members:
                f1, f2 = int(crng.integers(0, 3)), int(crng.integers(0, 3))
                c_contig.append(int(chrom[j]))
                c_s1.append(int(pos[j] - contig_off[chrom[j]]) + 1 - f1)
                c_e1.append(int(pos[j] - contig_off[chrom[j]] + lens[j]) + f2)
                c_minus.append(1 if meta[j][1] else 0)
            copy_first.append(len(c_contig))
            c_fam.append(fi)
            c_div.append(divs[i])
    cand_off = np.zeros(len(cand_len) + 1, dtype=np.int64)
    np.cumsum(cand_len, out=cand_off[1:])
    cands = np.concatenate(cand_chunks) if cand_chunks else np.zeros(0, np.uint8)
    return dict(genome=genome, genome_bp=genome_bp, contig_off=contig_off, cands=cands, cand_off=cand_off,
                copy_first=np.array(copy_first, dtype=np.int32), contig=np.array(c_contig, dtype=np.int32),
                start1=np.array(c_s1, dtype=np.int64), end1=np.array(c_e1, dtype=np.int64),
                minus=np.array(c_minus, dtype=np.uint8), family=np.array(c_fam, dtype=np.int32),
                cand_div=np.array(c_div, dtype=np.float64),   # divergence of the copy each candidate was cut from
               
                n_families=len(fams), n_planted=int(ok.sum()), planted_bp=int(lens[ok].sum()),
                fam_is_ltr=np.array([f["ltr"] for f in fams], dtype=bool),
                fam_len=np.array([len(f["cons"]) for f in fams], dtype=np.int64),
                # ground truth of the planted copies (tests / recall measurements): family, contig, 0-based start inside the
                # contig, length, strand, "full length" flag (not truncated beyond 5 %), divergence from the family consensus
                planted=dict(family=np.array([m[0] for m in meta], dtype=np.int32)[ok], contig=chrom[ok].astype(np.int32),
                             start=(pos - contig_off[chrom])[ok], length=lens[ok],
                             minus=np.array([m[1] for m in meta], dtype=bool)[ok], full=np.array([m[2] for m in meta], dtype=bool)[ok],
                             div=np.array(divs, dtype=np.float64)[ok]))


def make_ltr_flank_genome(plan, genome_bp=450_000, chrom_bp=150_000, seed=1, term_len=300, homo_len=150, div=0.03):
    """A genome for the LTR flank filter (util.ltr_flank_filter; tests and tools/ltr_filter_bench.py): plan = [(kind, copies), ...],
    one family of `copies` copies of a term_len-base terminal sequence per entry --
      "ltr"    every copy sits in random flanks (a true LTR terminal);
      "inner"  the terminal is the middle of a longer repeat: homo_len homologous bases on both sides of every copy;
      "left" / "right"  one flank homologous, the other random (in the orientation of the terminal sequence).
    Copies diverge by `div` (substitutions, a few indels), lie on either strand, and keep more than 100 bases from each other and
    from the contig ends.  -> dict(contigs [str], names [str], terminals {name: sequence of copy 0}, kind {name}, copies {name})"""
    rng = np.random.default_rng(seed)
    n_chr = max(1, genome_bp // chrom_bp)
    genome = [ASCII[_rand_codes(rng, chrom_bp)] for _ in range(n_chr)]
    slot = term_len + 2 * homo_len + 300
    per_chr = chrom_bp // slot - 2
    total = sum(n for _k, n in plan)
    if total > n_chr * per_chr:
        raise ValueError("planted copies do not fit the genome")
    slots = rng.permutation(n_chr * per_chr)[:total]
    names, terminals, kind, copies = [], {}, {}, {}
    at = 0
    for f, (k, n) in enumerate(plan):
        term, hl, hr = _rand_codes(rng, term_len), _rand_codes(rng, homo_len), _rand_codes(rng, homo_len)
        name = "%s_%d_%d" % (k, n, f)
        names.append(name)
        terminals[name] = ASCII[term].tobytes().decode()
        kind[name], copies[name] = k, n
        for c in range(n):
            ci, si = divmod(int(slots[at]), per_chr)
            at += 1
            parts = [_mutate_copy(rng, hl, div, 0.002)] if k in ("inner", "left") else []
            parts.append(_mutate_copy(rng, term, div, 0.002) if c else term)
            if k in ("inner", "right"):
                parts.append(_mutate_copy(rng, hr, div, 0.002))
            unit = np.concatenate(parts)
            lead = len(parts[0]) if k in ("inner", "left") else 0      # the terminal starts at the same place of its slot
            if rng.integers(0, 2):
                unit, lead = COMP[unit[::-1]], len(unit) - lead - len(parts[1 if k in ("inner", "left") else 0])
            pos = (si + 1) * slot + homo_len + 150 - lead
            genome[ci][pos:pos + len(unit)] = ASCII[unit]
    return dict(contigs=[g.tobytes().decode() for g in genome], names=names, terminals=terminals, kind=kind, copies=copies)


LTR_ELEMENT_KINDS = ("clean", "recomb", "nested", "overhang", "shifted", "dirty", "dup")
_LTR_SLOT = 10_000          # bases of chromosome per planted element (the longest is 2 x 1 200 + 6 000 and its guards)
_LTR_GUARD = 12             # bases outside a terminal that cannot match the other terminal's (disjoint alphabets)
_LTR_CLEAN_END = 20         # bases at both ends of a terminal that its second copy keeps unchanged


def _diverged_terminal(rng, term, div, n_indel):
    """the second copy of a terminal: substitutions at rate div and n_indel indels of 1 .. 3 bases, its two ends left as they are"""
    s = term.copy()
    L = len(s)
    m = rng.random(L) < div
    m[:_LTR_CLEAN_END] = False
    m[L - _LTR_CLEAN_END:] = False
    if m.any():
        s[m] = (s[m] + rng.integers(1, 4, size=int(m.sum())).astype(np.uint8)) & 3
    for _ in range(n_indel):
        pos = int(rng.integers(2 * _LTR_CLEAN_END, len(s) - 2 * _LTR_CLEAN_END))
        k = int(rng.integers(1, 4))
        s = np.delete(s, np.arange(pos, pos + k)) if rng.integers(0, 2) else np.insert(s, pos, rng.integers(0, 4, size=k).astype(np.uint8))
    return s


def _ltr_element(rng, kind, term_len, int_len):
    """one planted element -> (codes of the element and its guards, dict of 0-based half-open intervals inside them: left, right and,
    by kind, repeat (start of the first copy, end of the second) / inner (another element's intervals))"""
    term = _rand_codes(rng, term_len)
    right = _diverged_terminal(rng, term, float(rng.uniform(0.01, 0.08)), int(rng.integers(0, 4)))
    inner = None
    if kind == "recomb":        # a third copy of the terminal inside the internal sequence
        a = int_len // 3
        internal = np.concatenate([_rand_codes(rng, a), _diverged_terminal(rng, term, 0.02, 0), _rand_codes(rng, max(200, int_len - a - term_len))])
    elif kind == "nested":      # a direct repeat of >= 400 bases, more than 500 apart, inside the internal sequence
        rep = _rand_codes(rng, int(rng.integers(400, 601)))
        gap = int(rng.integers(600, 1201))
        a = int(rng.integers(150, 400))
        internal = np.concatenate([_rand_codes(rng, a), rep, _rand_codes(rng, gap), _diverged_terminal(rng, rep, 0.02, 0),
                                   _rand_codes(rng, max(150, int_len - a - 2 * len(rep) - gap))])
        inner = ("repeat", a, a + 2 * len(rep) + gap)
    elif kind == "dirty":       # a whole element of its own family inside the internal sequence
        sub, sub_iv = _ltr_element(rng, "clean", int(rng.integers(150, 301)), int(rng.integers(1500, 2001)))
        a = int(rng.integers(300, 600))
        internal = np.concatenate([_rand_codes(rng, a), sub, _rand_codes(rng, int(rng.integers(300, 600)))])
        inner = ("inner", a, sub_iv)
    else:
        internal = _rand_codes(rng, int_len)
    over = 120 if kind == "overhang" else 0       # the annotated terminals are the middle of a longer duplicated segment
    if over:
        ol, orr = _rand_codes(rng, over), _rand_codes(rng, over)
        left_unit = np.concatenate([ol, term, orr])
        right_unit = np.concatenate([_diverged_terminal(rng, ol, 0.02, 0), right, _diverged_terminal(rng, orr, 0.02, 0)])
    else:
        left_unit, right_unit = term, right
    # guards: what lies next to the left unit is drawn from {A, C}, next to the right unit from {G, T}
    g = lambda pair: np.array(pair, dtype=np.uint8)[rng.integers(0, 2, size=_LTR_GUARD)]  # noqa: E731
    parts = [g((0, 1)), left_unit, g((0, 1)), internal, g((2, 3)), right_unit, g((2, 3))]
    at = np.cumsum([0] + [len(p) for p in parts])
    iv = dict(left=(int(at[1]) + over, int(at[2]) - over), right=(int(at[5]) + over, int(at[6]) - over))
    if inner is not None and inner[0] == "repeat":
        iv["repeat"] = (int(at[3]) + inner[1], int(at[3]) + inner[2])
    if inner is not None and inner[0] == "inner":
        iv["inner"] = {k: (int(at[3]) + inner[1] + v[0], int(at[3]) + inner[1] + v[1]) for k, v in inner[2].items()}
    return np.concatenate(parts), iv


def _scn_line(left, right, seq_id, chr_name, shift=(0, 0)):
    """the twelve space-separated fields of a candidate line from 0-based half-open terminal intervals; shift moves the annotated
    starts and ends"""
    ls, le, rs, re_ = left[0] + 1 + shift[0], left[1] + shift[1], right[0] + 1 + shift[0], right[1] + shift[1]
    return " ".join(str(x) for x in (ls, re_, re_ - ls + 1, ls, le, le - ls + 1, rs, re_, re_ - rs + 1, "95.00", seq_id, chr_name))


def make_ltr_element_genome(plan, seed=1, chrom_elements=12):
    """A genome of whole LTR elements for the `.scn` filters (util.ltr_scn_filter; tests and tools/ltr_scn_bench.py): plan = [(kind,
    count), ...] with the kinds
      "clean"     two terminals (150 .. 1 200 bases, the second 1 .. 8 % diverged with up to three short indels) around a random
                  internal sequence (1 500 .. 6 000 bases), annotated exactly;
      "recomb"    a third copy of the terminal inside the internal sequence;
      "nested"    a direct repeat of 400 .. 600 bases at 98 % identity, more than 500 apart, inside the internal sequence;
      "overhang"  the annotated terminals are the middle of a longer duplicated segment (120 more bases on both sides);
      "shifted"   annotated starts 5 bases late and ends 4 bases early;
      "dirty"     a whole smaller element (terminals of at most 300 bases) inside the internal sequence, with its own line;
      "dup"       a clean element whose line is there twice.
    Elements lie in random sequence, chrom_elements to a chromosome, in random order; the bases next to the two terminals are drawn
    from disjoint alphabets, so an alignment of the terminals ends at their boundary.
    -> dict(contigs {name: sequence}, scn (the text of the candidate table, sorted by chromosome and start), truth [dict(kind, id,
    line, name (chr-start-end of the left terminal), and by kind adjusted (the line with the true boundaries) / repeat ((start of the
    first copy, end of the second), 1-based) / inner (id of the element inside)])"""
    rng = np.random.default_rng(seed)
    kinds = [k for k, n in plan for _ in range(n)]
    for k in kinds:
        if k not in LTR_ELEMENT_KINDS:
            raise ValueError("unknown kind " + k)
    kinds = [kinds[i] for i in rng.permutation(len(kinds))]
    contigs, lines, truth = {}, [], []
    for c0 in range(0, len(kinds), chrom_elements):
        chr_name = "chr%d" % (c0 // chrom_elements + 1)
        chunk = kinds[c0:c0 + chrom_elements]
        seq = _rand_codes(rng, _LTR_SLOT * len(chunk) + 1000)
        for e, kind in enumerate(chunk):
            unit, iv = _ltr_element(rng, kind, int(rng.integers(150, 1201)), int(rng.integers(1500, 6001)))
            pos = 500 + e * _LTR_SLOT + int(rng.integers(0, 300))
            seq[pos:pos + len(unit)] = unit
            mv = lambda t: (t[0] + pos, t[1] + pos)  # noqa: E731
            seq_id = len(truth)
            left, right = mv(iv["left"]), mv(iv["right"])
            line = _scn_line(left, right, seq_id, chr_name, (5, -4) if kind == "shifted" else (0, 0))
            parts = line.split(" ")
            t = dict(kind=kind, id=seq_id, line=line, name="%s-%s-%s" % (chr_name, parts[3], parts[4]))
            if kind == "shifted":
                t["adjusted"] = _scn_line(left, right, seq_id, chr_name)
                # (the adjusted line keeps the annotated fields 0 .. 2: the reference rewrites fields 3 .. 8 only)
                t["adjusted"] = " ".join(parts[:3] + t["adjusted"].split(" ")[3:])
            if kind == "nested":
                t["repeat"] = (iv["repeat"][0] + pos + 1, iv["repeat"][1] + pos)
            truth.append(t)
            lines.append((chr_name, int(parts[0]), line))
            if kind == "dup":
                lines.append((chr_name, int(parts[0]), line))
            if kind == "dirty":
                sub = {k: mv(v) for k, v in iv["inner"].items()}
                sub_id = len(truth)
                sub_line = _scn_line(sub["left"], sub["right"], sub_id, chr_name)
                sp = sub_line.split(" ")
                t["inner"] = sub_id
                truth.append(dict(kind="inner", id=sub_id, line=sub_line, name="%s-%s-%s" % (chr_name, sp[3], sp[4])))
                lines.append((chr_name, int(sp[0]), sub_line))
        contigs[chr_name] = ASCII[seq].tobytes().decode()
    order = sorted(range(len(lines)), key=lambda k: (int(lines[k][0][3:]), lines[k][1]))
    scn = "# planted LTR elements: start end len lLTR_start lLTR_end lLTR_len rLTR_start rLTR_end rLTR_len similarity seq_id chr\n" + \
        "".join(lines[k][2] + "\n" for k in order)
    return dict(contigs=contigs, scn=scn, truth=truth)


def ltr_element_decisions(truth, recomb_lines, final_lines, dirty_dicts):
    """what util.ltr_scn_filter did with the elements of make_ltr_element_genome against what was planted: recomb_lines / final_lines =
    the lines of remove_recomb.scn / filter_terminal_align.scn.  -> {kind: [as planted, elements]} and the ids that are not"""
    final, recomb = {}, {}
    for dst, src in ((final, final_lines), (recomb, recomb_lines)):
        for line in src:
            dst.setdefault(int(line.split(" ")[10]), []).append(line)
    table, wrong = {}, []
    for t in truth:
        f, r = final.get(t["id"], []), recomb.get(t["id"], [])
        kind = t["kind"]
        if kind == "recomb":
            ok = not r and not f
        elif kind == "overhang":
            ok = r == [t["line"]] and not f
        elif kind == "shifted":
            ok = f == [t["line"], t["adjusted"]]
        elif kind == "nested":
            extra = [x.split(" ") for x in f if x != t["line"]]
            ok = t["line"] in f and any(abs(int(x[3]) - t["repeat"][0]) <= 5 and abs(int(x[7]) - t["repeat"][1]) <= 5 for x in extra)
        else:       # clean, dup, dirty, inner: the line once, nothing else
            ok = f == [t["line"]]
        # (the new line of a nested element lies inside its internal sequence, so remove_dirty_LTR names that element too)
        ok = ok and ((t["name"] in dirty_dicts) == (kind in ("dirty", "nested")))
        n = table.setdefault(kind, [0, 0])
        n[0] += bool(ok)
        n[1] += 1
        if not ok:
            wrong.append(t["id"])
    return table, wrong


# families of (copies, length of the target-site duplication or None for none) of make_ltr_library_genome's default plan
LTR_LIBRARY_PLAN = ((1, 5), (1, None), (2, 4), (2, 6), (5, 5), (1, 6))


def make_ltr_library_genome(plan=LTR_LIBRARY_PLAN, seed=1, div=0.004, edge=True):
    """A genome of FAMILIES of whole LTR elements with target-site duplications, for FiLTR's steps 4 to 8 (util.ltr_library; tests and
    tools/gen_ltr_library_fixture.py): plan = [(copies, tsd_len or None), ...].  A family is two terminals (300 .. 500 bases, TG .. CA,
    the second 1 .. 4 % apart) around an internal sequence of 1 500 .. 2 500 bases; every copy is the family's element with
    substitutions at rate div, planted between two copies of a random k-mer of tsd_len bases (None: eight C before it and bases of
    G / T after it, which share no k-mer), every copy in a slot of 6 000 bases of random sequence, eight slots to a chromosome.  With
    edge, two more single elements lie at the very start of the first and at the very end of the last chromosome (the windows of the
    structure search are cut there).  The last copy of a family of five or more has NO candidate line.
    -> dict(contigs {name: sequence}, scn (the candidate table, by chromosome and start; the identity column takes 100.00, 98.50,
    95.00, ... in turn), truth [dict(family, copy, chr, line or None, name, tsd)])"""
    rng = np.random.default_rng(seed)
    slot, per_chr = 6000, 8
    units = []
    for f, (copies, tsd) in enumerate(plan):
        term = _rand_codes(rng, int(rng.integers(300, 501)))
        term[:3] = (3, 2, 3)          # TGT .. ACA
        term[-3:] = (0, 1, 0)
        right = _diverged_terminal(rng, term, float(rng.uniform(0.01, 0.04)), 0)
        internal = _rand_codes(rng, int(rng.integers(1500, 2501)))
        element = np.concatenate([term, internal, right])
        for c in range(copies):
            body = element.copy()
            m = rng.random(len(body)) < div
            m[:_LTR_CLEAN_END] = False
            m[len(body) - _LTR_CLEAN_END:] = False
            body[m] = (body[m] + rng.integers(1, 4, size=int(m.sum())).astype(np.uint8)) & 3
            units.append(dict(family=f, copy=c, body=body, term=len(term), rterm=len(right), tsd=tsd, line=not (copies >= 5 and c == copies - 1)))
    order = [int(i) for i in rng.permutation(len(units))]
    n_chr = (len(units) + per_chr - 1) // per_chr
    contigs, lines, truth = {}, [], []
    idents = ("100.00", "98.50", "95.00", "99.20", "90.00")
    for ci in range(n_chr):
        chr_name = "chr%d" % (ci + 1)
        chunk = [units[i] for i in order[ci * per_chr:(ci + 1) * per_chr]]
        extra = []
        if edge and ci == 0:
            extra.append("start")
        if edge and ci == n_chr - 1:
            extra.append("end")
        seq = _rand_codes(rng, slot * len(chunk) + 1000)
        placed = []
        for e, u in enumerate(chunk):
            pos = 700 + e * slot + int(rng.integers(0, 200))
            body = u["body"]
            if u["tsd"] is None:
                seq[pos - 8:pos] = 1
                seq[pos + len(body):pos + len(body) + 8] = rng.integers(2, 4, size=8).astype(np.uint8)
            else:
                k = _rand_codes(rng, u["tsd"])
                seq[pos - u["tsd"]:pos] = k
                seq[pos + len(body):pos + len(body) + u["tsd"]] = k
            seq[pos:pos + len(body)] = body
            placed.append((u, pos))
        parts, shift = [seq], 0
        if "start" in extra:
            unit, iv = _ltr_element(rng, "clean", 300, 1500)
            head = unit[iv["left"][0]:iv["right"][1]]
            parts.insert(0, head)
            shift = len(head)
            placed.append((dict(family=-1, copy=0, body=head, term=iv["left"][1] - iv["left"][0], rterm=iv["right"][1] - iv["right"][0], tsd=None,
                                line=True), -shift))
        if "end" in extra:
            unit, iv = _ltr_element(rng, "clean", 300, 1500)
            tail = unit[iv["left"][0]:iv["right"][1]]
            placed.append((dict(family=-2, copy=0, body=tail, term=iv["left"][1] - iv["left"][0], rterm=iv["right"][1] - iv["right"][0], tsd=None,
                                line=True), len(seq)))
            parts.append(tail)
        for u, pos in placed:
            a = pos + shift
            n = len(u["body"])
            line = _scn_line((a, a + u["term"]), (a + n - u["rterm"], a + n), len(truth), chr_name)
            f = line.split(" ")
            f[9] = idents[len(truth) % len(idents)]
            line = " ".join(f)
            truth.append(dict(family=u["family"], copy=u["copy"], chr=chr_name, line=line if u["line"] else None, name="%s-%s-%s" % (chr_name, f[3], f[4]),
                              tsd=u["tsd"]))
            if u["line"]:
                lines.append((ci, a, line))
        contigs[chr_name] = ASCII[np.concatenate(parts)].tobytes().decode()
    lines.sort(key=lambda t: (t[0], t[1]))
    scn = "# planted LTR families: start end len lLTR_start lLTR_end lLTR_len rLTR_start rLTR_end rLTR_len similarity seq_id chr\n" + \
        "".join(t[2] + "\n" for t in lines)
    return dict(contigs=contigs, scn=scn, truth=truth)
