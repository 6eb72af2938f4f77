"""Inputs of the pairwise aligner's limit tests (hite_amd/csrc/hite_align.hip): deterministic pairs, built with numpy alone, each NAMED
FOR THE CLASS IT ENDS IN -- (band words of the run kept, status, certified) per exact cap; 320 = kept from the 64-word fall-back.
test_align_limit_cases.py proves on the CPU, with the twin (oracle/hite_oracle_msa.c) and the band-free definition
(oracle/hite_oracle_nw.c), that every pair lands in the class promised here; test_gpu_align_limits.py compares HIP with the twin on the
same pairs and asserts the tally of classes the GPU reports against the promise.

The schedule's constants that the cases are built around (hite_align_run / align_flag_kernel, twin: orc_align_pair):
  * a pair whose 4-word run is not certified is re-run from the first level of {8, 16, 32} words with 96 level >= U4 + 144, up to the
    cap, until a run is certified: U4 <= 624 starts at 8 words, <= 1392 at 16, <= 2928 at 32, beyond that the 4-word run is kept;
  * a run is certified when U <= k*.  For a pair of equal lengths whose band follows the main diagonal
    k* = KSTAR[words] = 365 / 749 / 1517 / 3053 (measured with the twin; asserted by the CPU test, used here only to name classes);
  * a traceback that leaves the 64-row slice of the run kept goes to the 64-word fall-back, whose band starts at t_0 = -1024.

Classes (the letters of the test functions):
  A  the row is the centre with k substitutions spaced evenly: U = k exactly.  Both sides of k*(4) and of the three level thresholds.
  B  A plus gradual drift -- s insertions of 8 bases, then s deletions of 8 bases further on: the band steers after the drift and the
     path stays in the slice, but the certificate's diagonal range shrinks (k* falls by 6 per diagonal lost).  Pairs kept uncertified
     from 8 and from 16 words, pairs escalated twice (8 -> 16, 16 -> 32).
  C  A plus one long insertion: the traceback leaves the slice, the fall-back takes over -- after a kept run of 4, 8, 16 and 32
     words; the longest insertion the fall-back still aligns and the next (the row is dropped); centres below 1024 and below 64 rows.
  D  geometry: lengths around the strip of 16 columns and the 64-strip round of the lane-parallel traceback, the window limit of
     32 767 columns, N runs, '.' and lower-case pads inside a pair that reaches 8 words.
  E  launch grains: lists of 1 .. 129 pairs that all reach 8 words, of 1 .. 65 that reach 16 and 32.
  F  one centre whose rows end in every class at once."""
from typing import NamedTuple

import numpy as np

CAPS = (0, 8, 16, 32)
FB = 64 | 0x100
KSTAR = {4: 365, 8: 749, 16: 1517, 32: 3053}       # certificate bound of an equal-length pair on the main diagonal
LEVEL_MAX_U = {8: 624, 16: 1392, 32: 2928}          # largest U4 that starts at / is allowed this level: 96 level - 144

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_ROT = np.zeros(256, np.uint8)
_ROT[list(b"ACGT")] = list(b"CGTA")


class Case(NamedTuple):
    name: str
    a: np.ndarray        # centre
    b: np.ndarray        # row
    cls: dict            # exact cap -> (band words of the run kept, status, certified)
    U: object = None     # the cost, where the construction fixes it
    fb_from: object = None     # fall-back cases: exact cap -> band words of the run whose traceback left the slice
    nw_pair: bool = True       # False: the definition's full matrix is too large (the two pairs at the window limit only)


def rnd(seed, n):
    return ACGT[np.random.default_rng(seed).integers(0, 4, n)]


def subs(a, k):
    """a with k substitutions spaced evenly (each base rotated to the next letter)"""
    b = a.copy()
    if k:
        pos = np.linspace(3, len(a) - 4, k).astype(np.int64)
        assert len(set(pos.tolist())) == k
        b[pos] = _ROT[b[pos]]
    return b


def insert(b, p, seed, n):
    return np.ascontiguousarray(np.concatenate([b[:p], rnd(seed, n), b[p:]]))


def drift(a, k, n_ins, n_del, ins0, del0, step, seed, w=8):
    """subs(a, k), then n_del deletions of w bases at del0 - step i and n_ins insertions of w random bases at ins0 - step i: applied
    from the highest index down, so that every edit hits its stated index of the centre"""
    rng = np.random.default_rng(seed)
    b = subs(a, k)
    for i in range(n_del):
        p = del0 - step * i
        b = np.concatenate([b[:p], b[p + w:]])
    for i in range(n_ins):
        p = ins0 - step * i
        b = np.concatenate([b[:p], ACGT[rng.integers(0, 4, w)], b[p:]])
    return np.ascontiguousarray(b)


def _by_caps(*cls):
    return dict(zip(CAPS, cls))


def class_of_u(U):
    """class per cap of an equal-length pair on the main diagonal with U4 = U (class A, and the pairs of D and E built like it)"""
    out = {}
    for cap in CAPS:
        c = (4, 0, int(U <= KSTAR[4]))
        if U > KSTAR[4] and cap >= 8 and U <= LEVEL_MAX_U[cap]:
            lvl = min(l for l in (8, 16, 32) if U <= LEVEL_MAX_U[l])
            assert U <= KSTAR[lvl]
            c = (lvl, 0, 1)
        out[cap] = c
    return out


# ---- A -------------------------------------------------------------------------------------------------------------------------
THRESHOLDS = ((365, 366), (624, 625), (1392, 1393), (2928, 2929))


def class_a():
    out = []
    for lo, hi in THRESHOLDS:
        a = rnd(5, 3 * hi + 8)          # the shortest centre that keeps hi substitutions 3 apart; both sides share it
        for k in (lo, hi):
            out.append(Case("A_u%d" % k, a, subs(a, k), class_of_u(k), U=k))
    # both orientations: two bases less at the end of the row (n < m) or of the centre (n > m) -- a gap of two, U = k + 6 or one less
    for k in (500, 1000, 1450):
        a = rnd(50 + k, 3 * k + 40)
        b = subs(a, k)
        c = class_of_u(k + 6)
        out.append(Case("A_u%d_short_row" % k, a, b[:-2], c))
        out.append(Case("A_u%d_short_centre" % k, a[:-2], b, c))
    return out


# ---- B -------------------------------------------------------------------------------------------------------------------------
def class_b():
    a = rnd(5, 4000)
    d = lambda k, ni, nd: drift(a, k, ni, nd, 1500, 3500, 150, 6)      # noqa: E731
    return [
        # kept uncertified from 8 words at cap 8; at cap 16 the 8-word run is not certified either: a SECOND wide run (16 words)
        Case("B_s8_k150", a, d(150, 8, 8), _by_caps((4, 0, 0), (8, 0, 0), (16, 0, 1), (16, 0, 1))),
        Case("B_s10_k100", a, d(100, 10, 10), _by_caps((4, 0, 0), (8, 0, 0), (16, 0, 1), (16, 0, 1))),
        Case("B_s8_k150_long_row", a, d(150, 8, 7), _by_caps((4, 0, 0), (8, 0, 0), (16, 0, 1), (16, 0, 1))),
        Case("B_s8_k150_short_row", a, d(150, 7, 8), _by_caps((4, 0, 0), (8, 0, 0), (16, 0, 1), (16, 0, 1))),
        # starts at 16 words: certified there ...
        Case("B_s8_k800", a, d(800, 8, 8), _by_caps((4, 0, 0), (4, 0, 0), (16, 0, 1), (16, 0, 1))),
        # ... or kept uncertified from 16 words at cap 16 and escalated 16 -> 32 at cap 32
        Case("B_s8_k900", a, d(900, 8, 8), _by_caps((4, 0, 0), (4, 0, 0), (16, 0, 0), (32, 0, 1))),
        Case("B_s8_k1000", a, d(1000, 8, 8), _by_caps((4, 0, 0), (4, 0, 0), (16, 0, 0), (32, 0, 1))),
        Case("B_s8_k900_long_row", a, d(900, 8, 7), _by_caps((4, 0, 0), (4, 0, 0), (16, 0, 0), (32, 0, 1))),
        Case("B_s8_k950_long_row", a, d(950, 8, 7), _by_caps((4, 0, 0), (4, 0, 0), (16, 0, 0), (32, 0, 1))),
        Case("B_s8_k950_short_row", a, d(950, 7, 8), _by_caps((4, 0, 0), (4, 0, 0), (16, 0, 0), (32, 0, 1))),
        # U == k* of the 16-word run, to the unit (1 229): certified; one more (the long row above: 1 230) is not
        Case("B_s8_k900_short_row_u_is_kstar", a, d(900, 7, 8), _by_caps((4, 0, 0), (4, 0, 0), (16, 0, 1), (16, 0, 1)), U=1229),
    ]


# pairs that run TWO wide levels: name -> (cap, the two levels)
ESCALATED_TWICE = {"B_s8_k150": (16, (8, 16)), "B_s10_k100": (16, (8, 16)), "B_s8_k150_long_row": (16, (8, 16)),
                   "B_s8_k150_short_row": (16, (8, 16)), "B_s8_k900": (32, (16, 32)), "B_s8_k1000": (32, (16, 32)),
                   "B_s8_k900_long_row": (32, (16, 32)), "B_s8_k950_long_row": (32, (16, 32)), "B_s8_k950_short_row": (32, (16, 32))}


# ---- C -------------------------------------------------------------------------------------------------------------------------
FB_LONGEST_ROW, FB_LONGEST_CENTRE = 1020, 1024     # the longest insertion into 2 500 bases that the fall-back aligns (long row / long centre)


def class_c():
    out = []
    kept = _by_caps((FB, 0, 1), (FB, 0, 1), (FB, 0, 1), (FB, 0, 1))
    # substitutions + one 45-base insertion in the middle; the run kept before the fall-back is that of the schedule without it
    for k, frm in ((0, (4, 4, 4, 4)), (120, (4, 8, 8, 8)), (400, (4, 8, 8, 8)), (700, (4, 4, 16, 16)), (1500, (4, 4, 4, 32))):
        L = max(3 * k + 8, 1000)
        a = rnd(5, L)
        b = insert(subs(a, k), L // 2, 7, 45)
        out.append(Case("C_k%d_long_row" % k, a, b, kept, U=135 if k == 0 else None, fb_from=_by_caps(*frm)))
        out.append(Case("C_k%d_long_centre" % k, b, a, kept, U=135 if k == 0 else None, fb_from=_by_caps(*frm)))
    # the fall-back's own limit: its band starts 1024 rows above the diagonal and cannot move faster than the steering allows
    a = rnd(5, 2500)
    drop = _by_caps((FB, 1, 0), (FB, 1, 0), (FB, 1, 0), (FB, 1, 0))
    four = _by_caps(4, 4, 4, 4)
    b = insert(a, 1200, 8, FB_LONGEST_ROW)
    out.append(Case("C_limit_long_row_kept", a, b, kept, U=3 * FB_LONGEST_ROW, fb_from=four))
    out.append(Case("C_limit_long_row_dropped", a, insert(a, 1200, 8, FB_LONGEST_ROW + 1), drop, fb_from=four))
    b = insert(a, 1200, 8, FB_LONGEST_CENTRE)
    out.append(Case("C_limit_long_centre_kept", b, a, _by_caps((FB, 0, 0), (FB, 0, 0), (FB, 0, 0), (FB, 0, 0)), U=3 * FB_LONGEST_CENTRE, fb_from=four))
    out.append(Case("C_limit_long_centre_dropped", insert(a, 1200, 8, FB_LONGEST_CENTRE + 1), a, drop, fb_from=four))
    out.append(Case("C_ins1100_long_row_dropped", a, insert(a, 1200, 8, 1100), drop, fb_from=four))
    out.append(Case("C_ins1100_long_centre_dropped", insert(a, 1200, 8, 1100), a, drop, fb_from=four))
    # centres below 1024 rows (the fall-back band holds virtual rows to its end) and below 64 rows
    a = rnd(5, 900)
    out.append(Case("C_m900_long_row", a, insert(a, 450, 8, 45), kept, U=135, fb_from=four))
    out.append(Case("C_m945_long_centre", insert(a, 450, 8, 45), a, kept, U=135, fb_from=four))
    a = rnd(5, 60)
    out.append(Case("C_m60_long_row", a, insert(a, 30, 8, 40), kept, U=120, fb_from=four))
    a = rnd(5, 63)
    out.append(Case("C_m63_long_row", a, insert(a, 31, 8, 60), kept, U=180, fb_from=four))
    return out


# ---- D -------------------------------------------------------------------------------------------------------------------------
EDGES = ((15, 16, 17), (31, 32, 33), (511, 512, 513), (1023, 1024, 1025))
D_CAPS = (0, 8)


def class_d():
    out = []
    M = rnd(21, 1100)
    for g in EDGES:
        for m in g:
            for n in g:
                out.append(Case("D_m%d_n%d" % (m, n), M[:m], subs(M[:n], max(1, n // 40)), _by_caps(*[(4, 0, 1)] * 4)))
    # a row far shorter than half the centre cannot be reached by a band that moves 8 rows in 4 columns: infeasible, dropped.  The
    # longest such row and the next, which is aligned (found with the twin), for a centre of 64 and of 400
    for m, n in ((40, 16), (64, 28), (400, 196), (1025, 480)):
        out.append(Case("D_too_short_m%d_n%d" % (m, n), M[:m], M[:n], _by_caps(*[(4, 2, 0)] * 4)))
    out.append(Case("D_just_long_enough_m64_n29", M[:64], M[:29], _by_caps(*[(4, 0, 1)] * 4)))
    out.append(Case("D_just_long_enough_m400_n197", M[:400], M[:197], _by_caps(*[(FB, 0, 1)] * 4)))
    for L in (1024, 1025):               # (380 substitutions in 1 024 columns are 2 or 3 apart: U = 380 all the same, says the definition)
        out.append(Case("D_u380_m%d" % L, M[:L], subs(M[:L], 380), class_of_u(380), U=380))
    # N runs, '.' and lower-case bytes INSIDE a pair that reaches 8 words (decode_bases4 of the lane kernels, base_mask elsewhere)
    A = rnd(11, 1200)
    b0 = subs(A, 380)
    wide = class_of_u(380)
    b = b0.copy(); b[500:530] = ord("N")
    out.append(Case("D_n_run_in_row", A, b, wide))
    a = A.copy(); a[700:740] = ord("N")
    out.append(Case("D_n_run_in_centre", a, b0, wide))
    b = b0.copy(); b[300:310] = ord(".")
    out.append(Case("D_dots", A, b, wide))
    b = b0.copy(); b[600:640] |= 0x20
    out.append(Case("D_lower_case", A, b, wide, U=380))         # a lower-case byte is its base: the cost of the pair without them
    b = b0.copy(); b[500:530] = ord("N"); b[300:310] = ord("."); b[600:640] |= 0x20; b[3:9] = ord("."); b[-9:-2] |= 0x20
    out.append(Case("D_all_of_them", A, b, wide))
    return out


def class_d_window_limit():
    """32 767 columns (AL_KBINS strips): compared with the twin and with the definition's COST; the definition's traceback keeps the
    whole matrix, 4 GB here -- the one omission"""
    a = rnd(22, 32767)
    b = subs(a, 200)
    return [Case("D_32767_32767", a, b, _by_caps(*[(4, 0, 1)] * 4), U=200, nw_pair=False),
            Case("D_32767_32764", a, b[:32764], _by_caps(*[(4, 0, 1)] * 4), nw_pair=False)]


# ---- E -------------------------------------------------------------------------------------------------------------------------
GRAINS_8 = (1, 31, 32, 33, 63, 64, 65, 129)       # align_fwd8_pair_kernel: 32 pairs per block; align_fwd_lanes_kernel<8> / <4>: 8 / 16 per wave
GRAINS_WIDE = (1, 63, 64, 65)                     # align_fwd_kernel<16 | 32>: 64 pairs per block


def _variants(A, B, count):
    """count pairs cut from (A, B): lengths 0 .. 42 columns below the full one so that the length sort interleaves them, and up to
    two columns less in the row (odd i) or in the centre (even i)"""
    out = []
    for i in range(count):
        L = len(A) - (17 * i) % 43
        d = i % 3
        a, b = A[:L], B(A[:L]) if callable(B) else B[:L]
        out.append((a, b[:L - d]) if i % 2 else (a[:L - d], b))
    return out


def grains_8():
    """129 pairs of about 1 200 columns that all end in (8, 0, 1) at cap 8"""
    return [Case("E8_%d" % i, a, b, {8: (8, 0, 1), 32: (8, 0, 1)}) for i, (a, b) in enumerate(_variants(rnd(11, 1200), lambda a: subs(a, 380), 129))]


def grains_16():
    """65 pairs of about 2 200 columns that all end in (16, 0, 1) at cap 32"""
    return [Case("E16_%d" % i, a, b, {32: (16, 0, 1)}) for i, (a, b) in enumerate(_variants(rnd(12, 2200), lambda a: subs(a, 700), 65))]


def grains_32():
    """65 pairs of unrelated random sequences of about 2 500 columns (U about 1 690): all end in (32, 0, 1) at cap 32"""
    return [Case("E32_%d" % i, a, b, {32: (32, 0, 1)}) for i, (a, b) in enumerate(_variants(rnd(13, 2500), rnd(14, 2500), 65))]


def mixed_wave():
    """pairs of 3 000 columns that reach 8 words beside pairs of 40 certified at once: one wave holds pairs that end in different strips"""
    a = rnd(15, 3000)
    long8 = {8: (8, 0, 1)}
    out = [Case("E_mix_3000", a, subs(a, 380), long8, U=380), Case("E_mix_2990", a[:2990], subs(a, 500), long8)]
    for i in range(6):
        s = rnd(160 + i, 40 + i)
        out.append(Case("E_mix_%d" % (40 + i), s, subs(s, 2), {8: (4, 0, 1)}, U=2))
    out.append(Case("E_mix_2950", a[:2950], subs(a[:2950], 400), long8, U=400))
    return out


# ---- F -------------------------------------------------------------------------------------------------------------------------
F_CAP = 32


def one_centre_many_fates():
    """-> (groups, classes per group at cap 32): group 0 has rows that end at 4, 8, 16 and 32 words, uncertified twice over, in the
    fall-back (kept certified, kept uncertified, dropped) and dropped as too short; group 1, beside it, loses no row"""
    A = rnd(31, 4600)
    fb = insert(subs(A, 50), 2300, 32, 45)
    g0 = [A, subs(A, 100), subs(A, 500), subs(A, 1000), subs(A, 1450), fb, insert(A, 2300, 33, 1100), A[:2000],
          drift(A, 150, 8, 8, 1500, 3500, 150, 6), drift(A, 900, 8, 8, 1500, 3500, 150, 6), A[1000:3290], A[:2300], subs(A, 3000)]
    c0 = ((4, 0, 1), (8, 0, 1), (16, 0, 1), (32, 0, 1), (FB, 0, 1), (FB, 1, 0), (4, 2, 0),
          (16, 0, 1), (32, 0, 1), (4, 2, 0), (FB, 0, 0), (4, 0, 0))
    B = rnd(34, 1300)
    g1 = [B, subs(B, 30), subs(B, 400), insert(subs(B, 20), 650, 35, 45), subs(B, 366)[:-1]]
    c1 = ((4, 0, 1), (8, 0, 1), (FB, 0, 1), (8, 0, 1))
    return [g0, g1], [c0, c1]


def tally(cases, cap):
    out = {}
    for c in cases:
        out[c.cls[cap]] = out.get(c.cls[cap], 0) + 1
    return out
