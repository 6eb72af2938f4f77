"""Inputs of the tests of the wide fall-back's traceback by runs (hite_amd/csrc/hite_align.hip, align_wide_tb_runs_kernel): small
deterministic pairs, built with the helpers of tests/align_limit_cases.py, that ALL end in the fall-back -- class (320, 0, .) at cap 8,
or (320, 1, 0) for the two pairs the fall-back is meant to drop.  test_wide_walk_cases.py proves that on the CPU with the twin and
reads the runs each case is named for out of the twin's ops; test_gpu_wide_walk.py sends them through both forms of the kernel.

What sends a pair to the fall-back: a gap of 45 bases (class C of align_limit_cases.py): the traceback of the kept run leaves its
64-row slice.  Every case carries one, as a deletion from the row (an up run of the walk) or an insertion into it (a left run), away
from what the case is about.

The walk runs from the last cell to the first, so "after" below is "towards the front of the sequences".

One combination the issue of this change lists cannot be built from sequences: an up run DIRECTLY behind a left run (or the
reverse). A left step and an up step next to each other cost 6; the diagonal step between the same two cells costs at most 1, so no
path the forward pass marks ever holds the two side by side. Nor does a best path hold them a few steps apart: u up steps and as
many left steps with d matching columns between them cost 6 u, the same stretch as d + u diagonal steps about 0.75 (d + u). What
pairs can show is the two kinds of run in both orders with a diagonal run of 64 or 128 between them (`K_diag_64`, `K_diag_128`,
`K_up_128_left`); the adjacent forms are walked on hand-made
bit matrices in test_host_wide_walk.py."""
from typing import NamedTuple

import numpy as np

from align_limit_cases import ACGT, FB, FB_LONGEST_CENTRE, FB_LONGEST_ROW, _ROT, insert, rnd

CAP = 8
DIAG_RUNS = (1, 63, 64, 65, 127, 128, 129)
LEFT_RUNS = (1, 63, 64, 65, 200)
SEND = 45                # the gap that sends a pair to the fall-back


class WalkCase(NamedTuple):
    name: str
    a: np.ndarray         # centre
    b: np.ndarray         # row
    dropped: bool = False
    diag: tuple = ()      # lengths of diagonal runs the twin's path must hold
    left: tuple = ()      # ... of left runs (columns of the row that face no centre base)
    up: tuple = ()        # ... of up runs (centre bases that face no row base)


def cut(b, p, n):
    return np.ascontiguousarray(np.concatenate([b[:p], b[p + n:]]))


def put(b, p, block):
    return np.ascontiguousarray(np.concatenate([b[:p], block, b[p:]]))


def clean(before, n, seed):
    """n bases none of which is `before`.  Gaps cost 3 a base whatever their length, so a gap breaks up wherever a base of the block
    it faces equals the base in front of the gap: the walk, which takes a diagonal step wherever one is on a best path, steps over
    that chance match and goes on with the gap behind it (the 45-base gaps of class C are a dozen runs each).  A block made of the
    three other letters keeps its gap in ONE run, at the place it was put."""
    three = np.array([ch for ch in ACGT if ch != before], np.uint8)
    return three[np.random.default_rng(seed).integers(0, 3, n)]


def build(a0, edits, seed=1, send=True):
    """-> (centre, row).  edits: ("del", p, n) -- the row lacks the centre's bases p .. p + n - 1, an up run of exactly n -- and
    ("ins", p, n) -- the row holds n bases more in front of the centre's base p, a left run of exactly n; positions of the centre, no
    two edits touching.  The centre's block of a deletion and the row's of an insertion are clean(the centre's base p - 1).
    send: one more deletion, of SEND bases at a quarter of the centre's length, in front of all the others."""
    a = a0.copy()
    if send:
        edits = list(edits) + [("del", len(a) // 4, SEND)]
    edits = sorted(edits, key=lambda e: -e[1])
    for x, (kind, p, n) in enumerate(edits):
        if kind == "del":
            a[p:p + n] = clean(a[p - 1], n, seed + x)
    row = a.copy()
    for x, (kind, p, n) in enumerate(edits):
        row = cut(row, p, n) if kind == "del" else put(row, p, clean(a[p - 1], n, seed + 100 + x))
    return a, row


def runs_of(ops, n):
    """(diagonal runs, left runs, up runs) of the path the ops describe, each a list of lengths, front to back.  ops[p] = row index
    | 0x8000 when centre base p faces a gap.  A left run is a stretch of row bases no centre base faces."""
    diag, left, up = [], [], []
    nxt, d, u = 0, 0, 0
    for p in range(len(ops)):
        q, gap = int(ops[p]) & 0x7FFF, int(ops[p]) >> 15
        if gap:
            if d:
                diag.append(d)
            d = 0
            u += 1
            continue
        if u:
            up.append(u)
        u = 0
        if q > nxt:
            left.append(q - nxt)
            if d:
                diag.append(d)
            d = 0
        d += 1
        nxt = q + 1
    if d:
        diag.append(d)
    if u:
        up.append(u)
    if n > nxt:
        left.append(n - nxt)
    return diag, left, up


def diag_run_cases():
    """a diagonal run of exactly k steps between two gaps: deletions on both sides (odd k), a deletion in front and an insertion
    behind (even k)"""
    out = []
    for k in DIAG_RUNS:
        p = 900
        a, b = build(rnd(200 + k, 1500), [("del", p, 5), ("del" if k % 2 else "ins", p + 5 + k, 6)])
        out.append(WalkCase("K_diag_%d" % k, a, b, diag=(k,), up=(5, SEND) + ((6,) if k % 2 else ()), left=() if k % 2 else (6,)))
    return out


def left_run_cases():
    out = []
    for r in LEFT_RUNS:
        a, b = build(rnd(300 + r, 1400), [("ins", 1000, r)])
        out.append(WalkCase("K_left_%d" % r, a, b, left=(r,), up=(SEND,)))
    return out


def neighbour_cases():
    """a left run and an up run as near to each other as a best path holds them, in the other order than K_diag_64 and K_diag_128
    have them (see the module's text): the walk meets the up run first"""
    p = 800
    a, b = build(rnd(41, 1200), [("ins", p, 9), ("del", p + 128, 7)])
    return [WalkCase("K_up_128_left", a, b, diag=(128,), left=(9,), up=(7, SEND))]


def edge_cases():
    """gaps at the very first and last columns and rows; runs that end because i or j reaches 0 inside a trip; the sending gap at
    the front (at the back the kept run's own traceback takes it: no fall-back)"""
    a0 = rnd(51, 1000)
    L = len(a0)
    out = []
    a, b = build(a0, [("ins", 0, 5), ("ins", L, 6)])
    out.append(WalkCase("K_row_longer_at_both_ends", a, b, left=(5, 6), up=(SEND,)))
    a, b = build(a0, [("del", 0, 5), ("del", L - 6, 6)])
    out.append(WalkCase("K_centre_longer_at_both_ends", a, b, up=(5, 6, SEND)))
    # i reaches 0 with 30 columns to go: the trip whose diagonal run ends at row 0; j reaches 0 with 20 rows to go
    a, b = build(a0, [("ins", 0, 30), ("del", 700, SEND)], send=False)
    out.append(WalkCase("K_i_reaches_0", a, b, diag=(700,), left=(30,), up=(SEND,)))
    a, b = build(a0, [("del", 0, 20)])
    out.append(WalkCase("K_j_reaches_0", a, b, up=(20, SEND)))
    a, b = build(a0, [("del", 0, SEND)], send=False)
    out.append(WalkCase("K_up_45_at_the_front", a, b, diag=(L - SEND,), up=(SEND,)))
    a, b = build(a0, [("ins", 0, SEND)], send=False)
    out.append(WalkCase("K_left_45_at_the_front", a, b, diag=(L,), left=(SEND,)))
    return out


def short_cases():
    """centres shorter than 64 rows (random blocks: their gaps break up) and a row shorter than 64 bases"""
    a = rnd(5, 60)
    c, r = build(rnd(5, 120), [("del", 30, 60)], send=False)
    return [WalkCase("K_centre_60_row_100", a, insert(a, 30, 8, 40)),
            WalkCase("K_centre_63_row_123", rnd(5, 63), insert(rnd(5, 63), 31, 8, 60)),
            WalkCase("K_centre_120_row_60", c, r, diag=(30, 30), up=(60,))]


def mismatch_cases():
    """stretches of mismatches and of N / lower-case / '.' bytes: diagonal steps without a match, in the row and in the centre"""
    a, b = build(rnd(61, 1300), [])
    b[700:790] = _ROT[b[700:790]]
    b[820:890] = ord("N")
    b[900:1000] |= 0x20
    b[1010:1030] = ord(".")
    out = [WalkCase("K_mismatch_n_lower_in_row", a, b, up=(SEND,))]
    a, b = build(rnd(61, 1300), [("ins", 900, SEND)], send=False)
    a[600:700] = ord("N")
    a[1100:1170] = _ROT[a[1100:1170]]
    out.append(WalkCase("K_n_and_mismatch_in_centre", a, b, left=(SEND,)))
    # a row of N alone: every column a mismatch, one diagonal run from corner to ... the 45 rows it is short of
    out.append(WalkCase("K_row_all_n", rnd(61, 400), np.full(400 - SEND, ord("N"), np.uint8), diag=(400 - SEND,), up=(SEND,)))
    return out


def dropped_cases():
    """the path leaves the fall-back's 2 048 rows: `fail` in the middle of the walk; beside each the longest pair still kept"""
    a = rnd(5, 2500)
    return [WalkCase("K_long_row_kept", a, insert(a, 1200, 8, FB_LONGEST_ROW)),
            WalkCase("K_long_row_dropped", a, insert(a, 1200, 8, FB_LONGEST_ROW + 1), dropped=True),
            WalkCase("K_long_centre_kept", insert(a, 1200, 8, FB_LONGEST_CENTRE), a),
            WalkCase("K_long_centre_dropped", insert(a, 1200, 8, FB_LONGEST_CENTRE + 1), a, dropped=True)]


def table():
    return diag_run_cases() + left_run_cases() + neighbour_cases() + edge_cases() + short_cases() + mismatch_cases() + dropped_cases()


N_MANY = 70


def many():
    """more than 64 fall-back pairs for one call: several workgroups at once, rows and centres of different lengths"""
    out = []
    for x in range(N_MANY):
        L = 300 + 7 * (x % 9)
        a, b = build(rnd(400 + x, L), [("ins" if x % 2 else "del", 40 + 2 * x, SEND)], send=False)
        out.append(WalkCase("K_many_%d" % x, a, b, left=(SEND,) if x % 2 else (), up=() if x % 2 else (SEND,)))
    return out


def is_class(c, cls):
    """whether (band words, status, certified) is what the case must end in: dropped by the fall-back, or kept from it"""
    return cls == (FB, 1, 0) if c.dropped else cls[:2] == (FB, 0)
