"""TEST INFRASTRUCTURE: the CPU twin of hite_msa_subcluster (include/hite_gpu.h, "sub-clusters of an alignment"), a plain statement
of the definition: per pair of rows the integer counts (diff, n), ONE binary64 compare, and the ordered pass over the rows.
    n    = columns where either row is not a gap (byte 45 and nothing else)
    diff = columns where the rows differ as bytes (a column where both are gaps never counts)
    x matches y  <=>  n > 0 and float(diff) <= cutoff * float(n)
Rows are visited in order; a row joins the first leader (in leader order) it matches, else it becomes the next leader."""
import numpy as np

GAP = 45


def as_matrix(al):
    """an alignment as Context.msa_subcluster takes it (list of equal-length byte strings / str, or a 2-D uint8 array) -> 2-D uint8"""
    if isinstance(al, np.ndarray):
        assert al.ndim == 2
        return np.ascontiguousarray(al, dtype=np.uint8)
    rows = [r.encode("latin-1") if isinstance(r, str) else bytes(r) for r in al]
    if not rows:
        return np.zeros((0, 0), dtype=np.uint8)
    assert all(len(r) == len(rows[0]) for r in rows)
    return np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), len(rows[0]))


def pair_counts(x, y):
    """-> (diff, n) of two rows (1-D uint8)"""
    return int((x != y).sum()), int(((x != GAP) | (y != GAP)).sum())


def matches(diff, n, cutoff):
    return n > 0 and float(diff) <= float(cutoff) * float(n)


def match_row(m, r, leaders, cutoff):
    """bool per leader: row r of m matches it (the counts of all leaders at once, the compare in binary64)"""
    if not leaders:
        return np.zeros(0, dtype=bool)
    lead = m[leaders]
    diff = (lead != m[r]).sum(axis=1).astype(np.int64)
    n = ((lead != GAP) | (m[r] != GAP)).sum(axis=1).astype(np.int64)
    return (n > 0) & (diff.astype(np.float64) <= np.float64(cutoff) * n.astype(np.float64))


def sub_of_row(al, cutoff=0.2):
    """-> (per row the index of its sub-cluster, number of sub-clusters)"""
    m = as_matrix(al)
    leaders, sub = [], []
    for r in range(m.shape[0]):
        ok = np.nonzero(match_row(m, r, leaders, cutoff))[0]
        if len(ok):
            sub.append(int(ok[0]))
        else:
            sub.append(len(leaders))
            leaders.append(r)
    return sub, len(leaders)


def groups(sub, n_sub):
    out = [[] for _ in range(n_sub)]
    for r, k in enumerate(sub):
        out[k].append(r)
    return out


def subcluster(al, cutoff=0.2):
    """-> list of lists of row indices, sub-clusters in order of their leaders (the value Context.msa_subcluster gives per alignment)"""
    return groups(*sub_of_row(al, cutoff))


def chunked(al, cutoff, B):
    """the chunked form (hite_subcluster.hip): phase A against the leaders born before the chunk, phase B the match bits inside the
    chunk and one ordered pass over the rows phase A left open"""
    m = as_matrix(al)
    R = m.shape[0]
    leaders, sub = [], [0] * R
    for r0 in range(0, R, B):
        rows = list(range(r0, min(R, r0 + B)))
        best = []
        for r in rows:                                    # phase A: independent of each other
            ok = np.nonzero(match_row(m, r, leaders, cutoff))[0]
            best.append(int(ok[0]) if len(ok) else None)
        bits = [[matches(*pair_counts(m[i], m[j]), cutoff) for j in rows[:k]] for k, i in enumerate(rows)]   # phase B, all pairs
        born = {}                                         # chunk position -> sub-cluster of a leader born here
        for k, r in enumerate(rows):
            if best[k] is not None:
                sub[r] = best[k]
                continue
            hit = [j for j in range(k) if j in born and bits[k][j]]
            if hit:
                sub[r] = born[hit[0]]
            else:
                born[k] = sub[r] = len(leaders)
                leaders.append(r)
    return groups(sub, len(leaders))
