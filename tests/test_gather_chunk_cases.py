"""tests/gather_chunk_cases.py by the twin alone (no GPU): every table of tests/test_gpu_gather_chunks.py reaches the edge it is named
for -- rows of exactly 1, 2, 3 and 4 items, the first500 + last500 form with every pad of the list in front and behind, rows of 1 and 4
items in turn, candidates of 0 / 1 / 5 / 100 rows."""
import gather_chunk_cases as GC


def test_tables_reach_their_edges():
    GC.selfcheck()
