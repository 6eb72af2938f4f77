"""CPU-side checks of bench.py: the cpu_baseline leg (the oracle chain is test / measurement infrastructure, the only
part of bench.py that may touch it) on a tiny workload, scalar and multi-process."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_cpu_baseline_leg_runs_on_a_tiny_workload():
    import torch

    import bench
    from hite_amd import synth

    w = synth.make_workload(genome_bp=2_000_000, n_tir=6, n_ltr=4, cands_per_family=2, seed=11, device=torch.device("cpu"))
    n_cand = len(w["cand_off"]) - 1
    wv = bench.host_workload(w, None, None, 0, n_cand)       # the generator's copy table
    for threads in (1, 2):
        r = bench.cpu_baseline(wv, 1.0, threads)
        assert set(r) == {"value", "unit", "cores", "kind", "sample", "reference_python_vs_c_port"}
        assert r["cores"] == threads and r["kind"] == "port" and r["unit"] == "candidates/s" and r["value"] > 0
    r = bench.cpu_baseline(wv, 0.5, 1, with_copies=True)     # + the CPU twin of the copy finder, charged per candidate
    assert r["copy_finding"]["index_s"] > 0 and r["value"] > 0
    # the twin's copy table is kept and compared with the table of the step (here: the generator's, which differs -- the
    # comparison itself is what is exercised; on the GPU box the step's table comes from the HIP finder and must agree)
    assert r["copy_tables"]["checked"] > 0 and r["copy_tables"]["copies_in_sample"] > 0


def test_coarse_cpu_worker_runs():
    """the CPU leg of the coarse block of the default bench line: the twins of stage 3.1 on one small sub-genome"""
    import bench

    dt, n_hsp, n_iv, stages, n_masked = bench._coarse_cpu_worker((5, 2))
    assert dt > 0 and n_hsp > 0 and n_iv > 0
    # stage 3.1 end to end: tandem masking, prev_TE masking, search + FMEA, flanked sequences -- every leg ran
    assert set(stages) == {"tandem", "prev_te", "search_fmea", "flank"} and all(v > 0 for v in stages.values()) and n_masked >= 0


def test_bench_shards_like_the_library():
    """--scaling strong uses hite_amd.dist.shard_candidates: the shares tile the batch"""
    import numpy as np

    from hite_amd import dist as hd

    cand_off = np.arange(0, 1010, 10)
    copy_first = np.arange(0, 303, 3)
    seen = []
    for r in range(3):
        c0, c1, (b0, b1), (k0, k1) = hd.shard_candidates(cand_off, copy_first, r, 3)
        assert (b0, b1) == (10 * c0, 10 * c1) and (k0, k1) == (3 * c0, 3 * c1)
        seen += list(range(c0, c1))
    assert seen == list(range(100))


def test_bench_refuses_to_run_without_a_gpu():
    """no CPU fallback: without a GPU the bench exits with a message instead of timing something else"""
    import subprocess

    import torch

    if torch.cuda.is_available():
        return
    rc = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "0"],
                        capture_output=True, text=True)
    assert rc.returncode != 0 and "needs a GPU" in (rc.stdout + rc.stderr)


def test_dumped_outputs_are_float_bounded_and_seeded(tmp_path):
    """--dump-outputs on a batch above the size limit: float32 / float64 arrays only, 64 MB at most, the same seeded sample on every
    call, and the consensus pieces and copy rows are those of the sampled candidates"""
    import numpy as np
    import pytest
    import torch

    import bench
    from hite_amd._lib import CALL_DTYPE

    rng = np.random.default_rng(5)
    n = bench.DUMP_MAX_ROWS + 1000
    calls = np.zeros(n, dtype=CALL_DTYPE)
    calls["is_te"] = rng.random(n) < 0.6
    calls["cons_len"] = np.where(calls["is_te"], rng.integers(50, 9000, n), 0)
    calls["cons_off"] = np.concatenate([[0], np.cumsum(calls["cons_len"])[:-1]])
    pool = rng.integers(65, 90, int(calls["cons_len"].sum()) + 64).astype(np.uint8)
    n_copies = rng.integers(0, 4, n)
    cf = np.concatenate([[0], np.cumsum(n_copies)]).astype(np.int32)
    nc = int(cf[-1])
    table = {1: cf, 2: rng.integers(0, 20, nc).astype(np.int32), 3: rng.integers(1, 10**9, nc), 4: rng.integers(1, 10**9, nc),
             5: rng.integers(0, 2, nc).astype(np.uint8), 6: rng.integers(0, 2**20, nc).astype(np.uint32)}

    class FakeCtx:
        def download(self, ptr, count, dtype):
            a = table[ptr]
            assert a.dtype == np.dtype(dtype) and len(a) == count
            return a.copy()

    merged = calls[::-1].copy()
    got = [bench.fine_outputs(FakeCtx(), calls, torch.from_numpy(pool), (nc, 1, 2, 3, 4, 5, 6), merged) for _ in range(2)]
    assert set(got[0]) == set(got[1]) and all(np.array_equal(got[0][k], got[1][k]) for k in got[0])
    a = got[0]
    ids = a["calls_candidates"].astype(np.int64)
    assert len(ids) == bench.DUMP_MAX_ROWS and np.all(np.diff(ids) > 0)
    assert np.array_equal(a["calls"][:, 5], calls["cons_len"][ids]) and np.array_equal(a["calls"][:, 6], calls["cons_off"][ids])
    assert np.array_equal(a["copies_per_candidate"], n_copies[ids])
    pick = a["consensus_candidates"].astype(np.int64)
    assert len(pick) == bench.DUMP_CONS_CANDIDATES
    off = a["consensus_off"].astype(np.int64)
    for j in (0, 7, len(pick) - 1):
        c = pick[j]
        want = pool[calls["cons_off"][c]:calls["cons_off"][c] + calls["cons_len"][c]]
        if off[j + 1] <= bench.DUMP_CONS_MAX_BASES:
            assert np.array_equal(a["consensus"][off[j]:off[j + 1]], want.astype(np.float32))
    assert len(a["consensus"]) == min(off[-1], bench.DUMP_CONS_MAX_BASES)
    rows = np.concatenate([np.arange(cf[c], cf[c + 1]) for c in pick])
    assert np.array_equal(a["copies"][:, 1], table[3][rows]) and np.array_equal(a["copies"][:, 4], table[6][rows])
    assert a["calls_all"].shape == (bench.DUMP_MAX_ROWS, 7)

    bench.write_outputs(str(tmp_path / "d"), a)
    files = sorted(os.listdir(tmp_path / "d"))
    assert files == sorted(k + ".npy" for k in a)
    back = {f[:-4]: np.load(tmp_path / "d" / f) for f in files}
    assert all(b.dtype in (np.float32, np.float64) and np.array_equal(b, a[k]) for k, b in back.items())
    assert sum(b.nbytes for b in back.values()) <= bench.DUMP_MAX_BYTES
    with pytest.raises(SystemExit):
        bench.write_outputs(str(tmp_path / "big"), {"x": np.zeros(bench.DUMP_MAX_BYTES // 8 + 1)})


def test_bench_options():
    """--full and --dump-outputs are options of the bench"""
    import subprocess

    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True)
    assert p.returncode == 0 and "--full" in p.stdout and "--dump-outputs" in p.stdout
