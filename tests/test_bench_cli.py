"""bench.py and __graft_entry__.py at the repo root: importable / runnable on a host without a GPU as far as they can go."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_help_lists_the_contract_flags():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0
    for flag in ("--gpus", "--steps", "--warmup", "--lanes", "--inflight", "--interval-optimization", "--no-cpu-baseline", "--full",
                 "--dump-outputs"):
        assert flag in out.stdout


def test_bench_isolated_pass_only_with_full():
    """--isolated-only is one of the --full measurements: asked for in a plain run it is refused before anything runs"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--isolated-only"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "--full" in out.stderr


def test_bench_dump_outputs_writes_a_fixed_float64_sample(tmp_path):
    """--dump-outputs: per-read counts of the whole step, every record of a seeded sample of reads (CIGAR offset left out) and
    their CIGAR words in record order, all float64 and exact, far below 64 MB"""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    from floxer_amd import RunResult
    rng = np.random.default_rng(5)
    n_reads, per_read = 500, 3
    raw = np.zeros(n_reads * per_read, dtype=[("read", np.uint32), ("flag", np.uint16), ("ref", np.int32), ("pos", np.uint64),
                                               ("nm", np.uint32), ("coff", np.uint64), ("clen", np.uint32)])
    raw["read"] = np.repeat(np.arange(n_reads), per_read)
    raw["flag"] = rng.choice([0, 16, 256, 272], size=len(raw))
    raw["pos"] = rng.integers(0, 3_100_000_000, size=len(raw))
    raw["nm"] = rng.integers(0, 800, size=len(raw))
    raw["clen"] = rng.integers(1, 40, size=len(raw))
    # CIGAR slabs in an order of their own, as the lanes leave them
    order = rng.permutation(len(raw))
    raw["coff"][order] = np.concatenate(([0], np.cumsum(raw["clen"][order])[:-1]))
    cig = rng.integers(0, 2**32, size=int(raw["clen"].sum()), dtype=np.uint64).astype(np.uint32)
    res = RunResult(raw, cig, np.zeros(n_reads, np.uint8))
    bench.dump_outputs(str(tmp_path / "a"), res, n_reads)
    bench.dump_outputs(str(tmp_path / "b"), res, n_reads)
    names = ("records_per_read", "skipped", "records", "cigars")
    got = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in names}
    assert all(a.dtype == np.float64 for a in got.values())
    assert all(np.array_equal(got[n], np.load(tmp_path / "b" / f"{n}.npy")) for n in names)
    assert sum(os.path.getsize(tmp_path / "a" / f"{n}.npy") for n in names) < 64 << 20
    assert got["records_per_read"].tolist() == [per_read] * n_reads and not got["skipped"].any()
    reads = np.unique(got["records"][:, 0]).astype(np.int64)
    assert len(reads) == bench.DUMP_READS
    rows = res.rows[np.isin(res.rows[:, 0], reads)]
    assert np.array_equal(got["records"], rows[:, [0, 1, 2, 3, 4, 6]].astype(np.float64))
    words = np.concatenate([cig[r[5]: r[5] + r[6]] for r in rows])
    assert np.array_equal(got["cigars"], words.astype(np.float64))


def test_bench_refuses_to_run_without_a_gpu():
    """the product has no CPU path: on a host without a HIP device bench.py stops with a message instead of falling back"""
    import torch
    if torch.cuda.is_available():
        return
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "0"], capture_output=True, text=True,
                         timeout=300, env=dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"))
    assert out.returncode != 0
    assert "MI355X" in (out.stderr + out.stdout)


def test_graft_entry_exposes_build_and_smoke():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    assert callable(g.build) and callable(g.smoke)
