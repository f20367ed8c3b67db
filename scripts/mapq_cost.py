#!/usr/bin/env python3
"""What the mapping quality option costs (profiles/mapq_cli.txt), in the setup of profiles/output_options_cli.txt: a uniform 253 MB
reference (5 x 50 Mb) and reads of 10 kb at 8 %.
  library: flx_align_reads_resident[_with_options] on 16384 resident reads, one call at a time, the four forms (plain, -D, -Q,
           -D -N 1 -Q) interleaved over ROUNDS rounds after one warm-up call each; the clock holds the call alone
  CLI:     FASTQ -> BAM at default flags, 65,536 reads, 16 I/O threads, the same four forms (skipped with --no-cli)
    python3 scripts/mapq_cost.py [--no-cli] [--rounds 7] > profiles/mapq_cli.txt"""
import argparse
import ctypes as C
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import floxer_amd as F                      # noqa: E402
from floxer_amd import capi, simulate as S  # noqa: E402


def library(rounds):
    pool, chroms = S.make_genome_fast(50_000_000, 5, seed=7)
    idx = F.fmindex(chroms, device=0)
    ctx = F.context(idx)
    (rp, ro), _ = S.make_reads_fast(pool, [len(c) for c in chroms], 16384, 10000, 0.08, seed=8)
    rr = F.resident_reads(ctx, (rp, ro))
    p = F.params(error_probability=0.08)
    L = capi.lib()
    forms = [("plain", None), ("-D", F.output_options(True)), ("-Q", F.output_options(mapq=True)),
             ("-D -N 1 -Q", F.output_options(True, 1, True))]
    ms = {name: [] for name, _ in forms}
    records = {}
    for rnd in range(rounds + 1):
        for name, opt in forms:
            run = C.c_void_p()
            t0 = time.perf_counter()
            if opt is None:
                rc = L.flx_align_reads_resident(ctx.h, C.byref(p), rr.h, C.byref(run))
            else:
                rc = L.flx_align_reads_resident_with_options(ctx.h, C.byref(p), rr.h, C.byref(opt), C.byref(run))
            dt = (time.perf_counter() - t0) * 1e3
            capi.check(rc)
            records[name] = L.flx_run_num_records(run)
            L.flx_run_free(run)
            if rnd:
                ms[name].append(dt)
    for name, _ in forms:
        v = sorted(ms[name])
        med = v[len(v) // 2]
        print(f"library, {name}: step median {med:.1f} ms (min {v[0]:.1f}, max {v[-1]:.1f}, {rounds} rounds) -> {16384 / med * 1e3:.0f} reads/s, "
              f"{records[name] / 16384:.2f} records per read", flush=True)
    rr.close()
    ctx.close()


def cli():
    w = tempfile.mkdtemp(prefix="flx_mapq_cost_")
    try:
        binp = os.path.join(ROOT, "floxer_amd")
        fa, fq = os.path.join(w, "g.fasta"), os.path.join(w, "r.fastq")
        subprocess.run([os.path.join(binp, "simulated_dataset"), "create", "--genomes", fa, "--reads", fq, "-c", "50000000", "-n", "5", "-l", "10000",
                        "-m", "65536", "-e", "0.08", "-s", "7", "--revcomp-fraction", "0.5"], check=True, timeout=600,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        for name, extra in [("index_build", []), ("plain", []), ("-D", ["-D"]), ("-Q", ["-Q"]), ("-D -N 1 -Q", ["-D", "-N", "1", "-Q"]),
                            ("plain again", [])]:
            out = os.path.join(w, "o.bam")
            t0 = time.time()
            r = subprocess.run([os.path.join(binp, "floxer"), "--reference", fa, "--queries", fq, "--output", out, "--error-probability", "0.08",
                                "--index", os.path.join(w, "g.index"), "--threads", "16", *extra], stderr=subprocess.PIPE, stdout=subprocess.DEVNULL,
                               timeout=600, env=dict(os.environ, FLX_CLI_PROFILE="1", FLX_WRITER_PROFILE="1"))
            wall = time.time() - t0
            err = r.stderr.decode()
            if r.returncode != 0:
                print(f"CLI, {name}: failed\n{err[-2000:]}")
                sys.exit(1)                                   # nothing more is started after a failed run
            align = float(re.search(r"finished aligning successfully in ([0-9.]+) seconds", err).group(1))
            counts = re.search(r"\((\d+) queries, (\d+) records\)", err)
            print(f"CLI, {name}: wall {wall:.1f} s, aligning phase {align:.2f} s -> {65536 / align:.0f} reads/s end to end, "
                  f"{counts.group(2)} records, BAM {os.path.getsize(out)} bytes", flush=True)
            for line in err.splitlines():
                if "flx writer profile" in line:
                    print(line, flush=True)
    finally:
        shutil.rmtree(w, ignore_errors=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-cli", action="store_true")
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    library(a.rounds)
    if not a.no_cli:
        cli()
