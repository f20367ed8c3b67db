"""Cost of flx_partial_options (profiles/partial_alignments.txt): ms per step with the option off / on over a bench-like batch, and over
a batch with 10 % chimeras - trace launches added, share of chimeras rescued. One MI355X: python scripts/partial_cost.py"""
import sys, time, os
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import floxer_amd as F
from floxer_amd import simulate as S

GEN, NCH, N, LEN, RATE, P = 100_000_000, 4, 8192, 10000, 0.08, 0.1
pool, chroms = S.make_genome_fast(GEN // NCH, NCH, seed=7)
(rp, ro), _ = S.make_reads_fast(pool, [GEN // NCH] * NCH, N, LEN, RATE, seed=8)
t = time.time(); idx = F.fmindex(chroms, device=0); print(f"index on device: {time.time()-t:.1f} s", flush=True)
ctx = F.context(idx)
p = F.params(error_probability=P)

def step(reads, partial, timing=False):
    if timing:
        ctx.enable_kernel_timing(True); ctx.reset_kernel_stats()
    ctx.path_counters(reset=True)
    t = time.perf_counter()
    run = F.aligner(ctx, p, partial=partial).align_reads(reads)
    ms = (time.perf_counter() - t) * 1e3
    ks = ctx.kernel_stats() if timing else None
    if timing:
        ctx.enable_kernel_timing(False)
    return ms, run, ctx.path_counters(), ks

def series(name, batch, n_chim):
    rr = F.resident_reads(ctx, batch)
    step(rr, None); step(rr, F.partial_options())
    rows = {"off": [], "on": []}
    last = {}
    for i in range(5):
        for tag, po in (("off", None), ("on", F.partial_options())):
            ms, run, pc, _ = step(rr, po)
            rows[tag].append(ms); last[tag] = (run, pc)
    print(f"{name}: ms/step (run_copy included) off {' '.join(f'{x:.1f}' for x in rows['off'])} | on {' '.join(f'{x:.1f}' for x in rows['on'])}")
    print(f"{name}: median off {np.median(rows['off']):.1f} ms, on {np.median(rows['on']):.1f} ms")
    (r0, pc0), (r1, pc1) = last["off"], last["on"]
    un0 = int((r0.raw['flag'] & 4 != 0).sum()); un1 = int((r1.raw['flag'] & 4 != 0).sum())
    print(f"{name}: records off {r0.n_records} on {r1.n_records}; unmapped reads off {un0} on {un1}; partial records {pc1['partial_records']}, reads rescued {pc1['reads_rescued']}")
    if n_chim:
        flags = {}
        for rd, fl in zip(r1.raw['read'], r1.raw['flag']):
            flags.setdefault(int(rd), []).append(int(fl))
        both = sum(1 for i in range(n_chim) if any(f & 2048 for f in flags.get(i, [])))
        one = sum(1 for i in range(n_chim) if flags.get(i) and not flags[i][0] & 4 and not any(f & 2048 for f in flags[i]))
        print(f"{name}: of {n_chim} chimeras: both sides rescued {both} ({100*both/n_chim:.1f} %), one side only {one}, neither {n_chim-both-one}")
    else:
        same = r0.records() == r1.records() and (r0.cigars == r1.cigars).all()
        print(f"{name}: records and CIGAR pool identical off/on: {same}")
    k = {}
    for tag, po in (("off", None), ("on", F.partial_options())):
        _, _, _, ks = step(rr, po, timing=True)
        k[tag] = ks
    for kn in ("ed_align_trace", "ed_lastrow_min", "ed_traceback", "ed_align_exists"):
        a, b = k["off"].get(kn, dict(launches=0, device_ms=0)), k["on"].get(kn, dict(launches=0, device_ms=0))
        print(f"{name}: {kn}: launches off {a['launches']} on {b['launches']} (+{b['launches']-a['launches']}), device ms off {a['device_ms']:.1f} on {b['device_ms']:.1f}")
    rr.close()

reads = [rp[int(ro[i]): int(ro[i + 1])] for i in range(N)]
series("bench-like batch (8192 x 10 kb @ 8 %, 100 Mb, no chimeras)", (rp, ro), 0)
n_chim = N // 10
chim = []
for i in range(n_chim):
    a, b = reads[2 * i], reads[2 * i + 1]
    chim.append(np.concatenate([a[: len(a) // 2], b[len(b) // 2:]]))
series(f"batch with {n_chim} chimeras of {N} reads (10 %; halves of two simulated reads)", chim + reads[2 * n_chim:] + reads[:n_chim], n_chim)
ctx.close()
