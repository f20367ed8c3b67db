"""Consensus without a GPU (flx_consensus): the numpy reference against its own naive loop, flx_consensus_host against the reference on
random records and on pileup's special rows, the allele key's round trip, the ABI's sizes and names, the parser of floxer_consensus
through its parse-only switch, and tests/consensus_check.cpp: the rule header against a column walk under ASan + UBSan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import floxer_amd as F
from floxer_amd import capi
import consensus_ref as R
import pileup_ref as P
from test_pileup_gpu import special_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "floxer_amd", "floxer_consensus")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def same(got, want):
    assert got[0] == want[0], [(i, a[:60], b[:60]) for i, (a, b) in enumerate(zip(got[0], want[0])) if a != b][:3]
    assert len(got[1]) == len(want[1]) and got[1].tobytes() == want[1].tobytes(), (got[1][:5], want[1][:5])
    assert len(got[2]) == len(want[2]) and got[2].tobytes() == want[2].tobytes(), (got[2][:5], want[2][:5])


def batches():
    """(text, lengths, records, words, reads, options): random records at several depths and thresholds, then pileup's special rows"""
    rng = np.random.default_rng(20261021)
    out = []
    for case in range(12):
        lengths = [int(x) for x in rng.integers(1, 90, size=int(rng.integers(1, 4)))]
        rec, words = P.random_records(rng, lengths, 80 + 40 * case)
        reads = P.attach_reads(rng, rec, words)
        o = R.options(count_secondary=bool(case % 2), min_mapq=0 if case % 4 else 20, min_depth=int(rng.integers(0, 5)), min_count=int(rng.integers(0, 4)),
                      min_permille=int(rng.integers(0, 800)), mask_low_depth=case % 3 == 0)
        out.append((R.random_text(rng, sum(lengths)), lengths, rec, words, reads, o))
    lengths = [700, 40]
    rec, words, reads = R.records_with_reads(rng, special_rows() * 3)       # three copies of each, each with a read of its own
    for o in (R.options(), R.options(min_depth=1, min_count=1, min_permille=1), R.options(min_depth=2, min_count=1, min_permille=1, mask_low_depth=True)):
        out.append((R.random_text(rng, sum(lengths)), lengths, rec, words, reads, o))
    return out


BATCHES = batches()


def test_reference_against_its_naive_loop():
    n_changes = 0
    for text, lengths, rec, words, reads, o in BATCHES:
        letters, changes, al = R.consensus(text, lengths, rec, words, reads, o)
        cnt = P.counts(lengths, rec, words, reads, o)
        assert (cnt == P.counts_naive(lengths, rec, words, reads, o)).all()
        naive_letters, naive_changes = R.call_naive(text, lengths, cnt, al, o)
        assert naive_letters == letters and naive_changes.tobytes() == changes.tobytes()
        n_changes += len(changes)
        for r, n in enumerate(lengths):                                   # the letters add up: one per position that is not deleted, plus the insertions
            mine = changes[changes["ref"] == r]
            assert len(letters[r]) == n - int((mine["kind"] == R.DEL).sum()) + int(mine["length"][mine["kind"] == R.INS].sum())
    assert n_changes > 50


def test_host_rule_equals_the_reference():
    kinds = set()
    for text, lengths, rec, words, reads, o in BATCHES:
        want = R.consensus(text, lengths, rec, words, reads, o)
        same(F.consensus_host(text, lengths, rec, words, reads, R.c_options(o)), want)
        kinds |= {int(k) for k in want[1]["kind"]}
    assert kinds == {R.SUB, R.DEL, R.INS}


def column_inputs(R_rank, planes, ins=()):
    """a single position of rank R_rank between two A with the given counts, as records of one column each: planes = dict(eq, A, C, G, T,
    DEL); ins: insertion strings behind the column, one record of [= 1, I n] each (they add to eq). Returns (text, records, words, reads)."""
    text = np.array([1, R_rank, 1], dtype=np.uint8)
    rows, reads = [], []
    for name, n in planes.items():
        for _ in range(n):
            if name == "DEL":
                rows.append((0, 0, 0, 0, [R.word("=", 1), R.word("D", 1), R.word("=", 1)]))
                reads.append([1, 1])
            elif name == "eq":
                rows.append((0, 0, 1, 0, [R.word("=", 1)]))
                reads.append([R_rank if 1 <= R_rank <= 4 else 1])
            else:
                rows.append((0, 0, 1, 0, [R.word("X", 1)]))
                reads.append(["NACGT".index(name)])
    for s in ins:
        rows.append((0, 0, 1, 0, [R.word("=", 1), R.word("I", len(s))]))
        reads.append([R_rank if 1 <= R_rank <= 4 else 1] + list(s))
    rec, words = R.records_of(rows)
    return text, rec, words, [np.array(x, dtype=np.uint8) for x in reads]


def one_column(R_rank, planes, o, ins=()):
    """the host rule's outputs on such a column, checked against the reference's"""
    text, rec, words, reads = column_inputs(R_rank, planes, ins)
    got = F.consensus_host(text, [3], rec, words, reads, R.c_options(o))
    same(got, R.consensus(text, [3], rec, words, reads, o))
    return got


# (name, R, planes, options, insertions) -> (the column's letters, its change rows as (kind, alt_rank, count, cov))
COLUMNS = [
    ("tie with R keeps R", 2, dict(eq=2, A=2), R.options(min_depth=1, min_count=1, min_permille=1), (), "C", []),
    ("tie without R takes the first of A C G T DEL", 2, dict(G=2, T=2, DEL=2), R.options(min_depth=1, min_count=1, min_permille=1), (), "G", [(R.SUB, 3, 2, 6)]),
    ("tie of T and DEL takes T", 1, dict(T=2, DEL=2), R.options(min_depth=1, min_count=1, min_permille=1), (), "T", [(R.SUB, 4, 2, 4)]),
    ("cov one below min_depth is uncalled", 2, dict(A=2), R.options(min_depth=3, min_count=1, min_permille=1), (), "C", []),
    ("cov at min_depth is called", 2, dict(A=3), R.options(min_depth=3, min_count=1, min_permille=1), (), "A", [(R.SUB, 1, 3, 3)]),
    ("count one below min_count", 2, dict(A=2), R.options(min_depth=1, min_count=3, min_permille=1), (), "C", []),
    ("count at min_count", 2, dict(A=3), R.options(min_depth=1, min_count=3, min_permille=1), (), "A", [(R.SUB, 1, 3, 3)]),
    ("fraction just below min_permille", 2, dict(A=2, eq=1), R.options(min_depth=1, min_count=1, min_permille=667), (), "C", []),
    ("fraction just at min_permille", 2, dict(A=2, eq=1), R.options(min_depth=1, min_count=1, min_permille=666), (), "A", [(R.SUB, 1, 2, 3)]),
    ("R = N stays N without a call", 5, dict(eq=3), R.options(min_depth=1, min_count=1, min_permille=1), (), "N", []),
    ("R = N takes a call", 0, dict(eq=1, G=2), R.options(min_depth=1, min_count=1, min_permille=1), (), "G", [(R.SUB, 3, 2, 3)]),
    ("R = N of rank 5 under a deletion is deleted", 5, dict(DEL=2), R.options(min_depth=1, min_count=1, min_permille=1), (), "", [(R.DEL, 0, 2, 2)]),
    ("mask_low_depth writes N", 2, dict(eq=2), R.options(min_depth=3, mask_low_depth=True), (), "N", []),
    ("the defaults are 3 / 2 / 500", 2, dict(A=2, eq=1), R.options(), (), "A", [(R.SUB, 1, 2, 3)]),
    ("a DEL call with an insertion behind it", 3, dict(DEL=3, eq=0), R.options(min_depth=1, min_count=1, min_permille=1), ([1, 4], [1, 4]), "AT", [(R.DEL, 0, 3, 5), (R.INS, 0, 2, 5)]),
    ("two alleles of equal count: the smaller key", 3, dict(), R.options(min_depth=1, min_count=1, min_permille=1), ([4, 1], [2, 3], [4, 1], [2, 3]), "GCG", [(R.INS, 0, 2, 4)]),
    ("a shorter allele is the smaller key", 3, dict(), R.options(min_depth=1, min_count=1, min_permille=1), ([4, 1], [4]), "GT", [(R.INS, 0, 1, 2)]),
    ("an insertion below min_count is not applied", 3, dict(eq=2), R.options(min_depth=1, min_count=2, min_permille=1), ([4, 1],), "G", []),
]


@pytest.mark.parametrize("case", COLUMNS, ids=[c[0] for c in COLUMNS])
def test_the_call_column_by_column(case):
    _, rank, planes, o, ins, letters, rows = case
    got = one_column(rank, planes, o, ins)
    ends = "N" if o["mask_low_depth"] else "A"                            # (the neighbours are covered by the DEL records alone, or not at all)
    assert got[0][0][0] == ends and got[0][0][-1] == ends and got[0][0][1:-1] == letters, got[0]
    mine = got[1][got[1]["pos"] == 1]
    assert [(int(c["kind"]), int(c["alt_rank"]), int(c["count"]), int(c["cov"])) for c in mine] == rows, mine


def test_key_round_trip_and_the_void_key():
    rng = np.random.default_rng(3)
    text = np.array([1, 2, 3], dtype=np.uint8)
    for length in (1, 2, 31, 32, 33):
        s = [int(x) for x in rng.integers(1, 5, size=length)]
        assert length > 32 or R.unpack(R.pack(s), length) == s
        hi, lo = R.key_of(1, s)
        rec, words = R.records_of([(0, 0, 1, 0, [R.word("=", 1), R.word("I", length), R.word("=", 1)])] * 2)
        _, changes, al = F.consensus_host(text, [3], rec, words, [np.array([2] + s + [3], dtype=np.uint8)] * 2, F.consensus_options(min_depth=1))
        if length > 32:
            assert (hi, lo) == ((1 << 64) - 1, (1 << 64) - 1) and len(al) == 0 and len(changes) == 0
            continue
        assert hi == 1 << 8 | length and lo & ((1 << (64 - 2 * length)) - 1) == 0
        assert [(int(a["ref"]), int(a["pos"]), int(a["length"]), int(a["count"]), int(a["letters"])) for a in al] == [(0, 1, length, 2, lo)]
        assert F.consensus_letters_of(al[0]["letters"], length) == "".join("NACGT"[x] for x in s)
        assert [int(c["kind"]) for c in changes] == [R.INS] and int(changes[0]["letters"]) == lo
    for bad in ([1, 5], [0], []):
        assert R.key_of(1, bad)[0] == (1 << 64) - 1
    assert R.key_of(None, [1])[0] == (1 << 64) - 1
    assert R.key_of(7, [4, 4]) < R.key_of(8, [1]) and R.key_of(7, [4]) < R.key_of(7, [1, 1]) and R.key_of(7, [1, 4]) < R.key_of(7, [2, 1])


def test_symbols_sizes_and_python_names():
    L = capi.lib()
    names = [n for n in capi.EXPORTED if n.startswith("flx_consensus_")]
    header = open(os.path.join(ROOT, "include", "floxer_amd.h")).read()
    assert set(names) == {n for n in re.findall(r"\b(flx_[a-z0-9_]+)\s*\(", header) if n.startswith("flx_consensus_")}
    for name in names:
        getattr(L, name)
    assert len(names) == 15
    assert C.sizeof(capi.ConsensusOptions) == 32 and C.sizeof(capi.ConsensusChange) == 40 and C.sizeof(capi.ConsensusAllele) == 24
    assert F.CHANGE_DTYPE.itemsize == 40 and F.ALLELE_DTYPE.itemsize == 24 and F.CONSENSUS_KINDS == ("SUB", "DEL", "INS")
    o = F.consensus_options(count_secondary=True, min_mapq=7, min_depth=4, min_count=3, min_permille=250, mask_low_depth=True)
    assert (o.count_secondary, o.min_mapq, o.min_depth, o.min_count, o.min_permille, o.mask_low_depth, list(o.reserved)) == (1, 7, 4, 3, 250, 1, [0, 0])
    cap, waves, longest = F.consensus_geometry()
    assert cap >= 1 and waves == 4 and longest == 32
    with pytest.raises(F.FloxerError):                                   # no device: the host form is consensus_host
        F.consensus(text=[np.ones(5, dtype=np.uint8)], device=-1)


def test_refusals_of_the_host_rule():
    rng = np.random.default_rng(9)
    text = R.random_text(rng, 60)
    rec, words = R.records_of([(0, 0, 3, 0, [R.word("=", 20), R.word("I", 2), R.word("X", 3)])] * 3)
    rec["read"] = 0
    reads = [np.array([1] * 20 + [2, 3] + [4, 4, 4], dtype=np.uint8)]
    bad = capi.ConsensusOptions()
    bad.reserved[1] = 1
    for o in (bad, F.consensus_options(min_permille=1001)):
        with pytest.raises(F.FloxerError):
            F.consensus_host(text, [60], rec, words, reads, o)
    with pytest.raises(F.FloxerError, match="rank above 5"):
        F.consensus_host(np.full(60, 6, dtype=np.uint8), [60], rec, words, reads)
    for rows in ([(0, 0, 50, 0, [R.word("=", 11)])], [(0, 1, 0, 0, [R.word("=", 1)])], [(0, 0, 0, 0, [R.word("M", 5)])], [(0, 0, 0, 0, [R.word("S", 5), R.word("I", 1)])],
                 [(0, 0, 0, 0, [])]):
        rec2, words2, reads2 = R.records_with_reads(rng, [(0, 0, 3, 0, [R.word("=", 20)])] * 2 + rows)
        with pytest.raises(F.FloxerError):
            F.consensus_host(text, [60], rec2, words2, reads2)
    letters, changes, al = F.consensus_host(text, [60], rec, words, reads, F.consensus_options(min_depth=1))
    assert len(letters[0]) == 62 and len(al) >= 1


def tool(*args):
    env = dict(os.environ, FLX_CONSENSUS_PARSE_ONLY="1")                 # the parser alone: no device is touched, no file is opened
    return subprocess.run([TOOL] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)


def test_tool_parser(tmp_path):
    ref, reads = os.path.join(GOLDEN, "reference.fasta"), os.path.join(GOLDEN, "queries.fastq")
    fasta, tsv = str(tmp_path / "consensus.fasta"), str(tmp_path / "changes.tsv")
    base = ["--reference", ref, "--queries", reads, "--output", fasta]
    h = subprocess.run([TOOL, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert h.returncode == 0 and h.stdout == b""
    lines = h.stderr.decode().splitlines()
    options = ("reference", "queries", "output", "query-errors", "error-probability", "changes", "device", "min-depth", "min-count", "min-fraction", "mask-low-depth",
               "secondary", "min-mapq", "realign-affine", "batch-reads")
    for name in options:
        assert len([l for l in lines if re.search(rf"^\s+(-\w, )?--{name}(\s|$)", l)]) == 1, name
    assert len(lines) == 1 + len(options) and lines[0].startswith("floxer_consensus")
    good = (["-p", "0.05"], ["-e", "3"], ["-e", "2"], ["-p", "0.05", "--changes", tsv, "--device", "0", "--min-depth", "1", "--min-count", "1", "--min-fraction", "0.001"],
            ["-p", "0.05", "--device", "1023", "--min-depth", "1000000", "--min-count", "1000000", "--min-fraction", "1", "--mask-low-depth", "--secondary", "--min-mapq", "1",
             "--realign-affine", "--batch-reads", "1"], ["-p", "0.00001", "--min-mapq", "254", "--batch-reads", "16777216"], ["-p", "0.99999"], ["-e", "4096"],
            ["--error-probability=0.05", "--min-fraction=0.5"])
    for extra in good:
        r = tool(*base, *extra)
        assert r.returncode == 0 and r.stdout == b"" and b"CLI PARSER ERROR" not in r.stderr, (extra, r.stderr)
    d = dict(l.split("=", 1) for l in tool(*base, "-p", "0.05", "--min-fraction", "0.3", "--min-mapq", "5", "--mask-low-depth").stderr.decode().splitlines())
    assert (d["min-permille"], d["min-mapq"], d["mask-low-depth"], d["secondary"], d["batch-reads"], d["output"]) == ("300", "5", "1", "0", "16384", fasta)
    bad = ([], ["-e", "1"], ["-e", "4097"], ["-p", "0.000001"], ["-p", "1"], ["-p", "x"], ["-e", "-1"], ["-p", "0.05", "--device", "1024"], ["-p", "0.05", "--min-depth", "0"],
           ["-p", "0.05", "--min-depth", "1000001"], ["-p", "0.05", "--min-count", "0"], ["-p", "0.05", "--min-count", "1000001"], ["-p", "0.05", "--min-fraction", "0.0009"],
           ["-p", "0.05", "--min-fraction", "1.001"], ["-p", "0.05", "--min-mapq", "0"], ["-p", "0.05", "--min-mapq", "255"], ["-p", "0.05", "--batch-reads", "0"],
           ["-p", "0.05", "--batch-reads", "16777217"], ["-p", "0.05", "--changes", str(tmp_path / "changes.txt")], ["-p", "0.05", "--min-depth"], ["-p", "0.05", "--sam"],
           ["-p", "0.05", "--pileup", tsv], ["-p", "0.05", "stray"])
    for extra in bad:
        r = tool(*base, *extra)
        assert r.returncode == 255 and r.stderr.startswith(b"[CLI PARSER ERROR]\n") and r.stdout == b"", (extra, r.stderr)
    for args, what in ((["--queries", reads, "--output", fasta, "-p", "0.05"], b"-r/--reference is required"), (["--reference", ref, "--output", fasta, "-p", "0.05"], b"-q/--queries is required"),
                       (["--reference", ref, "--queries", reads, "-p", "0.05"], b"-o/--output is required"),
                       (["--reference", ref, "--queries", reads, "--output", str(tmp_path / "consensus.bam"), "-p", "0.05"], b"[fa,fasta]"),
                       (["--reference", reads, "--queries", reads, "--output", fasta, "-p", "0.05"], b"-r/--reference"),
                       (["--reference", ref, "--queries", ref, "--output", fasta, "-p", "0.05"], b"-q/--queries"),
                       (["--reference", str(tmp_path / "none.fa"), "--queries", reads, "--output", fasta, "-p", "0.05"], b"does not exist"),
                       (base, b"Either a fixed number of errors"), (base + ["-e", "1"], b"PEX tree leaves")):
        r = tool(*args)
        assert r.returncode == 255 and r.stderr.startswith(b"[CLI PARSER ERROR]\n") and what in r.stderr, (args, r.stderr)
    assert os.listdir(tmp_path) == []


def test_rule_header_against_a_column_walk_under_sanitizers(tmp_path):
    """tests/consensus_check.cpp: flx_consensus.hpp on random records, built with ASan + UBSan; nothing is preloaded"""
    exe = str(tmp_path / "consensus_check")
    src = os.path.join(ROOT, "tests", "consensus_check.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-o", exe, src], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
