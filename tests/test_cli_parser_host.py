"""The command line's parser without a GPU. The --help text and every refusal (argv, stderr, return code) were recorded from the CLI as
it stood before its option table was introduced (tests/golden/cli_help.txt, cli_rejected.json: every message of the parser at least once,
every range from both sides, and doubly wrong command lines that pin the order of the checks); the parser has to repeat them byte for
byte. The accepted command lines, one per option at least, and the parser's dump (FLX_CLI_PARSE_ONLY=options: one long-id=value line per
row of the table) need no recording: what they expect follows from the argv."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "floxer_amd", "floxer")
GOLD = os.path.join(ROOT, "tests", "golden")

with open(os.path.join(GOLD, "cli_rejected.json")) as _f:
    REJECTED = json.load(_f)


def run(argv, cwd, mode):
    env = dict(os.environ, FLX_CLI_PARSE_ONLY=mode)
    return subprocess.run([EXE, *argv], cwd=cwd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def test_help_is_the_recorded_text():
    r = subprocess.run([EXE, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    with open(os.path.join(GOLD, "cli_help.txt"), "rb") as f:
        assert (r.returncode, r.stdout, r.stderr) == (0, b"", f.read())
    h = subprocess.run([EXE, "-r", "x", "-h"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)       # wherever it stands, before anything is judged
    assert (h.returncode, h.stdout, h.stderr) == (0, b"", r.stderr)


def test_rejected_command_lines_get_the_recorded_message():
    assert len(REJECTED) >= 200
    before = sorted(os.listdir(GOLD))
    for case in REJECTED:                       # (relative paths from tests/golden, so that no message holds a path of the machine)
        r = run(case["argv"], GOLD, "1")
        assert (r.returncode, r.stdout, r.stderr.decode()) == (case["rc"], b"", case["stderr"]), case["argv"]
        assert case["rc"] == 255 and case["stderr"].startswith("[CLI PARSER ERROR]\n")
    assert sorted(os.listdir(GOLD)) == before


# every option in a command line that holds: (what follows the base, the output files it names)
ACCEPTED = [
    (["-i", "x.index"], []), (["-l", "run.log"], []), (["-c"], []), (["-e", "5"], []), (["-e", "0", "-s", "0"], []), (["-e", "4096"], []), (["-p", "0.00001"], []),
    (["-p", "0.99999"], []), (["-s", "3"], []), (["-M", "7", "-m", "7"], []), (["-m", "0"], []), (["-g", "errors_first"], []), (["-g", "none"], []), (["-g", "count_first"], []),
    (["-y", "full_groups"], []), (["-y", "first_reported"], []), (["-y", "round_robin"], []), (["-C", "3"], []), (["-E"], []), (["-b"], []), (["-I"], []), (["-v", "0.5"], []),
    (["-v", "-1"], []), (["-d"], []), (["-u", "1"], []), (["-w"], []), (["-t", "1"], []), (["-t", "4096"], []), (["-x", "0"], []), (["-x", "60"], []), (["-S", "terminal"], []),
    (["-S", "stats.toml", "-H", "simulated"], ["stats.toml"]), (["-H", "real_nanopore"], []), (["-G", "0,1"], []), (["-D"], []), (["-N", "1"], []), (["-Q"], []),
    (["--md-tag"], []), (["--cs-tag"], []), (["--cs-tag-long"], []), (["--partial-alignments"], []), (["--partial-alignments", "--partial-min-span", "1", "--partial-max", "65535"], []),
    (["--partial-alignments", "--partial-min-span", "100000", "--partial-max", "1"], []), (["--partial-alignments", "--partial-extend"], []),
    (["--partial-alignments", "--partial-extend", "--partial-extend-weight", "1", "--partial-extend-xdrop", "1073741824", "--partial-extend-max-errors", "4093"], []),
    (["--partial-alignments", "--partial-extend", "--partial-extend-weight", "65535", "--partial-extend-xdrop", "1", "--partial-extend-max-errors", "1"], []),
    (["--partial-alignments", "--sa-tag"], []), (["--partial-alignments", "--split-tails", "-N", "1"], []),
    (["--partial-alignments", "--split-tails", "-N", "1", "--split-tails-weight", "65535", "--split-tails-xdrop", "1", "--split-tails-min-rows", "524287"], []),
    (["--partial-alignments", "--split-tails", "-N", "1", "--split-tails-weight", "1", "--split-tails-xdrop", "1073741824", "--split-tails-min-rows", "1"], []),
    (["--left-align-indels"], []), (["--realign-affine"], []),
    (["--realign-affine", "--realign-match", "1", "--realign-mismatch", "255", "--realign-gap-open", "255", "--realign-gap-extend", "1", "--realign-band", "1024"], []),
    (["--realign-affine", "--realign-match", "255", "--realign-mismatch", "1", "--realign-gap-open", "1", "--realign-gap-extend", "255", "--realign-band", "1"], []),
    (["--coverage", "c.bedgraph"], ["c.bedgraph"]), (["--coverage-summary", "s.tsv"], ["s.tsv"]), (["--coverage-windows", "w.tsv", "--coverage-window", "1"], ["w.tsv"]),
    (["--coverage", "c.bedgraph", "--coverage-deletions", "--coverage-secondary", "--coverage-zero", "-Q", "--coverage-min-mapq", "1"], ["c.bedgraph"]),
    (["--coverage-summary", "s.tsv", "-Q", "--coverage-min-mapq", "254"], ["s.tsv"]), (["--pileup", "p.tsv"], ["p.tsv"]),
    (["--pileup", "p.tsv", "--pileup-min-depth", "1", "--pileup-min-count", "4294967295", "--pileup-min-fraction", "1", "--pileup-secondary", "-Q", "--pileup-min-mapq", "1"], ["p.tsv"]),
    (["--pileup", "p.tsv", "--pileup-min-depth", "4294967295", "--pileup-min-count", "1", "--pileup-min-fraction", "0.0001", "-Q", "--pileup-min-mapq", "254"], ["p.tsv"]),
    (["--sv-signatures", "v.tsv"], ["v.tsv"]),
    (["--sv-signatures", "v.tsv", "--sv-min-length", "1", "--sv-max-distance", "4294967295", "--sv-min-support", "1", "--sv-secondary", "-Q", "--sv-min-mapq", "1"], ["v.tsv"]),
    (["--sv-signatures", "v.tsv", "--sv-min-length", "268435455", "--sv-max-distance", "1", "--sv-min-support", "4294967295", "-Q", "--sv-min-mapq", "254"], ["v.tsv"]),
    (["--error-profile", "e.tsv"], ["e.tsv"]), (["--error-profile", "e.tsv", "--error-profile-secondary", "-Q", "--error-profile-min-mapq", "1"], ["e.tsv"]),
    (["--error-profile", "e.tsv", "-Q", "--error-profile-min-mapq", "254"], ["e.tsv"]), (["--paf", "m.paf"], ["m.paf"]),
    (["--paf", "m.paf", "--paf-cigar", "--paf-unmapped", "--paf-skip-secondary"], ["m.paf"]),
    (["--threads=2", "--max-alignments=3", "--stats-input-hint=simulated", "--md-tag=1"], []),          # the = form; a flag ignores its value
]


def test_accepted_command_lines(tmp_path):
    ref, fq = os.path.join(GOLD, "reference.fasta"), os.path.join(GOLD, "queries.fastq")
    lines = [(["-r", ref, "-q", fq, "-o", "out.sam", "-p", "0.08", *extra], ["out.sam", *files]) for extra, files in ACCEPTED]
    lines += [(["--reference", ref, "--queries", fq, "--output", "out.bam", "--query-errors", "2"], ["out.bam"]),
              (["-r", ref, "-q", fq, "-e", "3", "--paf", "only.paf"], ["only.paf"]),                                      # a PAF output alone is an output
              (["-r", ref, "-q", fq, "-o", "out.bam", "-e", "3", "--sort-by-coordinate"], ["out.bam"]),
              (["-r", ref, "-q", fq, "-o", "out.bam", "-e", "3", "--sort-by-coordinate", "--bam-index", "--sort-tmp", "."], ["out.bam", "out.bam.bai"])]
    for argv, files in lines:
        r = run(argv, tmp_path, "1")
        assert r.returncode == 0 and r.stdout == b"" and b"CLI PARSER ERROR" not in r.stderr, (argv, r.stderr)
        assert b"[flx cli parse only]" in r.stderr, argv                                        # the reader's diagnostic still follows
        assert not any(os.path.exists(tmp_path / f) for f in files), argv


def dump(argv, cwd):
    r = run(argv, cwd, "options")
    assert r.returncode == 0 and r.stdout == b"", (argv, r.stderr)
    rows = [line.split("=", 1) for line in r.stderr.decode().splitlines()]
    assert all(len(row) == 2 for row in rows), r.stderr                                         # nothing but the dump: no log line, no reader
    assert len({k for k, _ in rows}) == len(rows)
    return dict(rows)


def help_ids():
    with open(os.path.join(GOLD, "cli_help.txt")) as f:
        return [line.split("--", 1)[1].split()[0] for line in f.read().splitlines()[1:]]


# the parent's defaults: everything that is not listed here is 0 (a flag or a count) or empty (a text)
DEFAULTS = {"seed-errors": "2", "max-anchors-hard": "500", "max-anchors-soft": "50", "anchor-group-order": "count_first", "anchor-choice-strategy": "round_robin",
            "seed-sampling-step-size": "1", "extra-verification-ratio": "0.05", "num-anchors-per-task": "3000", "threads": "1"}
TEXTS = {"reference", "queries", "output", "index", "logfile", "anchor-group-order", "anchor-choice-strategy", "stats", "stats-input-hint", "devices", "coverage",
         "coverage-summary", "coverage-windows", "pileup", "sv-signatures", "error-profile", "sort-tmp", "paf"}


def test_dump_of_the_minimal_command_line_is_the_defaults():
    given = {"reference": "reference.fasta", "queries": "queries.fastq", "output": "out.sam", "query-errors": "7"}
    got = dump([a for k, v in given.items() for a in ("--" + k, v)], GOLD)
    assert list(got) == help_ids()                                                              # one line per row, in the table's order
    for k, v in got.items():
        assert v == given.get(k, DEFAULTS.get(k, "" if k in TEXTS else "0")), k
    assert not os.path.exists(os.path.join(GOLD, "out.sam"))


# one command line with a value of its own for every value option and every flag that can stand next to the others ...
VALUES = {"reference": "reference.fasta", "queries": "queries.fastq", "output": "out.bam", "index": "some.index", "logfile": "some.log", "query-errors": "11",
          "error-probability": "0.07", "seed-errors": "3", "max-anchors-hard": "401", "max-anchors-soft": "41", "anchor-group-order": "errors_first",
          "anchor-choice-strategy": "full_groups", "seed-sampling-step-size": "5", "extra-verification-ratio": "0.125", "num-anchors-per-task": "2999", "threads": "6",
          "timeout": "77", "stats": "stats.toml", "stats-input-hint": "simulated", "devices": "0-3", "max-alignments": "1", "partial-min-span": "501", "partial-max": "8",
          "partial-extend-weight": "9", "partial-extend-xdrop": "101", "partial-extend-max-errors": "1023", "split-tails-weight": "10", "split-tails-xdrop": "102",
          "split-tails-min-rows": "103", "realign-match": "12", "realign-mismatch": "13", "realign-gap-open": "14", "realign-gap-extend": "15", "realign-band": "17",
          "coverage": "c.bedgraph", "coverage-summary": "cs.tsv", "coverage-windows": "cw.tsv", "coverage-window": "1001", "coverage-min-mapq": "18", "pileup": "p.tsv",
          "pileup-min-depth": "19", "pileup-min-count": "20", "pileup-min-fraction": "0.25", "pileup-min-mapq": "21", "sv-signatures": "v.tsv", "sv-min-length": "51",
          "sv-max-distance": "99", "sv-min-support": "22", "sv-min-mapq": "23", "error-profile": "e.tsv", "error-profile-min-mapq": "24", "sort-tmp": "spill", "paf": "m.paf"}
FLAGS = ["console-debug-logs", "dont-erase-useless-anchors", "bottom-up-pex-tree", "interval-optimization", "direct-full-verification", "drop-duplicate-alignments",
         "mapping-quality", "md-tag", "cs-tag", "partial-alignments", "partial-extend", "sa-tag", "split-tails", "left-align-indels", "realign-affine", "coverage-deletions",
         "coverage-secondary", "coverage-zero", "pileup-secondary", "sv-secondary", "error-profile-secondary", "sort-by-coordinate", "bam-index", "paf-cigar", "paf-unmapped",
         "paf-skip-secondary"]
# ... and the two flags that cannot: -w refuses everything that reads a CIGAR, --cs-tag-long refuses --cs-tag
SECOND = ["without-cigar", "cs-tag-long"]


def test_dump_echoes_every_option_under_its_own_id():
    ids = help_ids()
    assert sorted(ids) == sorted([*VALUES, *FLAGS, *SECOND])                                    # every row of the table is exercised
    assert len(set(VALUES.values())) == len(VALUES)                                             # two rows bound to one field would show
    got = dump([a for k, v in VALUES.items() for a in ("--" + k, v)] + ["--" + k for k in FLAGS], GOLD)
    assert got == {k: VALUES.get(k, "1" if k in FLAGS else "0") for k in ids}
    # (they exclude each other as well, so each goes into a command line of its own and changes its own row alone)
    minimal = ["-r", "reference.fasta", "-q", "queries.fastq", "-o", "out.sam", "-e", "7"]
    base = dump(minimal, GOLD)
    for flag in SECOND:
        got = dump(minimal + ["--" + flag], GOLD)
        assert {k for k in ids if got[k] != base[k]} == {flag} and got[flag] == "1", flag
    assert not any(os.path.exists(os.path.join(GOLD, f)) for f in ("out.sam", "out.bam", "some.log", "m.paf", "stats.toml"))
