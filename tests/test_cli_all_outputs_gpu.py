"""The CLI's side outputs next to each other: coverage, pileup, sv signatures, error profile and PAF, each asked for alone and all five
at once, on one device context and on two. The members of the CLI's list of side outputs are independent and every batch's run reaches
the object of the context that aligned it, so every file of the combined run is the file of its solo run, the SAM is the same in all
runs, and two contexts write what one writes."""
import os
import subprocess

import pytest

from floxer_amd import simulate as S

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOLO = {"coverage": {"--coverage": "cov.bedgraph", "--coverage-summary": "cov_summary.tsv"}, "pileup": {"--pileup": "pileup.tsv"}, "sv": {"--sv-signatures": "sv.tsv"},
        "errprof": {"--error-profile": "errprof.tsv"}, "paf": {"--paf": "out.paf"}}
# 40 reads cover a position once at most and hold no long indel: with the thresholds at 1 every differing position is a pileup site and
# every indel an sv cluster, so that neither file is empty
THRESHOLDS = {"--pileup": ["--pileup-min-depth", "1", "--pileup-min-count", "1"], "--sv-signatures": ["--sv-min-length", "1", "--sv-min-support", "1"]}


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = tmp_path_factory.mktemp("all_outputs")
    genome = S.make_genome(100000, 1, seed=3)
    reads, names, _ = S.make_reads(genome, 40, 1000, 0.05, seed=4)
    S.write_fasta(d / "ref.fasta", genome)
    S.write_fastq(d / "reads.fastq", reads, names)
    return d


def run_cli(data, where, devices, outputs):
    """One run of the CLI into the folder `where`; returns {file name: bytes} of the SAM and of every output asked for."""
    where.mkdir()
    files = {"out.sam": None, **{name: None for name in outputs.values()}}
    argv = [os.path.join(ROOT, "floxer_amd", "floxer"), "-r", str(data / "ref.fasta"), "-q", str(data / "reads.fastq"), "-i", str(data / "ref.index"), "-p", "0.05",
            "-o", str(where / "out.sam"), "-D", "-N", "1", "-Q", "--devices", devices]
    for flag, name in outputs.items():
        argv += [flag, str(where / name), *THRESHOLDS.get(flag, [])]
    env = dict(os.environ, FLX_BATCH_READS="16")                           # three batches: a second context gets work
    r = subprocess.run(argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)
    assert r.returncode == 0 and r.stdout == b"", r.stderr.decode()
    for name in files:
        files[name] = (where / name).read_bytes()
        assert files[name], name
    return files


@pytest.fixture(scope="module")
def runs(data):
    """{devices: {run: {file name: bytes}}}: the twelve runs, one after the other (one process with the GPU open at a time)."""
    got = {}
    for devices in ("0", "0,0"):
        base = data / ("two" if "," in devices else "one")
        base.mkdir()
        got[devices] = {k: run_cli(data, base / k, devices, flags) for k, flags in SOLO.items()}
        got[devices]["all"] = run_cli(data, base / "all", devices, {f: n for flags in SOLO.values() for f, n in flags.items()})
    return got


@gpu
@pytest.mark.parametrize("devices", ["0", "0,0"])
def test_combined_run_writes_the_solo_runs_files(runs, devices):
    r = runs[devices]
    assert sorted(r["all"]) == sorted({"out.sam"} | {n for flags in SOLO.values() for n in flags.values()})
    for k in SOLO:
        for name, text in r[k].items():
            assert text == r["all"][name], (k, name)                       # its own file(s), and the SAM
    mapped = [l for l in r["all"]["out.sam"].decode().splitlines() if not l.startswith("@") and not int(l.split("\t")[1]) & 4]
    assert len(mapped) >= 30 and len(r["all"]["out.paf"].decode().splitlines()) == len(mapped) and r["all"]["errprof.tsv"].startswith(b"PAIR_EQ\t")


@gpu
def test_two_contexts_write_what_one_writes(runs):
    assert runs["0"]["all"] == runs["0,0"]["all"]
