"""Named texts built against the structure of the kernels that make the index on the device (flx_index_build.hip: sa_init, sa_flag,
sa_rank, sa_key, bwt, reverse, occ_planes, occ_counts around rocprim's sort and scans) and of the two that derive a context's tables
from it (isa_kernel and filter_build_kernel of flx_search.hip). TEST INFRASTRUCTURE ONLY.

A case is (name, cls, refs, props): the sequences the index is built from (ranks: 1..4 = A C G T, 5 = N; the index pads each with
4 - len % 4 delimiters of rank 0) and what the construction promises about the text, checked on the references of index_ref.py by
test_index_corpus_host.py, never on the product. No text has more than about 20 000 symbols, so that sorted() over its suffixes stays
cheap; the largest is filter_block (LARGE), which the GPU tests run once per K.

Classes:
  tiny     single sequences of 1, 3, 4, 5 and 7 symbols (n = 4, 4, 8, 8, 8) and two sequences of one symbol: every position's initial key of
           ten symbols reads past the end of the text
  block    texts of n = 28, 32, 36, 60, 64, 68, 252, 256, 260, 4092, 4096, 4100 symbols: n % 32 in {28, 0, 4}, the number of occurrence
           blocks nb = n // 32 + 1 of both parities (an even nb: the second half of the last wave of occ_planes_kernel is live), a last
           block of nothing but padding when n % 32 = 0, and the 256 threads of a block, the scans' and the sort's tiles on either side.
           props: n_mod_32, nb_mod_2, last_block_empty
  depth    repeats whose suffixes first differ on either side of a doubling step (ranks of h = 10, 20, 40, ..., 5120 symbols). props:
           distinct = (lo, hi): the number of symbols that tells every two suffixes apart (the longest common prefix of two neighbours of
           the suffix array, plus one) lies in lo < d <= hi, two neighbouring values of h. Homopolymers of 9, 10, 11, 19, 20, 21, 39, 40,
           41, 5119, 5120, 5121 symbols; two and three identical sequences of 3000 (their order is decided behind the delimiters); a sequence
           of 3000 and its prefix of 2999; tandem arrays of period 2, 3 and 7 over 3000 symbols, the period-3 one also with an N in one unit.
           depth_end_tie: "ACGT", "ACGT", "ACT...": in the reversed text the suffix of exactly ten symbols is the prefix of a suffix
           whose next ten symbols are the smallest suffix of all, and twenty symbols on both are past the end. A past-the-end rank that
           is not below every real rank leaves the two tied for good, and the shorter one is then not first.
  symbols  a sequence of nothing but N; N runs at a sequence's first and last positions; fifty sequences of one symbol each (the text is
           mostly delimiters, in runs of three); sequences whose lengths are multiples of 4 (four delimiters each)
  filter   texts for filter_build_kernel, run with FLX_FILTER_K = 8, 9 and 12 (FILTER_KS), each also with the mirrored table. What a
           text plants depends on K and tmin, so props["features"] is a function (K, tmin) -> [(label, first bit, number of bits)] of
           what must be set, and props["clear"] one (K) -> [bit] of K-mers that the text does not hold by construction.
           filter_runs_<K>_<j>: A/C/G/T runs of tmin - 1, tmin, K - 4, K - 3, K - 1, K and K + 1 symbols (five lengths: these texts are
               short, so tmin = K - 3), each between two delimiters and between two Ns; the j-th of the lengths also at the text's start
               and at its end. Built for that K and the tmin that follows from the text's own length
           filter_span: K-mers over G/T in a filler of A/C whose last symbols lie at positions 62, 63, 64, 65 mod 64 (the 64 window ends
               of one thread; the warm-up of K - 1 symbols reaches into the span before), in the spans 0, 1, 2 and 63
           filter_block: the same at positions 16383, 16384, 16385, where the second block of 256 threads begins (LARGE: 17 000 symbols)
           filter_ends: the all-A and the all-T K-mer (bit 0 of word 0, the last bit of the last word)
           filter_ext_<K>: runs of K - 1, K - 2 and K - 3 symbols behind a delimiter: left-extension ranges of 4, 16 and 64 bits, the last
               a whole word
           filter_homopolymer: 4096 x G: some thousand window ends, 64 threads, one bit
"""
import collections
import functools
import zlib

import numpy as np

import index_ref as R

Case = collections.namedtuple("Case", "name cls refs props")

BLOCK_NS = (28, 32, 36, 60, 64, 68, 252, 256, 260, 4092, 4096, 4100)
HOMOPOLYMERS = (9, 10, 11, 19, 20, 21, 39, 40, 41, 5119, 5120, 5121)
STEPS = (0, 10, 20, 40, 80, 160, 320, 640, 1280, 2560, 5120, 10240, 20480)          # the depths the doubling ranks at
TINY_LENGTHS = (1, 3, 4, 5, 7)
FILTER_KS = (8, 9, 12)
SPAN_RESIDUES = (62, 63, 64, 65)
SPAN_SPANS = (0, 1, 2, 63)                                                           # thread spans at whose ends filter_span plants (63: the last lane of a wave)
BLOCK_ENDS = (16383, 16384, 16385)
LARGE = ("filter_block",)
RUN_LENGTHS = 5                                                                      # run_lengths(k, k - 3) has five entries
A, C_, G, T, N = 1, 2, 3, 4, 5


def _rng(name):
    return np.random.default_rng(zlib.crc32(("index_" + name).encode()))


def _arr(x):
    return np.asarray(x, dtype=np.uint8)


def _step_interval(d):
    """the two neighbouring doubling depths with lo < d <= hi"""
    for lo, hi in zip(STEPS, STEPS[1:]):
        if lo < d <= hi:
            return lo, hi
    raise ValueError(d)


# ------------------------------------------------------------------------------------------------ tiny, block, symbols
def _tiny():
    rng = _rng("tiny")
    out = [Case(f"tiny_{n}", "tiny", [rng.integers(1, 5, size=n).astype(np.uint8)], dict(n=n + 4 - n % 4)) for n in TINY_LENGTHS]
    out.append(Case("tiny_1_1", "tiny", [_arr([G]), _arr([A])], dict(n=8)))
    return out


def _block():
    out = []
    for n in BLOCK_NS:
        rng = _rng(f"block_{n}")
        if n < 60:
            lens = [n - 3]                                           # n - 3 = 1 mod 4: three delimiters
        else:
            first = n // 8 * 4 + 2                                   # two delimiters behind it: n // 8 * 4 + 4 symbols of the text
            lens = [first, n - (first + 2) - 1]                      # the rest, less one delimiter
        refs = [rng.integers(1, 5, size=ln).astype(np.uint8) for ln in lens]
        out.append(Case(f"block_{n}", "block", refs, dict(n=n, n_mod_32=n % 32, nb_mod_2=(n // 32 + 1) % 2, last_block_empty=n % 32 == 0)))
    return out


def _symbols():
    rng = _rng("symbols")
    rand = lambda n: rng.integers(1, 5, size=n).astype(np.uint8)
    return [
        Case("symbols_only_n", "symbols", [np.full(37, N, np.uint8)], {}),
        Case("symbols_n_at_ends", "symbols", [np.concatenate([np.full(5, N, np.uint8), rand(90), np.full(3, N, np.uint8)]),
                                              np.concatenate([_arr([N]), rand(41), _arr([N])])], {}),
        Case("symbols_fifty_singles", "symbols", [_arr([int(c)]) for c in rng.integers(1, 6, size=50)], dict(delimiter_runs=3)),
        Case("symbols_multiples_of_4", "symbols", [rand(n) for n in (4, 8, 64, 128, 12)], dict(delimiter_runs=4)),
    ]


# ------------------------------------------------------------------------------------------------ depth
def _depth():
    out = []
    for n in HOMOPOLYMERS:
        out.append(Case(f"depth_homopolymer_{n}", "depth", [np.full(n, C_, np.uint8)], dict(distinct=_step_interval(n))))
    rng = _rng("depth")
    s = rng.integers(1, 5, size=3000).astype(np.uint8)
    # two copies: S 0000 S 0000 against S 0000 <end>: 3004 symbols in common; three: 6008
    out.append(Case("depth_two_identical", "depth", [s.copy(), s.copy()], dict(distinct=_step_interval(3005))))
    out.append(Case("depth_three_identical", "depth", [s.copy(), s.copy(), s.copy()], dict(distinct=_step_interval(6009))))
    out.append(Case("depth_prefix_2999", "depth", [s.copy(), s[:2999].copy()], dict(distinct=_step_interval(3000))))
    for p in (2, 3, 7):
        unit = {2: [A, G], 3: [A, C_, T], 7: [A, A, C_, G, T, T, G]}[p]
        arr = np.tile(_arr(unit), 3000 // p + 1)[:3000]
        out.append(Case(f"depth_tandem_{p}", "depth", [arr], dict(distinct=_step_interval(3000 - p + 1))))       # suffixes i and i + p
    arr = np.tile(_arr([A, C_, T]), 1000)
    arr[1501] = N                                                    # suffixes 0 and 3 agree up to the N: 1498 symbols
    out.append(Case("depth_tandem_3_n", "depth", [arr], dict(distinct=_step_interval(1499))))
    # reversed text: ... x C A | 0000 T G C A | 0000 T G C A: the last ten symbols (C A 0000 T G C A) also stand eighteen from the end
    out.append(Case("depth_end_tie", "depth", [_arr([A, C_, G, T]), _arr([A, C_, G, T]), _arr([A, C_, T, T, G, A, C_]), _arr([G, G, A, T, C_])],
                    dict(distinct=_step_interval(11), end_tie=True)))
    return out


# ------------------------------------------------------------------------------------------------ filter
def _starts(refs):
    """where each sequence begins in the padded text"""
    return np.cumsum([0] + [len(r) + 4 - len(r) % 4 for r in refs])


def _gt(rng, n, k=min(FILTER_KS)):
    """n symbols over G/T whose windows of k symbols are all different (so are the longer ones): grown symbol by symbol, begun again when
    neither symbol gives a new window"""
    while True:
        s, seen = [int(c) for c in rng.integers(3, 5, size=k - 1)], set()
        while len(s) < n:
            options = [c for c in rng.permutation([G, T]) if tuple(s[len(s) - k + 1:] + [int(c)]) not in seen]
            if not options:
                break
            s.append(int(options[0]))
            seen.add(tuple(s[-k:]))
        if len(s) == n:
            return _arr(s)


def _planted(name, groups, length):
    """a filler over A/C of `length` symbols; for every group of neighbouring positions a piece over G/T that holds the windows of up
    to max(FILTER_KS) symbols ending at them. All pieces are cut from one G/T string without a repeated window, so each window ending
    at one of the positions stands nowhere else in the text."""
    rng = _rng(name)
    kmax = max(FILTER_KS)
    text = rng.integers(1, 3, size=length).astype(np.uint8)
    spans = [(min(g) - kmax + 1, max(g) + 1) for g in groups]
    pool = _gt(rng, sum(hi - lo for lo, hi in spans))
    at = 0
    for lo, hi in spans:
        text[lo:hi] = pool[at:at + hi - lo]
        at += hi - lo
    ends = [q for g in groups for q in g]
    padded = R.padded_text([text])
    return Case(name, "filter", [text], dict(
        ends=ends, features=lambda k, tmin: [(f"window ending at {q}", R.code_of(padded[q - k + 1:q + 1]), 1) for q in ends],
        # the filler holds neither G nor T and no piece an A or a C: no A or C stands between two of G/T
        clear=lambda k: [R.code_of(([G, A, T] * k)[:k]), R.code_of(([T, C_] * k)[:k]), R.code_of([A] * (k - 3) + [G, C_, G])]))


def run_lengths(k, tmin):
    return sorted({ln for ln in (tmin - 1, tmin, k - 4, k - 3, k - 1, k, k + 1) if ln >= 1})


def _runs_case(k, j):
    """the j-th run length of run_lengths(k, tmin) at the text's start and at its end, every length between delimiters and between Ns.
    tmin follows from the text's length: the text is built for the tmin it turns out to have (the host test checks that it has)."""
    name = f"filter_runs_{k}_{j}"
    for tmin in range(max(1, k - 3), k + 1):
        rng = _rng(name)
        letters = lambda ln: rng.integers(1, 5, size=ln).astype(np.uint8)
        lengths = run_lengths(k, tmin)
        own = lengths[j]
        refs = [np.concatenate([letters(own), _arr([N]), letters(2)])]
        runs = [(0, 0, own, "start")]                                # (sequence, offset in it, length, what bounds it)
        for ln in lengths:
            refs.append(letters(ln))
            runs.append((len(refs) - 1, 0, ln, "delimiter"))
            refs.append(np.concatenate([letters(3), _arr([N]), letters(ln), _arr([N]), letters(1)]))
            runs.append((len(refs) - 1, 4, ln, "n"))
        refs.append(np.concatenate([letters(2), _arr([N]), letters(own)]))
        runs.append((len(refs) - 1, 3, own, "end"))
        text = R.padded_text(refs)
        if R.filter_tmin_for(len(text), k) == tmin:
            break
    else:
        raise AssertionError("no text whose tmin is the one it was built for")
    starts = _starts(refs)

    def features(kk, tm):
        out = []
        for s, o, ln, bound in runs:
            for grown in range(1, ln + 1):                           # the run as it grows, window end by window end
                q, r = int(starts[s]) + o + grown - 1, min(grown, kk)
                if r == kk:
                    out.append((f"run of {ln} ({bound}), window ending at {q}", R.code_of(text[q - kk + 1:q + 1]), 1))
                elif tm <= r and kk - r <= 3:
                    out.append((f"run of {ln} ({bound}), {r} symbols ending at {q}", R.code_of(text[q - r + 1:q + 1]) << (2 * (kk - r)), 4 ** (kk - r)))
        return out
    return Case(name, "filter", refs, dict(features=features, k=k, tmin=tmin, lengths=lengths, runs=[(int(starts[s]) + o, ln, b) for s, o, ln, b in runs]))


def _ext_case(k):
    """runs of k - 1, k - 2 and k - 3 symbols between delimiters (the first at the text's start)"""
    rng = _rng(f"filter_ext_{k}")
    refs = [rng.integers(1, 5, size=k - u).astype(np.uint8) for u in (1, 2, 3)] + [rng.integers(1, 5, size=40).astype(np.uint8)]

    def features(kk, tm):
        if kk != k:
            return []
        return [(f"{4 ** u} left extensions of the run of {k - u}", R.code_of(refs[i]) << (2 * u), 4 ** u) for i, u in enumerate((1, 2, 3)) if tm <= k - u]
    return Case(f"filter_ext_{k}", "filter", refs, dict(features=features, k=k))


def _filter():
    out = [_runs_case(k, j) for k in FILTER_KS for j in range(RUN_LENGTHS)]
    out.append(_planted("filter_span", [[64 * s + r for r in SPAN_RESIDUES] for s in SPAN_SPANS], 64 * (max(SPAN_SPANS) + 2) + 11))
    out.append(_planted("filter_block", [list(BLOCK_ENDS)], 17003))
    rng = _rng("filter_ends")
    kmax = max(FILTER_KS)
    mid = rng.integers(2, 4, size=30).astype(np.uint8)               # C/G between them: an A stands beside an A or a C only, a T beside a T or a G
    out.append(Case("filter_ends", "filter", [np.concatenate([np.full(kmax + 1, A, np.uint8), _arr([C_]), mid, _arr([G]), np.full(kmax + 1, T, np.uint8)])], dict(
        features=lambda k, tmin: [("all A", 0, 1), ("all T", 4 ** k - 1, 1)],
        clear=lambda k: [R.code_of(([A, T] * k)[:k]), R.code_of(([T, A] * k)[:k]), R.code_of([T] * (k - 1) + [A]), R.code_of([A] * (k - 1) + [T])])))
    out += [_ext_case(k) for k in FILTER_KS]
    out.append(Case("filter_homopolymer", "filter", [np.full(4096, G, np.uint8)], dict(
        features=lambda k, tmin: [("all G", R.code_of([G] * k), 1)],
        clear=lambda k: [0, 4 ** k - 1, R.code_of([G] * (k - 1) + [A]), R.code_of([G] * (k - 2) + [A, G])])))
    return out

@functools.lru_cache(maxsize=None)
def cases():
    out = _tiny() + _block() + _depth() + _symbols() + _filter()
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


# every case by name (known without building the corpus: tests are parametrised over them); a case's class is its name's first word
NAMES = tuple([f"tiny_{n}" for n in TINY_LENGTHS] + ["tiny_1_1"] + [f"block_{n}" for n in BLOCK_NS] + [f"depth_homopolymer_{n}" for n in HOMOPOLYMERS] +
              ["depth_two_identical", "depth_three_identical", "depth_prefix_2999", "depth_tandem_2", "depth_tandem_3", "depth_tandem_7",
               "depth_tandem_3_n", "depth_end_tie", "symbols_only_n", "symbols_n_at_ends", "symbols_fifty_singles", "symbols_multiples_of_4"] +
              [f"filter_runs_{k}_{j}" for k in FILTER_KS for j in range(RUN_LENGTHS)] + ["filter_span", "filter_block", "filter_ends"] + [f"filter_ext_{k}" for k in FILTER_KS] +
              ["filter_homopolymer"])
# the texts whose filter tables are compared: the whole filter class and one text of each other class
FILTER_NAMES = tuple(n for n in NAMES if n.startswith("filter_")) + ("tiny_5", "block_4096", "depth_tandem_3_n", "symbols_n_at_ends")


def case(name):
    return {c.name: c for c in cases()}[name]


@functools.lru_cache(maxsize=None)
def reference(name):
    """everything index_ref makes of a case's text, computed once and shared (read-only arrays)"""
    c = case(name)
    text = R.padded_text(c.refs)
    sa = R.suffix_array(text)
    rev = text[::-1].copy()
    sa_rev = R.suffix_array(rev)
    bwt0, bwt1 = R.bwt(text, sa), R.bwt(rev, sa_rev)
    ref = dict(text=text, sa=sa, sa_rev=sa_rev, bwt0=bwt0, bwt1=bwt1, occ0=R.occ_blocks(bwt0), occ1=R.occ_blocks(bwt1), isa=R.inverse(sa))
    for v in ref.values():
        v.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def filter_reference(name, k):
    """(filter, mirrored filter, tmin) of a case's text at FLX_FILTER_K = k"""
    text = reference(name)["text"]
    tmin = R.filter_tmin_for(len(text), k)
    f, m = R.filter_tables(text, k, tmin)
    f.setflags(write=False); m.setflags(write=False)
    return f, m, tmin


def max_lcp(text, sa):
    """the longest common prefix of two neighbours of the suffix array"""
    tb = text.tobytes()
    best = 0
    for a, b in zip(sa[:-1], sa[1:]):
        x, y = tb[int(a):], tb[int(b):]
        if x[:best + 1] != y[:best + 1]:
            continue
        lo, hi = best + 1, min(len(x), len(y))                       # the first `lo` symbols agree
        while lo < hi:
            mid = (lo + hi + 1) // 2
            if x[:mid] == y[:mid]:
                lo = mid
            else:
                hi = mid - 1
        best = lo
    return best
