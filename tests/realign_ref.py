"""The affine-gap realignment rule (include/floxer_amd.h, flx_realign_options) in plain Python: full matrices with a real minus
infinity, written from the rule's text. A path is a list of (op, length) with the BAM op codes = (7), X (8), I (1), D (2), a reference
window `ref`, a query `qry` and `begin`, the window column of its first column; scores = (match, mismatch, gap_open, gap_extend), band = w.
Parsing, packing and replaying of paths are leftalign_ref's."""
import random

import numpy as np

from leftalign_ref import D, EQ, I, X, pack_jobs, parse, path_of, replay, show, words_of      # noqa: F401 (shared with the tests)

INF = float("inf")
DEFAULT = (2, 4, 4, 2)
SCORE_SETS = [DEFAULT, (1, 1, 1, 1), (5, 4, 10, 1), (1, 15, 1, 1)]       # the last: c_max = 16 = 8 c_min


def c_max_min(scores):
    a, b, o, e = scores
    return max(a + b, o + e + a), min(a + b, o + e)


def shape(path):
    """rows, columns, NM and the smallest and largest diagonal j - i over the cells the path visits, (0, 0) included"""
    m = n = nm = d = d_min = d_max = 0
    for op, ln in path:
        if op in (EQ, X):
            m += ln
            n += ln
        elif op == I:
            m += ln
            d -= ln
        else:
            n += ln
            d += ln
        if op != EQ:
            nm += ln
        d_min, d_max = min(d_min, d), max(d_max, d)
    return m, n, nm, d_min, d_max


def path_score(path, scores):
    a, b, o, e = scores
    return sum(a * ln if op == EQ else -b * ln if op == X else -(o + e * ln) for op, ln in path)


def cells(path):
    """the cells (i, j) a path visits, (0, 0) first"""
    i = j = 0
    out = [(0, 0)]
    for op, ln in path:
        for _ in range(ln):
            i += op != D
            j += op != I
            out.append((i, j))
    return out


def realign(path, ref, qry, begin, scores=DEFAULT, band=16):
    """the rule: (new path, score, num_errors, lo, hi)"""
    a, b, o, e = scores
    m, n, _, d_min, d_max = shape(path)
    lo, hi = d_min - band, d_max + band
    H = [[-INF] * (n + 1) for _ in range(m + 1)]
    E = [[-INF] * (n + 1) for _ in range(m + 1)]
    F = [[-INF] * (n + 1) for _ in range(m + 1)]
    for i in range(m + 1):
        for j in range(max(0, i + lo), min(n, i + hi) + 1):
            if i == 0 and j == 0:
                H[0][0] = 0
                continue
            if j > 0:
                E[i][j] = max(H[i][j - 1] - o - e, E[i][j - 1] - e)
            if i > 0:
                F[i][j] = max(H[i - 1][j] - o - e, F[i - 1][j] - e)
            dg = H[i - 1][j - 1] + (a if qry[i - 1] == ref[begin + j - 1] else -b) if i > 0 and j > 0 else -INF
            H[i][j] = max(dg, E[i][j], F[i][j])
    i, j, state, ops = m, n, "H", []
    while i > 0 or j > 0:
        if state == "H":
            if i > 0 and H[i][j] == F[i][j]:
                state = "F"
            elif j > 0 and H[i][j] == E[i][j]:
                state = "E"
            else:
                ops.append(EQ if qry[i - 1] == ref[begin + j - 1] else X)
                i -= 1
                j -= 1
        elif state == "F":
            ops.append(I)
            above_in_band = i - 1 >= 0 and lo <= j - (i - 1) <= hi
            state = "F" if above_in_band and F[i][j] == F[i - 1][j] - e else "H"
            i -= 1
        else:
            ops.append(D)
            left_in_band = j - 1 >= 0 and lo <= (j - 1) - i <= hi
            state = "E" if left_in_band and E[i][j] == E[i][j - 1] - e else "H"
            j -= 1
    out = []
    for op in reversed(ops):
        if out and out[-1][0] == op:
            out[-1] = (op, out[-1][1] + 1)
        else:
            out.append((op, 1))
    return out, H[m][n], sum(ln for op, ln in out if op != EQ), lo, hi


def check_properties(path, ref, qry, begin, out, score, scores=DEFAULT, band=16):
    """everything the rule promises of (out, score) = realign(path)"""
    m, n, nm, d_min, d_max = shape(path)
    before = replay(path, ref, qry, begin)                       # (the input is a true path: = over equal letters, X over unequal ones)
    after = replay(out, ref, qry, begin)
    assert after[:2] == before[:2] == (n, m), (show(path), show(out))
    assert all(ln > 0 for _, ln in out) and all(p[0] != q[0] for p, q in zip(out, out[1:])), show(out)
    assert score == path_score(out, scores) >= path_score(path, scores), (show(path), show(out), score)
    lo, hi = d_min - band, d_max + band
    assert all(lo <= j - i <= hi for i, j in cells(out)), (show(path), show(out))
    c_max, c_min = c_max_min(scores)
    not_eq = sum(op != EQ for op, _ in out)
    assert not_eq <= nm * c_max // c_min and len(out) <= 2 * (nm * c_max // c_min) + 1, (show(path), show(out))


def gap_words(path):
    return sum(op in (I, D) for op, _ in path)


def random_path(rng, cols, alphabet=4, rate=0.12, max_indel=5):
    """a random path of about `cols` columns with about `rate` errors and indels of 1..max_indel, and letters that make it true"""
    path, c = [], 0
    while c < cols:
        x = rng.random()
        if x < rate / 3:
            op, ln = X, 1
        elif x < 2 * rate / 3:
            op, ln = I, rng.randint(1, max_indel)
        elif x < rate:
            op, ln = D, rng.randint(1, max_indel)
        else:
            op, ln = EQ, rng.randint(1, 6)
        if path and path[-1][0] == op:
            path[-1] = (op, path[-1][1] + ln)
        else:
            path.append((op, ln))
        c += ln if op != I else 0
    begin = rng.randint(0, 3)
    n = begin + sum(ln for op, ln in path if op != I) + rng.randint(0, 3)
    ref = [rng.randrange(alphabet) for _ in range(n)]
    qry, r = [], begin
    for op, ln in path:
        if op == EQ:
            qry += ref[r: r + ln]
        elif op == X:
            qry += [(ref[r + i] + 1 + rng.randrange(max(1, alphabet - 1))) % max(2, alphabet) for i in range(ln)]
        elif op == I:
            qry += [rng.randrange(alphabet) for _ in range(ln)]
        if op != I:
            r += ln
    return path, np.array(ref, dtype=np.uint8), np.array(qry, dtype=np.uint8), begin


def random_corpus(seed, n_paths, max_cols=300):
    rng = random.Random(seed)
    return [random_path(rng, rng.randint(1, max_cols) if i % 3 else rng.randint(1, 40), alphabet=4 if i % 2 else 2,
                        rate=rng.choice((0.05, 0.12, 0.3)), max_indel=rng.choice((1, 3, 5))) for i in range(n_paths)]


def spell(path, ref_of, begin=0, tail=0, ins=None):
    """letters that make the path true over a reference given by column, ref_of(col), of ranks 1..4: = copies the column, X takes the
    next rank, I takes ins(row) (default: a rank that differs from the columns on both sides)"""
    cols = begin + sum(ln for op, ln in path if op != I) + tail
    ref = [ref_of(c) for c in range(cols)]
    qry, r = [], begin
    for op, ln in path:
        if op == EQ:
            qry += ref[r: r + ln]
        elif op == X:
            qry += [x % 4 + 1 for x in ref[r: r + ln]]
        elif op == I:
            around = {ref[min(cols - 1, r)], ref[max(0, r - 1)]} if cols else set()
            qry += [ins(len(qry) + i) if ins else min(x for x in (1, 2, 3, 4) if x not in around) for i in range(ln)]
        if op != I:
            r += ln
    return path, np.array(ref, dtype=np.uint8), np.array(qry, dtype=np.uint8), begin


def noise(seed):
    """a reference without structure: column -> rank 1..4"""
    letters = np.random.default_rng(seed).integers(1, 5, size=4096)
    return lambda c: int(letters[c % 4096])
