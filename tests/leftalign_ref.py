"""The left-align rule of floxer_amd/csrc/flx_leftalign.hpp in plain Python, a checker that replays a path over its letters, and the
paths the tests share. A path is a list of (op, length) with the BAM op codes = (7), X (8), I (1), D (2), a reference window `ref`, a
query `qry` (anything indexable whose items compare: bytes, lists, arrays of ranks) and `begin`, the window column of its first column."""
import random

import numpy as np

EQ, X, I, D = 7, 8, 1, 2
OPS = "MIDNSHP=X"


def words_of(path):
    return np.array([(ln << 4) | op for op, ln in path], dtype=np.uint32)


def path_of(words):
    return [(int(w) & 15, int(w) >> 4) for w in words]


def parse(cigar):
    """'5=2D1X' -> [(7, 5), (2, 2), (8, 1)]"""
    out, num = [], ""
    for ch in cigar.replace(" ", ""):
        if ch.isdigit():
            num += ch
        else:
            out.append((OPS.index(ch), int(num)))
            num = ""
    return out


def show(path):
    return "".join(f"{ln}{OPS[op]}" for op, ln in path)


def left_align(path, ref, qry, begin, gaps=None):
    """the rule: the words left to right into an output list. gaps (a list): receives (columns shifted, merged with a gap word in front)
    for every gap word of the path, in order"""
    out = []
    r, q = begin, 0
    for op, ln in path:
        if op in (EQ, X):
            if out and out[-1][0] == op:
                out[-1] = (op, out[-1][1] + ln)
            else:
                out.append((op, ln))
            r += ln
            q += ln
            continue
        seq = ref if op == D else qry
        c = r if op == D else q
        L, shift, merged = ln, 0, False
        while out:
            p_op, p_len = out[-1]
            if p_op == op:
                out.pop()
                L += p_len
                c -= p_len
                merged = True
                continue
            if p_op != EQ:
                break
            e_max = p_len - 1 if len(out) == 1 else p_len
            s = 0
            while s < e_max and seq[c - s - 1] == seq[c - s - 1 + L]:
                s += 1
            if s == 0:
                break
            if s == p_len:
                out.pop()
            else:
                out[-1] = (EQ, p_len - s)
            c -= s
            shift += s
            if s < p_len:
                break
        out.append((op, L))
        if shift:
            out.append((EQ, shift))
        if gaps is not None:
            gaps.append((shift, merged))
        if op == D:
            r += ln
        else:
            q += ln
    return out


def replay(path, ref, qry, begin):
    """asserts that = columns pair equal letters and X columns unequal ones; returns (columns, rows, NM) consumed"""
    r, q, nm = begin, 0, 0
    for op, ln in path:
        assert ln > 0, (show(path), "zero-length word")
        if op == EQ:
            for i in range(ln):
                assert ref[r + i] == qry[q + i], (show(path), r + i, q + i, "= over unequal letters")
        elif op == X:
            for i in range(ln):
                assert ref[r + i] != qry[q + i], (show(path), r + i, q + i, "X over equal letters")
        else:
            assert op in (I, D), op
        if op != D:
            q += ln
        if op != I:
            r += ln
        if op != EQ:
            nm += ln
    assert r <= len(ref) and q <= len(qry), (show(path), "path leaves its sequences")
    return r - begin, q, nm


def normal_form(path):
    """no two neighbouring words of one op, no zero length"""
    return all(ln > 0 for _, ln in path) and all(a[0] != b[0] for a, b in zip(path, path[1:]))


def can_step(path, ref, qry, begin):
    """True when some gap of the path could move one more column left under the rule: the word in front of it is an = that is not the
    path's first column, and the letter that would leave the = run equals the one that would enter it"""
    r, q = begin, 0
    for t, (op, ln) in enumerate(path):
        if op in (I, D) and t > 0 and path[t - 1][0] == EQ:
            e = path[t - 1][1] - (1 if t == 1 else 0)
            seq, c = (ref, r) if op == D else (qry, q)
            if e > 0 and seq[c - 1] == seq[c - 1 + ln]:
                return True
        if op != D:
            q += ln
        if op != I:
            r += ln
    return False


def check_properties(path, ref, qry, begin, out):
    """everything the rule promises of out = left_align(path)"""
    before = replay(path, ref, qry, begin)
    assert replay(out, ref, qry, begin) == before, (show(path), show(out))
    assert normal_form(out), show(out)
    assert len(out) <= 2 * before[2] + 1 and len(out) <= len(path) + sum(op in (I, D) for op, _ in path), (show(path), show(out))
    assert (path[0][0] == EQ) == (out[0][0] == EQ) if path else not out
    assert left_align(out, ref, qry, begin) == out, (show(path), show(out), "not idempotent")
    assert not can_step(out, ref, qry, begin), (show(path), show(out), "a gap can move further")


def random_path(rng, n_words, alphabet=2, max_len=6, unit=None, repeats=False):
    """A random, non-optimal path over low-complexity sequences: the words first, then letters that make them true. The reference is random
    over a small alphabet (or a tandem repeat of `unit` with a few substitutions), the query is read off the reference through the path:
    = copies, X takes another letter, I takes letters that continue the repeat (so that insertions can shift too). Words alternate in op
    unless `repeats`: then a word may repeat the op of the word in front (input that is not in normal form)."""
    ops, path = [EQ, X, I, D], []
    last = None
    for _ in range(n_words):
        op = rng.choice([o for o in ops if o != last] + [EQ, EQ])
        if op == last and not (repeats and rng.random() < 0.5):
            continue
        path.append((op, rng.randint(1, max_len)))
        last = op
    cols = sum(ln for op, ln in path if op != I)
    begin = rng.randint(0, 3)
    n = begin + cols + rng.randint(0, 3)
    if unit:
        ref = [unit[i % len(unit)] for i in range(n)]
        for _ in range(n // 40):
            ref[rng.randrange(n)] = rng.randrange(alphabet)
    else:
        ref = [rng.randrange(alphabet) for _ in range(n)]
    qry, r = [], begin
    for op, ln in path:
        if op == EQ:
            qry += ref[r: r + ln]
        elif op == X:
            qry += [(ref[r + i] + 1 + rng.randrange(max(1, alphabet - 1))) % max(2, alphabet) for i in range(ln)]
        elif op == I:
            qry += [ref[min(n - 1, r + i)] if n and rng.random() < 0.8 else rng.randrange(alphabet) for i in range(ln)]
        if op != I:
            r += ln
    return path, np.array(ref, dtype=np.uint8), np.array(qry, dtype=np.uint8), begin


def random_corpus(seed, n_paths, repeats=False):
    rng = random.Random(seed)
    out = []
    for i in range(n_paths):
        kind = i % 4
        if kind == 0:
            out.append(random_path(rng, rng.randint(1, 12), alphabet=1 + rng.randint(0, 1), max_len=4, repeats=repeats))
        elif kind == 1:
            out.append(random_path(rng, rng.randint(1, 20), alphabet=2, max_len=6, repeats=repeats))
        elif kind == 2:
            out.append(random_path(rng, rng.randint(1, 24), alphabet=4, max_len=5, unit=[rng.randrange(4) for _ in range(rng.randint(1, 3))], repeats=repeats))
        else:
            out.append(random_path(rng, rng.randint(1, 16), alphabet=3, max_len=3, repeats=repeats))
    return out


def pack_jobs(cases):
    """cases [(path, ref, qry, begin)] as the pools and jobs of flx_left_align / flx_left_align_batch"""
    words, refs, qrys, jobs = [], [], [], []
    n_w = n_r = n_q = 0
    for path, ref, qry, begin in cases:
        w = words_of(path)
        jobs.append((n_w, len(w), n_r, len(ref), begin, n_q, len(qry)))
        words.append(w)
        refs.append(np.asarray(ref, dtype=np.uint8))
        qrys.append(np.asarray(qry, dtype=np.uint8))
        n_w += len(w)
        n_r += len(ref)
        n_q += len(qry)
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    return cat(refs, np.uint8), cat(qrys, np.uint8), cat(words, np.uint32), jobs
