"""Hand-made inputs that the host test and the GPU test of the error profile share: reads of the lengths at which the position bins are
skipped, shared or uneven, and one gap per record at every case of the homopolymer bins, each with the bin worked out by hand."""
import numpy as np

import errprof_ref as R

POSITION_LENGTHS = [1, 2, 99, 100, 101, 10_007]


def _record(text, start, flag, pos, ops):
    """ops: [(op, length, letters or None)] -> (words, the read as given); = rows copy the reference, X rows differ from it, I and S rows are
    the letters given (or C G C G ..)"""
    words, seq, p = [], [], start + pos
    for op, n, letters in ops:
        words.append(R.word(op, n))
        if op == "=":
            seq += [int(x) for x in text[p: p + n]]
        elif op == "X":
            seq += [1 + int(x) % 4 for x in text[p: p + n]]             # (another letter; N and the sentinel become A)
        elif op in "IS":
            seq += list(letters) if letters is not None else [2 + k % 2 for k in range(n)]
        if op in "=XD":
            p += n
    return words, R.oriented(np.array(seq, dtype=np.uint8), flag)         # (the oriented sequence was written: the read as given is its reverse complement)


def _assemble(text, lengths, cases):
    starts = R.starts_of(lengths)
    rows, reads = [], []
    for flag, ref, pos, ops in cases:
        words, read = _record(text, int(starts[ref]), flag, pos, ops)
        rows.append((flag, ref, pos, 0, words))
        reads.append(read)
    rec, words = R.records_of(rows)
    return rec, words, reads


def position_case(n):
    """reads of n letters, forward and reverse: all rows of one op, and the rows cut into words of every op with a D in front of row 0, between
    rows and behind the last row"""
    rng = np.random.default_rng(n)
    lengths = [n + 40, 50]
    text = R.random_text(rng, lengths)
    cases = []
    for flag in (0, 16):
        cases += [(flag, 0, 3, [("=", n, None)]), (flag, 0, 5, [("X", n, None)]), (flag, 0, 7, [("D", 2, None), ("I", n, None)]), (flag, 1, 9, [("S", n, None), ("D", 3, None)])]
        if n >= 9:
            for _ in range(3):
                cuts = np.sort(rng.choice(np.arange(1, n), size=8, replace=False))
                parts = np.diff(np.concatenate([[0], cuts, [n]]))
                ops = "S=XI=X=IS"
                body = [(op, int(k), None) for op, k in zip(ops, parts)]
                body = body[:1] + [("D", 2, None)] + body[1:5] + [("D", 1, None)] + body[5:8] + [("D", 3, None)] + body[8:]     # D at row parts[0], in the middle, and with S alone behind it
                cases.append((flag, 0, 1, body))
            cases.append((flag, 0, 0, [("D", 1, None), ("=", n, None), ("D", 2, None)]))              # D at row 0 and at row n: min(r, len - 1)
    rec, words, reads = _assemble(text, lengths, cases)
    return text, lengths, rec, words, reads


def check_position_case(n, table):
    """what is known in closed form: every whole-read record spreads its n rows as g * 100 // n does, whichever strand"""
    hist = np.bincount(np.arange(n) * 100 // n, minlength=100).astype(np.uint64)
    extra = {k: table[k] - 2 * hist for k in ("POS_MATCH", "POS_MISMATCH", "POS_INS", "POS_CLIP")}
    assert all((table[k] >= 2 * hist).all() for k in extra)
    if n < 9:
        assert all(int(v.sum()) == 0 for v in extra.values())
    if n == 1:
        assert np.nonzero(hist)[0].tolist() == [0] and int(table["POS_DEL"][0]) == 4 and int(table["POS_DEL"].sum()) == 4
    if n == 2:
        assert np.nonzero(hist)[0].tolist() == [0, 50]
        assert int(table["POS_DEL"][0]) == 2 and int(table["POS_DEL"][50]) == 2      # D in front of the I: forward row 0 is g 0, reverse row 0 is g 1; S first: r = 2 -> row 1
    if n == 99:
        assert hist[99] == 0 and hist[98] == 1 and hist[0] == 1
    if n == 100:
        assert (hist == 1).all()
    if n == 101:
        assert hist[0] == 2 and (hist[1:] == 1).all()
    if n == 10_007:
        assert set(hist.tolist()) == {100, 101} and int(table["POS_DEL"][0]) >= 1 and int(table["POS_DEL"][99]) >= 1


def homopolymer_case():
    """-> text, lengths, records, words, reads, [(section, bin)] per record"""
    seq0, at = [], {}

    def put(name, letters):
        at[name] = len(seq0)
        seq0.extend(letters)

    def fill():
        seq0.extend([2, 3] * 5)                                           # C G C G ..: ends with G, begins with C
    for name, letters in (("A31", [1] * 31), ("A32", [1] * 32), ("A33", [1] * 33), ("A40", [1] * 40), ("T50", [4] * 50), ("N3", [5] * 3), ("A2", [1] * 2)):
        fill()
        put(name, letters)
    fill()
    put("end", [1] * 3)                                                   # sequence 0 ends with A A A ..
    seq1 = [1] * 5 + [2, 3] * 10                                          # .. and sequence 1 goes on with A A A A A
    lengths = [len(seq0), len(seq1)]
    text = np.array(seq0 + seq1, dtype=np.uint8)
    n0 = len(seq0)
    E, A2, N2, AC, T2 = ("=", 5, None), [1, 1], [5, 5], [1, 2], [4, 4]
    cases = [
        # deletions: (flag, ref, pos, ops), (section, bin)
        ((0, 0, at["A31"] + 10, [E, ("D", 1, None), E]), ("HP_DEL", 31)),
        ((16, 0, at["A32"] + 10, [E, ("D", 1, None), E]), ("HP_DEL", 32)),
        ((0, 0, at["A33"] + 10, [E, ("D", 1, None), E]), ("HP_DEL", 32)),                  # 33
        ((16, 0, at["A40"] - 5, [E, ("D", 1, None), E]), ("HP_DEL", 32)),                  # 0 + 1 + 32 of the 39 on the right
        ((0, 0, at["A40"] + 30, [E, ("D", 1, None), E]), ("HP_DEL", 32)),                  # 32 of the 35 on the left + 1 + 4
        ((0, 0, at["A40"] + 34, [E, ("D", 1, None)]), ("HP_DEL", 32)),                     # the D of the run's last letter: 32 + 1 + 0
        ((16, 0, at["T50"], [E, ("D", 40, None), E]), ("HP_DEL", 32)),                     # a D longer than 32
        ((0, 0, at["A40"] + 15, [E, ("D", 40, None), E]), ("HP_DEL", 33)),                 # 20 A, the filler, 10 T: mixed
        ((16, 0, at["A31"] + 25, [E, ("D", 2, None), E]), ("HP_DEL", 33)),                 # A C: mixed
        ((0, 0, at["N3"] - 5, [E, ("D", 3, None), E]), ("HP_DEL", 33)),                    # N N N
        ((0, 0, n0 - 8, [("=", 6, None), ("D", 2, None)]), ("HP_DEL", 3)),                 # ends on s1: 1 + 2 + 0, the next sequence's A A A A A are not its own
        ((16, 1, 0, [("D", 2, None), E]), ("HP_DEL", 5)),                                  # begins on s0: 0 + 2 + 3, not the 3 of the sequence in front
        ((0, 1, 0, [("=", 1, None), ("D", 2, None), E]), ("HP_DEL", 5)),                   # 1 + 2 + 2
        # insertions
        ((0, 0, at["A31"] + 5, [E, ("I", 3, [1] * 3), E]), ("HP_INS", 31)),                # 10 + 21
        ((16, 0, at["A32"] + 5, [E, ("I", 3, [1] * 3), E]), ("HP_INS", 32)),
        ((0, 0, at["A33"] + 5, [E, ("I", 3, [1] * 3), E]), ("HP_INS", 32)),                # 33
        ((16, 0, at["A40"] + 30, [E, ("I", 1, [1]), E]), ("HP_INS", 32)),                  # 32 of 35 + 5
        ((0, 0, at["A40"] + 5, [E, ("I", 2, N2), E]), ("HP_INS", 33)),                     # an I of N
        ((16, 0, at["A40"] + 5, [E, ("I", 2, AC), E]), ("HP_INS", 33)),                    # mixed
        ((0, 0, 0, [("=", 1, None), ("I", 2, T2), E]), ("HP_INS", 0)),                     # T T between C and G: no equal neighbour
        ((16, 0, at["A2"] + 2, [("I", 2, A2), E]), ("HP_INS", 2)),                         # the first word: the run lies in front of the record
        ((0, 0, at["A2"] + 2, [("S", 3, None), ("I", 2, A2), E]), ("HP_INS", 2)),          # directly behind an S
        ((16, 0, at["A2"] - 5, [E, ("D", 2, None), ("I", 2, A2), E]), ("HP_INS", 2)),      # directly behind a D (of the two A: they are still the reference's)
        ((0, 0, at["A31"] - 5, [E, ("I", 2, A2), ("S", 3, None)]), ("HP_INS", 31)),        # the last word in front of a trailing S: the run lies behind the record
        ((16, 0, n0 - 6, [("=", 6, None), ("I", 2, A2)]), ("HP_INS", 3)),                  # p = s1: 3 + 0
        ((0, 1, 0, [("I", 2, A2), E]), ("HP_INS", 5)),                                     # p = s0: 0 + 5
        ((0, 0, at["T50"] + 48, [("=", 2, None), ("I", 40, [4] * 40), E]), ("HP_INS", 32)),      # 40 T behind 50 T: 32 + 0
    ]
    rec, words, reads = _assemble(text, lengths, [c for c, _ in cases])
    return text, lengths, rec, words, reads, [e for _, e in cases]
