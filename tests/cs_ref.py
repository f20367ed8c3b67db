"""The cs tag in plain Python: the rule (cs_from_cigar) and its inverse (cigar_from_cs, sequences_from_cs, edits_from_cs). The inverse
reads a string back without the rule's code, so a test that has a string checks it against its inputs, not against a second copy of the
walk: the long form gives back both sequences, the short form the letters at every X, I and D, and both the CIGAR words."""
import re

OPS = {"I": 1, "D": 2, "=": 7, "X": 8}
LETTERS = "NACGTN"          # ranks 1..4 -> ACGT, anything else -> N


def letter(rank):
    return LETTERS[int(rank)] if int(rank) < 6 else "N"


def letters(ranks):
    return "".join(letter(x) for x in ranks)


def cigar_words(text):
    """'10=1X' -> BAM words (len << 4 | op); S clips are left out (they are not part of a traced path)"""
    return [int(n) << 4 | OPS[o] for n, o in re.findall(r"(\d+)([ID=X])", text)]


def left_clip(text):
    """the rows a CIGAR's leading S clips"""
    m = re.match(r"(\d+)S", text)
    return int(m.group(1)) if m else 0


def cs_from_cigar(ref, begin, query, words, long):
    """minimap2's cs string of the path `words` that starts at column `begin` of ref and at the first row of query: every word emits on
    its own; = gives ':' + length (short) or '=' + the reference letters in upper case (long), X gives '*' + reference letter + query
    letter per column, I gives '+' + the query letters, D gives '-' + the reference letters, all lower case"""
    out, r, q = [], int(begin), 0
    for w in words:
        op, n = int(w) & 15, int(w) >> 4
        if op == 7:
            out.append("=" + letters(ref[r: r + n]) if long else f":{n}")
            r += n
            q += n
        elif op == 8:
            out.append("".join("*" + letter(ref[r + i]).lower() + letter(query[q + i]).lower() for i in range(n)))
            r += n
            q += n
        elif op == 1:
            out.append("+" + letters(query[q: q + n]).lower())
            q += n
        elif op == 2:
            out.append("-" + letters(ref[r: r + n]).lower())
            r += n
        else:
            raise ValueError(f"op {op}")
    return "".join(out).encode()


TOKEN = re.compile(r":[0-9]+|=[ACGTN]+|\+[acgtn]+|-[acgtn]+|(?:\*[acgtn][acgtn])+")


def tokens(cs):
    """the string cut into one token per CIGAR word (a run of '*' columns is one X word: neighbouring words never share an op)"""
    text = cs.decode()
    toks = TOKEN.findall(text)
    assert "".join(toks) == text, "bytes that no token holds"
    return toks


def cigar_from_cs(cs):
    words = []
    for t in tokens(cs):
        if t[0] == ":":
            assert t[1] != "0" or t == ":0", "a count with a leading zero"
            words.append(int(t[1:]) << 4 | 7)
        elif t[0] == "=":
            words.append((len(t) - 1) << 4 | 7)
        elif t[0] == "*":
            words.append((len(t) // 3) << 4 | 8)
        else:
            words.append((len(t) - 1) << 4 | (1 if t[0] == "+" else 2))
    return words


def sequences_from_cs(cs):
    """long form: (reference part, query part) of the record, upper case"""
    ref, query = [], []
    for t in tokens(cs):
        assert t[0] != ":", "a short-form token in a long string"
        if t[0] == "=":
            ref.append(t[1:])
            query.append(t[1:])
        elif t[0] == "*":
            ref.append(t[1::3].upper())
            query.append(t[2::3].upper())
        elif t[0] == "+":
            query.append(t[1:].upper())
        else:
            ref.append(t[1:].upper())
    return "".join(ref), "".join(query)


def edits_from_cs(cs):
    """either form: (the reference letters under X and D, the query letters at X and I), in path order, upper case"""
    ref, query = [], []
    for t in tokens(cs):
        if t[0] == "*":
            ref.append(t[1::3].upper())
            query.append(t[2::3].upper())
        elif t[0] == "+":
            query.append(t[1:].upper())
        elif t[0] == "-":
            ref.append(t[1:].upper())
    return "".join(ref), "".join(query)


def edits_of_inputs(ref, begin, query, words):
    """what edits_from_cs must give, read off the inputs by position"""
    r, q, rl, ql = int(begin), 0, [], []
    for w in words:
        op, n = int(w) & 15, int(w) >> 4
        if op in (8, 2):
            rl.append(letters(ref[r: r + n]))
        if op in (8, 1):
            ql.append(letters(query[q: q + n]))
        r += n if op != 1 else 0
        q += n if op != 2 else 0
    return "".join(rl), "".join(ql)


def check_inverse(cs, ref, begin, query, words, long, true_path=False):
    """a string against its inputs through the inverse alone; true_path: every '=' column pairs equal letters (a traced alignment), so
    the long form gives back the query itself"""
    words = [int(w) for w in words]
    assert cigar_from_cs(cs) == words
    span = sum(w >> 4 for w in words if w & 15 != 1)
    rows = sum(w >> 4 for w in words if w & 15 != 2)
    assert edits_from_cs(cs) == edits_of_inputs(ref, begin, query, words)
    if long:
        r, q = sequences_from_cs(cs)
        assert r == letters(ref[begin: begin + span]) and len(q) == rows
        if true_path:
            assert q == letters(query[:rows])
        # under '=' the string holds the reference's letters: the query's are theirs only where the path is a true one
        at, col = 0, int(begin)
        for w in words:
            op, n = w & 15, w >> 4
            if op != 2:
                want = letters(query[at: at + n]) if op != 7 else letters(ref[col: col + n])
                assert q[at: at + n] == want
                at += n
            col += n if op != 1 else 0


def slab_bound(nm, rows, long):
    """flx_internal.hpp cs_slab_bytes"""
    return rows + 3 * nm + 1 if long else 10 * nm + 7
