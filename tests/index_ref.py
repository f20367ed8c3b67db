"""Plain references for what the index holds and what a context derives from it: the padded text, the suffix array, both BWTs, the
occurrence blocks, the inverse suffix array and the presence filter (with its K and tmin). TEST INFRASTRUCTURE ONLY: nothing here calls
the product, every array is made with sorted(), loops and numpy from the rules written in DESIGN.md and flx_fm_core.hpp.

Symbols are ranks: 0 the sequence delimiter, 1..4 = A C G T, 5 = N.
"""
import numpy as np

TEXT_PAD = 256                       # guard bytes in front of and behind the text in the image's text buffer
OCC_BLOCK_POS = 32                   # text positions per occurrence block
FILTER_MIN_K, FILTER_MAX_K = 8, 19
LETTERS = "ACGT"


def padded_text(refs):
    """every sequence followed by 4 - len % 4 delimiters"""
    parts = []
    for r in refs:
        r = np.asarray(r, dtype=np.uint8)
        parts += [r, np.zeros(4 - len(r) % 4, np.uint8)]
    return np.concatenate(parts)


def suffix_array(text):
    """a suffix that ends first is smaller (bytes compare so)"""
    tb = np.asarray(text, dtype=np.uint8).tobytes()
    return np.array(sorted(range(len(tb)), key=lambda i: tb[i:]), dtype=np.uint32)


def bwt(text, sa):
    text = np.asarray(text, dtype=np.uint8)
    return text[(sa.astype(np.int64) - 1) % len(text)]


def inverse(sa):
    isa = np.empty(len(sa), dtype=np.uint32)
    isa[sa] = np.arange(len(sa), dtype=np.uint32)
    return isa


def occ_blocks(b):
    """(nb, 8) uint32: words 0..4 the counts of the symbols 0..4 in front of the block, words 5..7 the bit-planes of its 32 positions
    (bit k: position 32 * block + k); positions past the end hold the symbol 7"""
    n = len(b)
    nb = n // OCC_BLOCK_POS + 1
    out = np.zeros((nb, 8), dtype=np.uint32)
    count = [0] * 5
    for blk in range(nb):
        out[blk, :5] = count
        planes = [0, 0, 0]
        for k in range(OCC_BLOCK_POS):
            pos = blk * OCC_BLOCK_POS + k
            sym = int(b[pos]) if pos < n else 7
            for p in range(3):
                planes[p] |= ((sym >> p) & 1) << k
            if pos < n and sym < 5:
                count[sym] += 1
        out[blk, 5:] = planes
    return out


def text_buffer(text):
    """the image's text buffer: TEXT_PAD zeros, the text, zeros to its end (n + 2 * TEXT_PAD + 16 bytes)"""
    out = np.zeros(len(text) + 2 * TEXT_PAD + 16, dtype=np.uint8)
    out[TEXT_PAD:TEXT_PAD + len(text)] = text
    return out


# ------------------------------------------------------------------------------------------------ presence filter
def filter_k_default(n):
    """two symbols more than the text needs to tell its positions apart, within [FILTER_MIN_K, FILTER_MAX_K]"""
    bits = 0
    while (1 << bits) < n and bits < 63:
        bits += 1
    return min(FILTER_MAX_K, max(FILTER_MIN_K, (bits + 1) // 2 + 2))


def filter_k_for(n, env=None):
    """with FLX_FILTER_K = env (a string; None: unset): 0 means no filter, anything else is clamped"""
    if env is None:
        return filter_k_default(n)
    k = int(env)
    return 0 if k == 0 else max(FILTER_MIN_K, min(FILTER_MAX_K, k))


def filter_tmin_for(n, k):
    """the shortest string the filter answers for: held by a random text of n symbols with probability <= 1/2, at most 3 short of k"""
    t = 1
    while t < k and 4 ** t < 2 * n:
        t += 1
    return max(t, k - 3 if k >= 3 else 1)


def filter_words(k):
    return (4 ** k + 63) // 64


def code_of(symbols):
    """leftmost symbol lowest"""
    return sum((int(c) - 1) << (2 * i) for i, c in enumerate(symbols))


def code_mirrored(symbols):
    """rightmost symbol lowest"""
    return code_of(list(symbols)[::-1])


def spell(code, k, mirrored=False):
    s = "".join(LETTERS[(code >> (2 * i)) & 3] for i in range(k))
    return s[::-1] if mirrored else s


def filter_sets(text, k, tmin):
    """(bit ranges, mirrored bits) position by position: ranges[q] = (first bit, number of bits) that the run of A/C/G/T ending at q
    sets in the filter (None: nothing), mirrored[q] = the bit it sets in the mirrored table (None: nothing)"""
    ranges, mirrored = [], []
    run = 0
    for q, c in enumerate(text):
        run = min(run + 1, k) if 1 <= c <= 4 else 0
        window = text[q - run + 1:q + 1]
        if run == k:
            ranges.append((code_of(window), 1))
            mirrored.append(code_mirrored(window))
        elif tmin <= run < k and k - run <= 3:
            u = k - run
            ranges.append((code_of(window) << (2 * u), 4 ** u))           # every left extension: u free symbols below the run's
            mirrored.append(None)
        else:
            ranges.append(None)
            mirrored.append(None)
    return ranges, mirrored


def _pack(bits):
    return np.packbits(bits, bitorder="little").view(np.uint64)


def filter_tables(text, k, tmin):
    """(filter, mirrored filter) as uint64 words, bit b of the table = bit b % 64 of word b // 64"""
    ranges, mirrored = filter_sets(text, k, tmin)
    bits = np.zeros(filter_words(k) * 64, dtype=np.uint8)
    bits_m = np.zeros(filter_words(k) * 64, dtype=np.uint8)
    for r in ranges:
        if r is not None:
            bits[r[0]:r[0] + r[1]] = 1
    for m in mirrored:
        if m is not None:
            bits_m[m] = 1
    return _pack(bits), _pack(bits_m)


def explain_filter_mismatch(text, k, tmin, got, want, mirrored=False):
    """the first differing word of two filter tables in words: its bits, the K-mers they stand for and where the text holds them"""
    diff = np.flatnonzero(got != want)
    if len(diff) == 0:
        return None
    w = int(diff[0])
    ranges, mirr = filter_sets(text, k, tmin)
    lines = [f"{len(diff)} words differ; first: word {w}: got {int(got[w]):#018x}, want {int(want[w]):#018x}"]
    for bit in range(64):
        g, e = (int(got[w]) >> bit) & 1, (int(want[w]) >> bit) & 1
        if g == e:
            continue
        b = w * 64 + bit
        if mirrored:
            at = [q for q, m in enumerate(mirr) if m == b]
        else:
            at = [q for q, r in enumerate(ranges) if r is not None and r[0] <= b < r[0] + r[1]]
        lines.append(f"  bit {b} ({spell(b, k, mirrored)}): got {g}, want {e}; windows that set it end at text positions {at[:8]}")
        if len(lines) > 8:
            break
    return "\n".join(lines)
