"""The two things the shared column step and the per-block symbol patch of the DP kernels (flx_myers.hpp, ed_block_body) can break, through
F.align_batch against the oracle's matrix DP, bit-exact: windows that end anywhere in a 16-column block, in a reference pool that goes on
matching the query behind the window, and carries that cross the halves of a word, words and word groups. Needs an MI355X (-m gpu)."""
import numpy as np
import pytest

import floxer_amd as F
import align_corpus as AC

pytestmark = pytest.mark.gpu

END_RESIDUES = (0, 1, 2, 7, 8, 14, 15)                     # columns of the window's last block that lie inside it (0: all sixteen)
CARRY_ROWS = (31, 32, 33, 63, 64, 65, 127, 128, 129, 193)
# (4, 2): the four-word trace kernel keeps the plain 64-bit step (ed_block_body: kPlainStep), the other shapes run the three-input one
CARRY_SHAPES = ((1, 2), (2, 2), (3, 2), (4, 2))


@pytest.fixture(scope="module")
def ctx():
    idx = F.fmindex([np.random.default_rng(5).integers(1, 5, size=2000).astype(np.uint8)])
    c = F.context(idx)
    yield c
    c.close()


def _letters(rng, n):
    return rng.integers(1, 4, size=n).astype(np.uint8)


def _window_end_cases():
    """(case, what follows the window in the pool). `exact`: the window is junk + the whole query, the alignment ends in the window's last
    column with NM 0 (a column masked by mistake costs an error or moves the end). `short`: the window holds the query but for its last d
    rows, NM d by trailing insertions, and the pool goes on with exactly those d symbols (a column not masked would reach NM 0)."""
    rng = np.random.default_rng(20250)
    out = []
    for res in END_RESIDUES:
        for m in (40, 97, 145, 200):
            q = _letters(rng, m)
            lead = (res - m) % 16
            ref = np.concatenate([np.full(lead, 4, np.uint8), q])
            assert len(ref) % 16 == res
            out.append((AC.Case(f"exact_m{m}_end{res}", "window_end", ref, q, 3, {}), q[-16:]))
            d = (m - res) % 16 or 16
            ref = q[:m - d].copy()
            assert len(ref) % 16 == res and 40 <= m <= 200
            out.append((AC.Case(f"short_m{m}_end{res}_d{d}", "window_end", ref, q, d + 1, {}), np.concatenate([q[m - d:], q[:16]])))
    return out


def _pools(cases_and_tails, modes):
    """like AC.batch, but every window is followed in the reference pool by its own continuation; the last window ends on the pool's last byte"""
    refs, queries, jobs, what = [], [], [], []
    ro = qo = 0
    for i, (c, tail) in enumerate(cases_and_tails):
        for mode in modes:
            jobs.append((ro, len(c.ref), qo, len(c.query), c.k, mode))
            what.append((c, mode))
        follow = tail if i + 1 < len(cases_and_tails) else tail[:0]
        refs += [c.ref, follow]
        queries.append(c.query)
        ro += len(c.ref) + len(follow)
        qo += len(c.query)
    return np.concatenate(refs), np.concatenate(queries), jobs, what


def _compare(ctx, rpool, qpool, jobs, what, label):
    got = F.align_batch(ctx, qpool, jobs, reference_pool=rpool)
    assert len(got) == len(what)
    wrong = [(label, c.name, mode, str(g)[:120], str(AC.expected(c, mode))[:120]) for (c, mode), g in zip(what, got) if g != AC.expected(c, mode)]
    assert not wrong, (len(wrong), wrong[:8])


@pytest.mark.parametrize("few_waves", [None, "0"], ids=["common_shape", "per_job_shapes"])
def test_windows_that_end_inside_a_block(ctx, monkeypatch, few_waves):
    """n mod 16 in 0, 1, 2, 7, 8, 14, 15 with queries of 40 to 200 rows; every window but the last is followed by symbols that go on matching
    the query, the last one ends on the pool's last byte (every residue takes that place once); all three modes"""
    if few_waves is not None:
        monkeypatch.setenv("FLX_ALIGN_FEW_WAVES", few_waves)
    cases = _window_end_cases()
    assert {len(c.ref) % 16 for c, _ in cases} == set(END_RESIDUES)
    for c, _ in cases:                                     # the constructions hold: the oracle sees NM 0 / NM d, ending in the last column
        nm, end = AC.expected(c, 1)[:2]
        assert nm == (0 if c.name.startswith("exact") else c.k - 1), c.name
    for mode in (0, 1, 2):
        _compare(ctx, *_pools(cases, (mode,)), f"window ends, mode {mode}")
    # each residue once with its window on the pool's last byte, both constructions
    for i in range(0, len(cases), 8):
        for j in (0, 1):
            rot = cases[:i + j] + cases[i + j + 1:] + [cases[i + j]]
            _compare(ctx, *_pools(rot, (0, 1, 2)), f"window ends, {cases[i + j][0].name} last in the pool")


def _carry_cases():
    """queries of CARRY_ROWS rows with one run of 1 or 3 insertions or deletions (the run's letters are 4, everything else 1..3: no cheaper
    path than the run) that straddles row 32, row 64 or a word-group boundary of one to four words per lane (rows 64, 128, 192)"""
    rng = np.random.default_rng(20251)
    out = []
    for m in CARRY_ROWS:
        for pos in (32, 64, 128, 192):
            for L in (1, 3):
                s = pos - (L + 1) // 2                     # the run's first row: rows s .. s + L - 1 hold row pos - 1, and for L = 3 row pos too
                if s < 1 or s + L > m - 1:
                    continue
                q = _letters(rng, m)
                lead, trail = _letters(rng, 7), _letters(rng, 5)
                qi = q.copy()
                qi[s:s + L] = 4
                out.append(AC.Case(f"ins{L}_m{m}_row{pos}", "carry", np.concatenate([lead, qi[:s], qi[s + L:], trail]), qi, L + 1, {}))
                out.append(AC.Case(f"del{L}_m{m}_row{pos}", "carry", np.concatenate([lead, q[:pos], np.full(L, 4, np.uint8), q[pos:], trail]), q, L + 1, {}))
        q = _letters(rng, m)                               # and the exact query: every row's carry is a diagonal move
        out.append(AC.Case(f"exact_m{m}", "carry", np.concatenate([_letters(rng, 9), q, _letters(rng, 3)]), q, 2, {}))
    return tuple(out)


@pytest.mark.parametrize("shape", (None,) + CARRY_SHAPES, ids=lambda s: "default" if s is None else f"{s[0]},{s[1]}")
def test_carries_across_halves_words_and_groups(ctx, monkeypatch, shape):
    """the carry cases in the default shape and in forced shapes of one to four words per lane, all three modes (mode 2: the CIGARs come
    from K5's recomputation of the same step)"""
    cases = _carry_cases()
    assert {len(c.query) for c in cases} == set(CARRY_ROWS)
    if shape is not None:
        monkeypatch.setenv("FLX_FORCE_SHAPE", f"{shape[0]},{shape[1]}")
        monkeypatch.setenv("FLX_ALIGN_FEW_WAVES", "0")
    for mode in (0, 1, 2):
        rpool, qpool, jobs, what = AC.batch(cases, (mode,))
        if shape is not None:
            assert all((w, r) == shape for w, r, _ in F.align_shapes(jobs))
        _compare(ctx, rpool, qpool, jobs, what, f"carries {shape} mode {mode}")
    for c in cases:                                        # the planted run is what the oracle finds
        if c.name.startswith(("ins", "del")):
            assert AC.expected(c, 0)[0] == c.k - 1, c.name
