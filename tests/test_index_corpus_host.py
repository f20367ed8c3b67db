"""The promises of index_corpus.py, proved on the references of index_ref.py, and the host-built index against those references: what
the GPU test of the index kernels relies on without checking. No case may be left out: one that does not keep its promise fails here.
Runs anywhere."""
import ctypes as C

import numpy as np
import pytest

import floxer_amd as F
from floxer_amd import capi
import index_corpus as IC
import index_ref as R


def _by_class(cls):
    return [n for n in IC.NAMES if n.split("_")[0] == cls]


def test_names_and_classes():
    assert tuple(c.name for c in IC.cases()) == IC.NAMES
    assert all(c.cls == c.name.split("_")[0] for c in IC.cases())
    assert {c.cls for c in IC.cases()} == {"tiny", "block", "depth", "symbols", "filter"}
    assert set(IC.FILTER_NAMES) >= set(_by_class("filter")) and {n.split("_")[0] for n in IC.FILTER_NAMES} == {c.cls for c in IC.cases()}
    for c in IC.cases():
        n = len(IC.reference(c.name)["text"])
        assert n <= 20_000 and all(r.dtype == np.uint8 and len(r) >= 1 and r.min() >= 1 and r.max() <= 5 for r in c.refs)
        assert (n > 10_000) == (c.name in IC.LARGE)


# ------------------------------------------------------------------------------------------------ the references themselves
@pytest.mark.parametrize("name", IC.NAMES)
def test_references_are_consistent(name):
    """what the references must satisfy whatever the text: a sorted permutation, the BWT a permutation of the text that LF-maps back
    onto it, block counters that are the running sums of what the planes hold, an inverse that inverts"""
    ref = IC.reference(name)
    text, sa = ref["text"], ref["sa"]
    n = len(text)
    assert n % 4 == 0 and text[-1] == 0
    assert sorted(sa.tolist()) == list(range(n))
    tb = text.tobytes()
    assert all(tb[int(a):] < tb[int(b):] for a, b in zip(sa[:-1], sa[1:]))
    assert (ref["isa"][sa] == np.arange(n)).all() and (sa[ref["isa"]] == np.arange(n)).all()
    for b, t in ((ref["bwt0"], text), (ref["bwt1"], text[::-1])):
        assert (np.bincount(b, minlength=8) == np.bincount(t, minlength=8)).all()
    assert ref["bwt0"][ref["isa"][0]] == text[n - 1] and ref["bwt1"][int(np.flatnonzero(ref["sa_rev"] == 0)[0])] == text[0]
    for occ, b in ((ref["occ0"], ref["bwt0"]), (ref["occ1"], ref["bwt1"])):
        assert occ.shape == (n // 32 + 1, 8) and occ.dtype == np.uint32
        sym = np.zeros(occ.shape[0] * 32, dtype=np.uint8)
        for p in range(3):
            sym |= (((occ[:, 5 + p][:, None] >> np.arange(32, dtype=np.uint32)[None, :]) & 1) << p).astype(np.uint8).reshape(-1)
        assert (sym[:n] == b).all() and (sym[n:] == 7).all()
        for c in range(5):
            assert (occ[:, c] == np.concatenate([[0], np.cumsum((sym.reshape(-1, 32) == c).sum(axis=1))[:-1]])).all()


# ------------------------------------------------------------------------------------------------ the promises, class by class
@pytest.mark.parametrize("name", _by_class("tiny"))
def test_tiny_texts_are_shorter_than_the_initial_key(name):
    c = IC.case(name)
    n = len(IC.reference(name)["text"])
    assert n == c.props["n"] and n < 10
    assert sorted(IC.case(m).props["n"] for m in _by_class("tiny")) == [4, 4, 8, 8, 8, 8]
    assert [len(r) for r in IC.case("tiny_1_1").refs] == [1, 1]


@pytest.mark.parametrize("name", _by_class("block"))
def test_block_texts_have_their_lengths(name):
    c = IC.case(name)
    ref = IC.reference(name)
    n = len(ref["text"])
    nb = n // 32 + 1
    assert n == c.props["n"] == int(name.split("_")[1])
    assert (c.props["n_mod_32"], c.props["nb_mod_2"], c.props["last_block_empty"]) == (n % 32, nb % 2, n % 32 == 0)
    assert (ref["occ0"][-1, 5:] == 0xFFFFFFFF).all() == c.props["last_block_empty"]
    props = [IC.case(m).props for m in _by_class("block")]
    assert {p["n_mod_32"] for p in props} == {28, 0, 4} and {p["nb_mod_2"] for p in props} == {0, 1}
    assert {(p["nb_mod_2"], p["last_block_empty"]) for p in props} == {(0, False), (0, True), (1, False), (1, True)}
    for edge in (256, 4096):
        assert {edge - 4, edge, edge + 4} <= {p["n"] for p in props}


@pytest.mark.parametrize("name", _by_class("depth"))
def test_depth_texts_need_the_promised_round(name):
    c = IC.case(name)
    ref = IC.reference(name)
    lo, hi = c.props["distinct"]
    d = IC.max_lcp(ref["text"], ref["sa"]) + 1
    assert lo < d <= hi and (lo, hi) in list(zip(IC.STEPS, IC.STEPS[1:])), (d, lo, hi)


def test_depth_covers_both_sides_of_the_doubling_steps():
    depths = {n: IC.case(f"depth_homopolymer_{n}").props["distinct"] for n in IC.HOMOPOLYMERS}
    for h in (10, 20, 40, 5120):
        assert depths[h - 1][1] == depths[h][1] == h and depths[h + 1][0] == h
    assert [len(r) for r in IC.case("depth_three_identical").refs] == [3000] * 3 and len({r.tobytes() for r in IC.case("depth_three_identical").refs}) == 1
    assert len({r.tobytes() for r in IC.case("depth_two_identical").refs}) == 1
    a, b = IC.case("depth_prefix_2999").refs
    assert len(a) == 3000 and (a[:2999] == b).all()
    for p in (2, 3, 7):
        t = IC.case(f"depth_tandem_{p}").refs[0]
        assert len(t) == 3000 and (t[p:] == t[:-p]).all() and not any((t[q:] == t[:-q]).all() for q in range(1, p))
    t, tn = IC.case("depth_tandem_3").refs[0], IC.case("depth_tandem_3_n").refs[0]
    assert (t != tn).sum() == 1 and (tn == 5).sum() == 1


def test_depth_end_tie_ties_at_the_end_of_the_reversed_text():
    """the last ten symbols of the reversed text stand eight symbols earlier too; what follows them there is the smallest suffix of
    all, and twenty symbols from either start are past the end"""
    ref = IC.reference("depth_end_tie")
    rev = ref["text"][::-1]
    n = len(rev)
    i, j = n - 10, n - 18
    assert (rev[j:j + 10] == rev[i:]).all() and ref["sa_rev"][0] == j + 10 and j + 20 >= n
    assert rev[i - 1] != rev[j - 1]                                  # the two rows' BWT symbols differ: their order shows in the BWT


@pytest.mark.parametrize("name", _by_class("symbols"))
def test_symbols_texts(name):
    c = IC.case(name)
    text = IC.reference(name)["text"]
    if name == "symbols_only_n":
        assert len(c.refs) == 1 and (c.refs[0] == 5).all()
    elif name == "symbols_n_at_ends":
        assert all(r[0] == 5 and r[-1] == 5 for r in c.refs) and (c.refs[0][:5] == 5).all() and (c.refs[0][-3:] == 5).all()
    elif name == "symbols_fifty_singles":
        assert [len(r) for r in c.refs] == [1] * 50 and (text.reshape(-1, 4)[:, 1:] == 0).all() and (text == 0).sum() == 150
    else:
        assert all(len(r) % 4 == 0 for r in c.refs) and (text == 0).sum() == 4 * len(c.refs)


# ------------------------------------------------------------------------------------------------ filter
def _tables(name, k):
    f, m, tmin = IC.filter_reference(name, k)
    return f, m, tmin


def _bit(table, b):
    return (int(table[b >> 6]) >> (b & 63)) & 1


@pytest.mark.parametrize("k", IC.FILTER_KS)
@pytest.mark.parametrize("name", _by_class("filter"))
def test_filter_features_are_set_and_clear_kmers_are_clear(name, k):
    c = IC.case(name)
    f, m, tmin = _tables(name, k)
    feats = c.props["features"](k, tmin)
    if c.props.get("k", k) == k:
        assert feats, "a text that plants nothing at its own K"
    for label, first, count in feats:
        assert all(_bit(f, b) for b in range(first, first + count)), label
        if count == 1:
            assert _bit(m, R.code_mirrored([int(s) for s in _symbols_of(first, k)])), label
    for b in (c.props["clear"](k) if c.props.get("clear") else []):
        assert not _bit(f, b), R.spell(b, k)
        assert not _bit(m, R.code_mirrored(_symbols_of(b, k))), R.spell(b, k)
    assert f.any() and not f.all()
    # the mirrored table holds the full windows only, each under the mirrored code
    ranges, mirrored = R.filter_sets(IC.reference(name)["text"], k, tmin)
    full = {r[0] for r in ranges if r is not None and r[1] == 1}
    assert {R.code_of(_symbols_of(b, k)[::-1]) for b in (int(x) for x in _set_bits(m))} == full


def _symbols_of(code, k):
    return [((code >> (2 * i)) & 3) + 1 for i in range(k)]


def _set_bits(table):
    return np.flatnonzero(np.unpackbits(table.view(np.uint8), bitorder="little"))


@pytest.mark.parametrize("k", IC.FILTER_KS)
@pytest.mark.parametrize("j", range(IC.RUN_LENGTHS))
def test_filter_runs_texts_have_every_length_at_every_boundary(k, j):
    c = IC.case(f"filter_runs_{k}_{j}")
    text = IC.reference(c.name)["text"]
    n = len(text)
    tmin = R.filter_tmin_for(n, k)
    assert tmin == c.props["tmin"] == k - 3 and R.filter_k_for(n, str(k)) == k
    lengths = c.props["lengths"]
    assert lengths == sorted({tmin - 1, tmin, k - 4, k - 3, k - 1, k, k + 1}) and len(lengths) == IC.RUN_LENGTHS
    letter = lambda q: 0 <= q < n and 1 <= text[q] <= 4
    seen = set()
    for at, ln, bound in c.props["runs"]:
        assert all(letter(q) for q in range(at, at + ln)) and not letter(at - 1) and not letter(at + ln)
        left, right = (text[at - 1] if at else None), text[at + ln]
        assert {"start": left is None and right == 5, "delimiter": left in (0, None) and right == 0, "n": left == 5 and right == 5,
                "end": left == 5 and right == 0 and at + ln + (4 - len(c.refs[-1]) % 4) == n}[bound]
        seen.add((ln, bound))
    assert seen == {(ln, b) for ln in lengths for b in ("delimiter", "n")} | {(lengths[j], "start"), (lengths[j], "end")}


@pytest.mark.parametrize("k", IC.FILTER_KS)
def test_filter_span_and_block_plant_unique_windows_at_the_promised_positions(k):
    for name, want in (("filter_span", [64 * s + r for s in IC.SPAN_SPANS for r in IC.SPAN_RESIDUES]), ("filter_block", list(IC.BLOCK_ENDS))):
        c = IC.case(name)
        text = IC.reference(name)["text"]
        assert c.props["ends"] == want and {q % 64 for q in IC.case("filter_span").props["ends"]} == {62, 63, 0, 1}
        ranges, _ = R.filter_sets(text, k, R.filter_tmin_for(len(text), k))
        for q in want:
            assert ranges[q] is not None and ranges[q][1] == 1
            assert [p for p, r in enumerate(ranges) if r is not None and r[0] <= ranges[q][0] < r[0] + r[1]] == [q]      # set by this window end alone
    assert 16_500 <= len(IC.reference("filter_block")["text"]) <= 17_500


@pytest.mark.parametrize("k", IC.FILTER_KS)
def test_filter_ends_ext_and_homopolymer(k):
    f, _, tmin = _tables("filter_ends", k)
    assert int(f[0]) & 1 and int(f[-1]) >> 63
    f, _, tmin = _tables(f"filter_ext_{k}", k)
    feats = IC.case(f"filter_ext_{k}").props["features"](k, tmin)
    assert [cnt for _, _, cnt in feats] == [4, 16, 64] and feats[2][1] % 64 == 0 and f[feats[2][1] // 64] == np.uint64(2 ** 64 - 1)
    f, m, tmin = _tables("filter_homopolymer", k)
    # (the run grows from the text's start: the left extensions of its first tmin symbols hold those of the longer runs and the K-mer)
    assert len(_set_bits(f)) == 4 ** (k - max(tmin, k - 3)) and len(_set_bits(m)) == 1
    assert len(IC.case("filter_homopolymer").refs[0]) == 4096


# ------------------------------------------------------------------------------------------------ the host-built index
@pytest.mark.parametrize("name", IC.NAMES)
def test_host_built_index_is_the_reference(name):
    ref = IC.reference(name)
    idx = F.fmindex(IC.case(name).refs)
    assert idx.text_length == len(ref["text"])
    assert (idx.suffix_array_u32() == ref["sa"]).all() and (idx.suffix_array() == ref["sa"]).all()
    assert (idx.bwt() == ref["bwt0"]).all() and (idx.bwt(reversed_text=True) == ref["bwt1"]).all()
    n = len(ref["text"])
    assert idx.image_layout()[:4] == [ref["occ0"].nbytes, ref["occ1"].nbytes, 4 * n, len(R.text_buffer(ref["text"]))]


@pytest.mark.parametrize("name", IC.NAMES)
def test_python_k_and_tmin_agree_with_the_library_on_the_table_size(name):
    n = len(IC.reference(name)["text"])
    k = R.filter_k_default(n)
    assert R.FILTER_MIN_K <= k <= R.FILTER_MAX_K and R.filter_k_for(n) == k and max(1, k - 3) <= R.filter_tmin_for(n, k) <= k
    assert F.fmindex(IC.case(name).refs).derived_device_bytes == 4 * n + 8 * R.filter_words(k)


def test_python_k_and_tmin_at_chosen_lengths():
    """the rules, at lengths where they step (no text of the corpus is that long): K = ceil(log4 n) + 2 within [8, 19]"""
    assert [R.filter_k_default(n) for n in (1, 4 ** 6, 4 ** 6 + 1, 4 ** 7, 4 ** 7 + 1, 4 ** 16, 4 ** 16 + 1, 2 ** 40)] == [8, 8, 9, 9, 10, 18, 19, 19]
    assert [R.filter_k_for(1000, e) for e in ("0", "1", "8", "12", "19", "25")] == [0, 8, 8, 12, 19, 19]
    assert [R.filter_tmin_for(n, 12) for n in (100, 4 ** 9 // 2, 4 ** 9 // 2 + 1, 4 ** 11 // 2 + 1, 4 ** 13)] == [9, 9, 10, 12, 12]
    assert R.filter_tmin_for(17004, 8) == 8 and R.filter_tmin_for(17004, 9) == 8 and R.filter_tmin_for(17004, 12) == 9


def test_hook_refuses_null_arguments():
    L = capi.lib()
    info = capi.DerivedInfo()
    buf = np.zeros(4, dtype=np.uint32)
    assert L.flx_ctx_derived_info(None, C.byref(info)) == -1 and b"flx_ctx_derived_info" in L.flx_last_error()
    for which in (0, 1, 2, 3):
        assert L.flx_ctx_copy_derived(None, which, buf.ctypes.data_as(C.c_void_p), buf.nbytes) == -1 and b"flx_ctx_copy_derived" in L.flx_last_error()
    assert not buf.any()
