"""The corpus of select_corpus.py, checked on the CPU against the oracle: every cell of group count and row total the GPU test
(test_select_gpu.py) relies on is there with its exact numbers, every form of the device's anchor selection and both reasons for
handing a seed to the host get seeds under the configurations that allow them, and the seeds meant to erase anchors do. This is
what keeps the GPU test from passing on an empty case."""
import numpy as np
import pytest

import select_corpus as SC


def form(cnt, rows, hard, soft):
    """The class of a seed with `cnt` groups of `rows` rows in all, restated from the description of seed_rows_kernel (not imported):
    excluded over the hard cap by groups or rows; to the host with more than 512 groups or more than 64 rows to keep; light with at
    most 8 groups and 8 rows to keep (one thread); else one wave, in the form for up to 64 or up to 512 groups."""
    if cnt == 0:
        return "none"
    if cnt > hard or rows > hard:
        return "excluded"
    if cnt > 512:
        return "host_groups"
    keep = min(rows, soft)
    if keep > 64:
        return "host_rows"
    if cnt <= 8 and keep <= 8:
        return "light"
    return "wave64" if cnt <= 64 else "wave512"


@pytest.fixture(scope="module")
def corpus():
    c = SC.build()
    g = SC.groups()
    return c, {n: (len(x), int(x[:, 1].sum())) for n, x in zip(c.names, g)}, dict(zip(c.names, g))


def test_every_cell_is_present_with_its_numbers(corpus):
    c, cell, groups = corpus
    assert len(c.refs) >= 3 and len(c.seeds) <= 255
    for name, want in SC.CELLS.items():
        assert cell[name] == want, name
    for name, want in SC.CELL_GROUPS.items():
        got = len(SC.groups(name)) if name in c.extra else cell[name][0]
        assert got == want, name
    # the tied cells: every group one row and one error; the mixed ones: several group lengths and 0 and 1 errors
    for name in ("tied_16", "tied_17", "wave_63", "wave_64", "wave_65", "hard_count_500", "hard_count_501"):
        g = groups[name]
        assert set(g[:, 1].tolist()) == {1} and len(set(g[:, 2].tolist())) == 1, name
    for name in ("mixed_17", "mixed_40"):
        g = groups[name]
        assert len(set(g[:, 1].tolist())) >= 3 and set(g[:, 2].tolist()) == {0, 1}, name
    assert sorted(groups["soft_4_46"][:, 1].tolist()) == [1, 2, 3, 40]
    assert cell["wave_65_multi"][1] > 65 and int(groups["wave_65_multi"][:, 1].max()) > 1
    assert [cell[n] for n in ("nohit_a", "nohit_b")] == [(0, 0), (0, 0)]
    assert all(cell[n][0] >= 1 for n in ("random_a", "random_b", "random_c"))
    # no seed between 513 groups and the hard cap whose rows exceed the cap: the search stops such a seed at the cap, and how many of
    # its groups the device then sees depends on the order of the walk
    for name, (cnt, rows) in cell.items():
        assert not (cnt > 512 and rows > 2000), name


def test_copies_run_against_the_reference_ids_and_share_a_position(corpus):
    c, cell, groups = corpus
    a, _ = SC.expected(2000, 50, False)[c.names.index("light_9_9")]
    # three copies per sequence; the first of each at the same in-sequence position
    assert sorted(a[:, 1].tolist()) == [0, 0, 0, 1, 1, 1, 2, 2, 2]
    assert [int(a[a[:, 1] == r][:, 2].min()) for r in range(3)] == [SC.LEAD + SC.PRE] * 3
    # a group of several rows in more than one sequence
    a, _ = SC.expected(2000, 64, False)[c.names.index("single_1_60")]
    assert len(a) == 60 and set(a[:, 1].tolist()) == {0, 1, 2}


@pytest.mark.parametrize("hard,soft,erase", SC.CONFIGS)
def test_forms_and_host_reasons_are_not_empty(corpus, hard, soft, erase):
    c, cell, groups = corpus
    forms = {}
    for name in c.names:
        forms.setdefault(form(*cell[name], hard, soft), []).append(name)
    print(hard, soft, {k: len(v) for k, v in forms.items()})
    assert len(forms["none"]) == 2 and forms["light"] and forms["wave64"]
    assert bool(forms.get("excluded")) == (hard <= 500)      # (no seed of the corpus has more than 2000 groups or rows)
    # (a hard cap of 60 excludes every seed with more than 64 groups; under a soft cap of 65 such a seed keeps 65 rows: the host)
    if hard >= 65 and soft <= 64:
        assert len(forms["wave512"]) >= 3          # one block of the 512-form takes several seeds in turn (n_seeds / 256 + 1 = 1 block)
    if hard >= 513:
        assert forms["host_groups"] == ["groups_513"]
    if min(hard, soft) > 64:
        assert len(forms["host_rows"]) >= 3 and "soft_5_70" in forms["host_rows"] and "wave_65" in forms["host_rows"]
    else:
        assert "host_rows" not in forms
    # the boundaries themselves
    assert form(*cell["light_8_8"], hard, soft) == "light" and form(*cell["light_9_9"], hard, soft) == "wave64"
    assert form(*cell["light_8_9"], hard, soft) == ("light" if soft <= 8 else "wave64")
    if hard >= 500:
        assert form(*cell["wave_64"], hard, soft) == "wave64"
        assert form(*cell["wave_65"], hard, soft) == ("wave512" if soft <= 64 else "host_rows")
        assert form(*cell["hard_count_500"], hard, soft) == ("wave512" if soft <= 64 else "host_rows")
        assert form(*cell["hard_rows_500"], hard, soft) == ("host_rows" if soft == 65 else "light" if soft == 1 else "wave64")
        assert form(*cell["soft_5_70"], hard, soft) == ("host_rows" if soft == 65 else "light" if soft == 1 else "wave64")
    if hard == 500:
        assert form(*cell["hard_count_501"], hard, soft) == form(*cell["hard_rows_501"], hard, soft) == "excluded"
    if hard == 2000:
        assert form(*cell["groups_512"], hard, soft) == ("wave512" if soft <= 64 else "host_rows")


@pytest.mark.parametrize("hard,soft", [(500, 50), (2000, 64)])
def test_erasure_and_equal_positions_in_both_wave_forms(corpus, hard, soft):
    c, cell, groups = corpus
    erased = SC.expected(hard, soft, True)
    kept = SC.expected(hard, soft, False)
    seen = {"wave64": [0, 0], "wave512": [0, 0]}
    for i, name in enumerate(c.names):
        f = form(*cell[name], hard, soft)
        if f not in seen:
            continue
        useful, raw = int(erased[i][1][0]), int(erased[i][1][1])
        assert raw == int(kept[i][1][1]) == len(kept[i][0])
        seen[f][0] += 0 < useful < raw                                          # partly erased
        pos = [(int(r[1]), int(r[2])) for r in kept[i][0]]
        seen[f][1] += len(pos) != len(set(pos))                                # two anchors of equal position in one bucket
    assert all(v[0] >= 1 and v[1] >= 1 for v in seen.values()), seen
