"""The kernels that build the index on the device (flx_index_build.hip) and the two that derive a context's tables from its image
(isa_kernel, filter_build_kernel of flx_search.hip) on the texts of index_corpus.py, against the plain references of index_ref.py:
every array whole and exact. The tables are read back through the hook flx_ctx_derived_info / flx_ctx_copy_derived, the image through
the torch tensors it was uploaded into."""
import functools

import numpy as np
import pytest

import floxer_amd as F
import index_corpus as IC
import index_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _cheap_contexts(monkeypatch):
    """two lanes per context; none of the variables a context reads when it is made is left over from the caller's environment"""
    monkeypatch.setenv("FLX_LANES", "2")
    for v in ("FLX_FILTER_K", "FLX_MIRRORED_FILTER", "FLX_NO_DERIVED"):
        monkeypatch.delenv(v, raising=False)


@functools.lru_cache(maxsize=None)
def _host_index(name):
    return F.fmindex(IC.case(name).refs)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    diff = np.argwhere(got != want)
    assert len(diff) == 0, f"{what}: {len(diff)} entries differ, first at {diff[0].tolist()}: got {got[tuple(diff[0])]}, want {want[tuple(diff[0])]}"


def _upload(idx):
    import torch
    image = [torch.zeros(n, dtype=torch.uint8, device="cuda:0") for n in idx.image_layout()]
    idx.image_upload(0, [b.data_ptr() for b in image])
    torch.cuda.synchronize()
    return image


def _read_back(image):
    occ0, occ1, sa, text, kmer = [b.cpu().numpy() for b in image]
    return occ0.view(np.uint32).reshape(-1, 8), occ1.view(np.uint32).reshape(-1, 8), sa.view(np.uint32), text, kmer.view(np.uint32)


def _filter_same(name, k, tmin, got, want, mirrored):
    assert got.shape == want.shape and got.dtype == want.dtype
    if not (got == want).all():
        pytest.fail(f"{name}, K = {k}, tmin = {tmin}, {'mirrored ' if mirrored else ''}filter:\n" +
                    R.explain_filter_mismatch(IC.reference(name)["text"], k, tmin, got, want, mirrored))


@pytest.mark.parametrize("name", IC.NAMES)
def test_device_built_index_image_and_inverse_are_the_reference(name):
    """the index built on the device (SA, both BWTs), the image of the host-built and of the device-built index as it stands in HBM
    (both occurrence tables word for word, the suffix array, the text between its guard bytes; the k-mer tables equal to each other),
    and the inverse suffix array of a context made on each image"""
    ref = IC.reference(name)
    n = len(ref["text"])
    dev = F.fmindex(IC.case(name).refs, device=0)
    assert dev.text_length == n
    _same(dev.suffix_array_u32(), ref["sa"], "device-built SA")
    _same(dev.bwt(), ref["bwt0"], "device-built BWT")
    _same(dev.bwt(reversed_text=True), ref["bwt1"], "device-built BWT of the reversed text")
    k = R.filter_k_default(n)
    kmers = []
    for who, idx in (("host-built", _host_index(name)), ("device-built", dev)):
        image = _upload(idx)
        occ0, occ1, sa, text, kmer = _read_back(image)
        _same(occ0, ref["occ0"], f"{who} image, occurrence blocks")
        _same(occ1, ref["occ1"], f"{who} image, occurrence blocks of the reversed text")
        _same(sa, ref["sa"], f"{who} image, SA")
        _same(text, R.text_buffer(ref["text"]), f"{who} image, text buffer")
        kmers.append(kmer)
        ctx = F.context(idx, image=image)
        try:
            assert ctx.derived_info() == dict(filter_k=k, filter_tmin=R.filter_tmin_for(n, k), have_isa=1, have_filter=1, have_filter_mirrored=0)
            _same(ctx.copy_derived("isa"), ref["isa"], f"{who} image, inverse suffix array")
            after = _read_back(image)
            for a, b, what in zip(after, (occ0, occ1, sa, text, kmer), ("occ0", "occ1", "sa", "text", "kmer")):
                _same(a, b, f"{who} image after the context was made, {what}")
        finally:
            ctx.close()
    _same(kmers[1], kmers[0], "k-mer table of the device-built image against the host-built one")


@pytest.mark.parametrize("k", IC.FILTER_KS)
@pytest.mark.parametrize("name", IC.FILTER_NAMES)
def test_filter_tables_are_the_reference(name, k, monkeypatch):
    """FLX_FILTER_K = k with and without FLX_MIRRORED_FILTER=1: every word of the filter, and of the mirrored one where it is asked for"""
    ref = IC.reference(name)
    n = len(ref["text"])
    want, want_m, tmin = IC.filter_reference(name, k)
    assert R.filter_k_for(n, str(k)) == k
    monkeypatch.setenv("FLX_FILTER_K", str(k))
    for mirrored in (1, 0):
        if mirrored:
            monkeypatch.setenv("FLX_MIRRORED_FILTER", "1")
        else:
            monkeypatch.delenv("FLX_MIRRORED_FILTER")
        ctx = F.context(_host_index(name))
        try:
            assert ctx.derived_info() == dict(filter_k=k, filter_tmin=tmin, have_isa=1, have_filter=1, have_filter_mirrored=mirrored)
            _filter_same(name, k, tmin, ctx.copy_derived("filter"), want, False)
            if mirrored:
                _filter_same(name, k, tmin, ctx.copy_derived("filter_mirrored"), want_m, True)
            else:
                with pytest.raises(F.FloxerError, match="no such table"):
                    ctx.copy_derived("filter_mirrored")
        finally:
            ctx.close()


def test_filter_at_the_default_k_of_a_larger_text():
    """no FLX_FILTER_K: filter_block has K = 10 by the rule, a K that no other test asks for"""
    name = "filter_block"
    n = len(IC.reference(name)["text"])
    k = R.filter_k_default(n)
    assert k == 10
    want, _, tmin = IC.filter_reference(name, k)
    ctx = F.context(_host_index(name))
    try:
        assert ctx.derived_info() == dict(filter_k=k, filter_tmin=tmin, have_isa=1, have_filter=1, have_filter_mirrored=0)
        _filter_same(name, k, tmin, ctx.copy_derived("filter"), want, False)
    finally:
        ctx.close()


def test_hook_refuses_what_it_cannot_copy(monkeypatch):
    """a wrong size and an unknown table are refused and copy nothing; FLX_FILTER_K=0 leaves the filter out, FLX_NO_DERIVED=1 everything"""
    import ctypes as C
    from floxer_amd import capi
    name = "block_260"
    ref = IC.reference(name)
    n = len(ref["text"])
    idx = _host_index(name)
    ctx = F.context(idx)
    try:
        L = capi.lib()
        for which, size in ((0, 4 * n), (1, 8 * R.filter_words(8))):
            for wrong in (size - 4, size + 4, 0):
                buf = np.full(size // 4 + 2, 0xA5A5A5A5, dtype=np.uint32)
                assert L.flx_ctx_copy_derived(ctx.h, which, buf.ctypes.data_as(C.c_void_p), wrong) == -1 and b"bytes" in L.flx_last_error()
                assert (buf == 0xA5A5A5A5).all()
        buf = np.zeros(n, dtype=np.uint32)
        assert L.flx_ctx_copy_derived(ctx.h, 3, buf.ctypes.data_as(C.c_void_p), buf.nbytes) == -1
        assert L.flx_ctx_copy_derived(ctx.h, -1, buf.ctypes.data_as(C.c_void_p), buf.nbytes) == -1
        assert L.flx_ctx_copy_derived(ctx.h, 0, None, buf.nbytes) == -1 and L.flx_ctx_derived_info(ctx.h, None) == -1
        _same(ctx.copy_derived("isa"), ref["isa"], "inverse suffix array after the refused calls")
    finally:
        ctx.close()
    monkeypatch.setenv("FLX_FILTER_K", "0")
    ctx = F.context(idx)
    try:
        assert ctx.derived_info() == dict(filter_k=0, filter_tmin=0, have_isa=1, have_filter=0, have_filter_mirrored=0)
        _same(ctx.copy_derived("isa"), ref["isa"], "inverse suffix array without a filter")
        for which in ("filter", "filter_mirrored"):
            with pytest.raises(F.FloxerError, match="no such table"):
                ctx.copy_derived(which)
    finally:
        ctx.close()
    monkeypatch.delenv("FLX_FILTER_K")
    monkeypatch.setenv("FLX_NO_DERIVED", "1")
    monkeypatch.setenv("FLX_MIRRORED_FILTER", "1")
    ctx = F.context(idx)
    try:
        assert ctx.derived_info() == dict(filter_k=0, filter_tmin=0, have_isa=0, have_filter=0, have_filter_mirrored=0)
        for which in ("isa", "filter", "filter_mirrored"):
            with pytest.raises(F.FloxerError, match="no such table"):
                ctx.copy_derived(which)
    finally:
        ctx.close()
