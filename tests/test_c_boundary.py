"""The C boundary of the extraction and container handles (csrc/snf_devmem.h `c_entry`, `c_create`; snf_extract.hip,
snf_container.h): six families, each with a thread-local error string of its own - extract, bgzf, bai (the index entry points of
the bgzf handle), deflate, fasta, vcftext.  What an entry point answers before it does any work: the return value and the exact
text, as the library answered before the families shared one helper.  No kernel is launched."""
import ctypes as C

import pytest

from sniffles_amd import abi, lib

NO_DEVICE = 1_000_000


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def L(request):
    if request.param == "emu":
        import emu.emu as E
        return E.lib()
    return lib.load()


def err(L, family):
    return getattr(L, f"snf_{family}_last_error")().decode()


def null_handle_calls(L):
    """family -> a call of one of its entry points with a null handle (every other argument valid or never looked at)."""
    bai_out, carry = abi.snf_bai_run_result_t(), abi.snf_bai_carry_t()
    return {"extract": lambda: L.snf_extract_run(None),
            "bgzf": lambda: L.snf_bgzf_inflate(None, None, 0, None, 0, C.byref(abi.snf_bam_carry_t())),
            "bai": lambda: L.snf_bai_run(None, None, C.byref(carry), C.byref(bai_out)),
            "deflate": lambda: L.snf_deflate_run(None, None, 0, None, 0, C.byref(abi.snf_deflate_result_t())),
            "fasta": lambda: L.snf_fasta_index(None, C.byref(abi.snf_fasta_index_result_t())),
            "vcftext": lambda: L.snf_vcftext_parse(None, 0, C.byref(abi.snf_vcftext_table_t()))}


def test_null_handle(L):
    for family, call in null_handle_calls(L).items():
        assert call() == 1, family
        assert err(L, family) == "null handle", family
    # the index entry point that checks its ranges before the device still looks at the handle first
    assert L.snf_csi_run(None, None, C.byref(abi.snf_bai_carry_t()), 7, 5, C.byref(abi.snf_bai_run_result_t())) == 1
    assert err(L, "bai") == "null handle"


def test_entries_that_check_arguments_first(L):
    """These look at all their pointers in one check, in front of everything else: a null handle is a null argument there."""
    assert L.snf_extract_result(None, C.byref(abi.snf_extract_result_t())) == 1 and err(L, "extract") == "null argument"
    assert L.snf_extract_result_meta(None, C.byref(abi.snf_extract_result_t())) == 1 and err(L, "extract") == "null argument"
    assert L.snf_bgzf_read_stream(None, 0, 0, None) == 1 and err(L, "bgzf") == "null argument"
    assert L.snf_bgzf_result(None, C.byref(abi.snf_bgzf_result_t())) == 1 and err(L, "bgzf") == "null argument"


def test_create_refuses_a_device_that_is_not_there(L):
    h = C.c_void_p()
    creates = {"extract": lambda: L.snf_extract_create(C.byref(abi.snf_extract_config_t()), NO_DEVICE, C.byref(h)),
               "bgzf": lambda: L.snf_bgzf_create(NO_DEVICE, C.byref(h)),
               "deflate": lambda: L.snf_deflate_create(NO_DEVICE, C.byref(h)),
               "fasta": lambda: L.snf_fasta_create(NO_DEVICE, 16, C.byref(h)),
               "vcftext": lambda: L.snf_vcftext_create(NO_DEVICE, 16, C.byref(h))}
    for family, create in creates.items():
        assert create() == 1, family
        assert err(L, family) == "device index out of range", family
        assert h.value is None, family
    # each create looks at its own arguments before it asks for the device
    assert L.snf_extract_create(None, NO_DEVICE, C.byref(h)) == 1 and err(L, "extract") == "snf_extract_create: null argument"
    for family in ("bgzf", "deflate"):
        assert getattr(L, f"snf_{family}_create")(NO_DEVICE, None) == 1 and err(L, family) == f"snf_{family}_create: null argument"
    for family in ("fasta", "vcftext"):
        assert getattr(L, f"snf_{family}_create")(NO_DEVICE, -1, C.byref(h)) == 1 and err(L, family) == f"snf_{family}_create: null argument"


def test_the_families_keep_their_own_strings(L):
    calls = null_handle_calls(L)
    assert L.snf_bgzf_read_stream(None, 0, 0, None) == 1 and err(L, "bgzf") == "null argument"
    assert calls["bai"]() == 1 and err(L, "bai") == "null handle"
    assert err(L, "bgzf") == "null argument"      # a failure of the index entry points is not the inflate's
    assert L.snf_extract_result(None, None) == 1
    for family in ("deflate", "fasta", "vcftext"):
        assert calls[family]() == 1
    assert err(L, "extract") == "null argument" and err(L, "bgzf") == "null argument" and err(L, "bai") == "null handle"


def test_what_a_handle_refuses_comes_back_as_text(L):
    """A live handle: the checks in front of the device, and what the work behind it throws, arrive in the family's string."""
    z = C.c_void_p()
    assert L.snf_bgzf_create(0, C.byref(z)) == 0
    try:
        out, carry = abi.snf_bai_run_result_t(), abi.snf_bai_carry_t()
        assert L.snf_bgzf_read_stream(z, 0, 0, None) == 1 and err(L, "bgzf") == "snf_bgzf_read_stream before a successful snf_bgzf_inflate"
        assert L.snf_bgzf_inflate(z, None, 0, None, 0, None) == 1 and err(L, "bgzf") == "snf_bgzf_inflate: null argument"
        assert L.snf_csi_run(z, None, C.byref(carry), 7, 5, C.byref(out)) == 1
        assert err(L, "bai") == "snf_csi_run: min_shift 7 / depth 5 out of range (min_shift 8..30, depth 1..10, min_shift + 3 depth at most 40)"
        assert L.snf_bai_run(z, None, C.byref(carry), C.byref(out)) == 1 and err(L, "bai") == "snf_bai_run: null argument"
        assert err(L, "bgzf") == "snf_bgzf_inflate: null argument"
    finally:
        L.snf_bgzf_destroy(z)
    x = C.c_void_p()
    assert L.snf_extract_create(C.byref(abi.snf_extract_config_t()), 0, C.byref(x)) == 0
    try:
        assert L.snf_extract_run(x) == 1 and err(L, "extract") == "snf_extract_run before snf_extract_upload"
        assert L.snf_extract_result(x, C.byref(abi.snf_extract_result_t())) == 1
        assert err(L, "extract") == "snf_extract_result before a successful snf_extract_run"
    finally:
        L.snf_extract_destroy(x)
    d = C.c_void_p()
    assert L.snf_deflate_create(0, C.byref(d)) == 0
    try:
        assert L.snf_deflate_run(d, None, 0, None, 0, None) == 1 and err(L, "deflate") == "snf_deflate_run: null argument"
    finally:
        L.snf_deflate_destroy(d)
    f = C.c_void_p()
    assert L.snf_fasta_create(0, 16, C.byref(f)) == 0
    try:
        assert L.snf_fasta_read_text(f, 0, 1, None) == 1 and err(L, "fasta") == "snf_fasta_read_text: null argument"
    finally:
        L.snf_fasta_destroy(f)
