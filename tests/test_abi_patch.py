"""The ranged-write entry points (include/pmc_codec.h "ranged writes") exist and validate before any HIP call: a
NULL context, a NULL store or a NULL array (n > 0) gives PMC_E_ARG.

On the CPU the handle is a dummy: the argument check answers before it looks into a handle, so a block of zero
bytes stands for a context or a store, and every array is NULL in turn, one at a time, beside valid others."""
import ctypes
import os

import pmc_codec

# src src_off src_len patch patch_off patch_len range_off | dst dst_off dst_cap dst_len rc
REWRITE_ARRAYS = (1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 12, 13)
STORE_ARRAYS = (1, 2, 3, 4, 5, 7)  # ext src src_off src_len range_off | rc


def each_null(args, positions):
    for k in positions:
        a = list(args)
        a[k] = None
        yield k, a


def test_the_three_symbols_exist():
    L = pmc_codec.lib()
    for name in ("pmc_gzip_rewrite_range_batch", "pmc_ctx_rewrite_counts", "pmc_store_set_range_batch"):
        assert name in pmc_codec.SIGNATURES and hasattr(L, name), name
    assert callable(pmc_codec.Context.rewrite_range_device) and callable(pmc_codec.Context.rewrite_counts)
    assert callable(pmc_codec.Store.set_range)


def test_rewrite_calls_reject_bad_arguments_without_touching_a_device():
    L = pmc_codec.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    fn = L.pmc_gzip_rewrite_range_batch
    assert fn(None, p, p, p, p, p, p, p, 1, p, p, p, p, p, None) == pmc_codec.E_ARG
    assert fn(None, None, None, None, None, None, None, None, 0, None, None, None, None, None, None) == pmc_codec.E_ARG
    assert L.pmc_ctx_rewrite_counts(None, (ctypes.c_uint64 * 5)()) == pmc_codec.E_ARG
    assert L.pmc_ctx_rewrite_counts(None, None) == pmc_codec.E_ARG
    g = L.pmc_store_set_range_batch
    assert g(None, p, p, p, p, p, 1, p) == pmc_codec.E_ARG
    assert g(None, None, None, None, None, None, 0, None) == pmc_codec.E_ARG


def test_null_array_is_rejected_behind_a_non_null_handle():
    L = pmc_codec.lib()
    handle = ctypes.create_string_buffer(4096)  # never looked into: the check answers first
    h = ctypes.addressof(handle)
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    for k, a in each_null([h, p, p, p, p, p, p, p, 1, p, p, p, p, p, None], REWRITE_ARRAYS):
        assert L.pmc_gzip_rewrite_range_batch(*a) == pmc_codec.E_ARG, k
    assert L.pmc_ctx_rewrite_counts(h, None) == pmc_codec.E_ARG
    for k, a in each_null([h, p, p, p, p, p, 1, p], STORE_ARRAYS):
        assert L.pmc_store_set_range_batch(*a) == pmc_codec.E_ARG, k
    # n == 0 is PMC_OK before anything is looked at
    assert L.pmc_gzip_rewrite_range_batch(h, None, None, None, None, None, None, None, 0, None, None, None, None, None,
                                          None) == 0
    assert L.pmc_store_set_range_batch(h, None, None, None, None, None, 0, None) == 0
    assert bytes(handle) == bytes(4096) and bytes(buf) == bytes(64)


def test_header_states_the_contract():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    h = open(os.path.join(root, "include", "pmc_codec.h")).read()
    assert "---- ranged writes ----" in h
    for name in ("pmc_gzip_rewrite_range_batch", "pmc_ctx_rewrite_counts", "pmc_store_set_range_batch"):
        assert name + "(" in h, name
    for word in ("BYTES:", "INTEGRITY:", "WRITES:", "Scratch:"):
        assert word in h.split("---- ranged writes ----")[1].split("---- preset dictionary")[0], word
