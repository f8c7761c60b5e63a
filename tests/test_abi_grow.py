"""The growing-write entry points (include/pmc_codec.h "growing writes") exist and validate before any HIP call: a
NULL context, a NULL store or a NULL array (n > 0) gives PMC_E_ARG, n == 0 gives PMC_OK.

On the CPU the handle is a dummy, as in tests/test_abi_patch.py: the argument check answers before it looks into a
handle, so a block of zero bytes stands for a context or a store."""
import ctypes
import os

import pmc_codec
from test_abi_patch import REWRITE_ARRAYS, STORE_ARRAYS, each_null

APPEND_ARRAYS = (1, 2, 3, 4, 6)  # ext src src_off src_len | rc
NAMES = ("pmc_gzip_grow_range_batch", "pmc_store_grow_range_batch", "pmc_store_append_batch")


def test_the_three_symbols_exist():
    L = pmc_codec.lib()
    for name in NAMES:
        assert name in pmc_codec.SIGNATURES and hasattr(L, name), name
    assert pmc_codec.SIGNATURES["pmc_gzip_grow_range_batch"] == pmc_codec.SIGNATURES["pmc_gzip_rewrite_range_batch"]
    assert pmc_codec.SIGNATURES["pmc_store_grow_range_batch"] == pmc_codec.SIGNATURES["pmc_store_set_range_batch"]
    assert callable(pmc_codec.Context.grow_range_device)
    assert callable(pmc_codec.Store.grow_range) and callable(pmc_codec.Store.append)


def test_grow_calls_reject_bad_arguments_without_touching_a_device():
    L = pmc_codec.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    fn = L.pmc_gzip_grow_range_batch
    assert fn(None, p, p, p, p, p, p, p, 1, p, p, p, p, p, None) == pmc_codec.E_ARG
    assert fn(None, None, None, None, None, None, None, None, 0, None, None, None, None, None, None) == pmc_codec.E_ARG
    g = L.pmc_store_grow_range_batch
    assert g(None, p, p, p, p, p, 1, p) == pmc_codec.E_ARG
    assert g(None, None, None, None, None, None, 0, None) == pmc_codec.E_ARG
    a = L.pmc_store_append_batch
    assert a(None, p, p, p, p, 1, p) == pmc_codec.E_ARG
    assert a(None, None, None, None, None, 0, None) == pmc_codec.E_ARG


def test_null_array_is_rejected_behind_a_non_null_handle():
    L = pmc_codec.lib()
    handle = ctypes.create_string_buffer(4096)  # never looked into: the check answers first
    h = ctypes.addressof(handle)
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    for k, a in each_null([h, p, p, p, p, p, p, p, 1, p, p, p, p, p, None], REWRITE_ARRAYS):
        assert L.pmc_gzip_grow_range_batch(*a) == pmc_codec.E_ARG, k
    for k, a in each_null([h, p, p, p, p, p, 1, p], STORE_ARRAYS):
        assert L.pmc_store_grow_range_batch(*a) == pmc_codec.E_ARG, k
    for k, a in each_null([h, p, p, p, p, 1, p], APPEND_ARRAYS):
        assert L.pmc_store_append_batch(*a) == pmc_codec.E_ARG, k
    # n == 0 is PMC_OK before anything is looked at
    assert L.pmc_gzip_grow_range_batch(h, None, None, None, None, None, None, None, 0, None, None, None, None, None,
                                       None) == 0
    assert L.pmc_store_grow_range_batch(h, None, None, None, None, None, 0, None) == 0
    assert L.pmc_store_append_batch(h, None, None, None, None, 0, None) == 0
    assert bytes(handle) == bytes(4096) and bytes(buf) == bytes(64)


def test_header_states_the_contract():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    h = open(os.path.join(root, "include", "pmc_codec.h")).read()
    assert "---- growing writes ----" in h
    assert h.index("---- ranged writes ----") < h.index("---- growing writes ----") < h.index("---- preset dictionary")
    for name in NAMES:
        assert name + "(" in h, name
    section = h.split("---- growing writes ----")[1].split("---- preset dictionary")[0]
    for word in ("BYTES:", "INTEGRITY:", "WRITES:", "Scratch:", "pmc_ctx_rewrite_counts", "does not pad", "shrinking"):
        assert word in section, word
