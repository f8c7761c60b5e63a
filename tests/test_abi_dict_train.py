"""The dictionary-training entry points (include/pmc_codec.h "dictionary training") exist and validate before any HIP
call: a NULL context, n == 0, n > PMC_DICT_TRAIN_MAX_SAMPLES, a dict_size that is no multiple of 64 in [64, 8192] or
a NULL array gives PMC_E_ARG.

On the CPU the handle is a dummy, as in tests/test_abi_grow.py: the argument check answers before it looks into a
handle, so a block of zero bytes stands for a context."""
import ctypes
import os

import pmc_codec
from test_abi_patch import each_null

NAMES = ("pmc_dict_train_batch", "pmc_dict_train_host")
MAX_SAMPLES = 262144
BAD_SIZES = (0, 1, 32, 63, 65, 100, 2047, 8192 + 64, 16384, 0xFFFFFFC0)
# ctx src src_off src_len n dict_size dict dict_len [stream]
ARRAYS = (1, 2, 3, 6, 7)


def test_the_two_symbols_exist():
    L = pmc_codec.lib()
    for name in NAMES:
        assert name in pmc_codec.SIGNATURES and hasattr(L, name), name
    assert callable(pmc_codec.Context.train_dictionary) and callable(pmc_codec.Context.train_dictionary_device)


def calls(L):
    return ((L.pmc_dict_train_batch, (None,)), (L.pmc_dict_train_host, ()))


def test_bad_arguments_are_rejected_without_touching_a_device():
    L = pmc_codec.lib()
    handle = ctypes.create_string_buffer(4096)  # never looked into: the check answers first
    h = ctypes.addressof(handle)
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    for fn, tail in calls(L):
        assert fn(None, p, p, p, 1, 2048, p, p, *tail) == pmc_codec.E_ARG
        assert fn(h, p, p, p, 0, 2048, p, p, *tail) == pmc_codec.E_ARG
        assert fn(h, p, p, p, MAX_SAMPLES + 1, 2048, p, p, *tail) == pmc_codec.E_ARG
        assert fn(h, p, p, p, 0xFFFFFFFF, 2048, p, p, *tail) == pmc_codec.E_ARG
        for size in BAD_SIZES:
            assert fn(h, p, p, p, 1, size, p, p, *tail) == pmc_codec.E_ARG, size
        for size in (64, 2048, 8192):  # a good size, and still no device: a NULL array answers first
            for k, a in each_null([h, p, p, p, 1, size, p, p, *tail], ARRAYS):
                assert fn(*a) == pmc_codec.E_ARG, (size, k)
    assert bytes(handle) == bytes(4096) and bytes(buf) == bytes(64)


def test_host_call_refuses_more_than_256_mib_of_samples():
    """The truncated lengths are summed before the handle is looked into: 16387 samples of 16382 counted bytes each
    are 16378 bytes too many."""
    L = pmc_codec.lib()
    handle = ctypes.create_string_buffer(4096)
    n = 16387
    assert n * 16382 > 256 << 20 >= (n - 1) * 16382
    lens = (ctypes.c_uint32 * n)(*([0xFFFFFFFF] * n))
    offs = (ctypes.c_uint64 * n)()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    assert L.pmc_dict_train_host(ctypes.addressof(handle), p, ctypes.addressof(offs), ctypes.addressof(lens), n, 2048,
                                 p, p) == pmc_codec.E_ARG
    assert bytes(handle) == bytes(4096) and bytes(buf) == bytes(64)


def test_header_states_the_contract():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    h = open(os.path.join(root, "include", "pmc_codec.h")).read()
    assert "---- dictionary training ----" in h
    assert h.index("---- preset dictionary") < h.index("pmc_ctx_get_dictionary_id(") < \
        h.index("---- dictionary training ----") < h.index("---- single value, host memory")
    section = h.split("---- dictionary training ----")[1].split("---- single value, host memory")[0]
    for name in NAMES:
        assert name + "(" in section, name
    assert "#define PMC_DICT_TRAIN_MAX_SAMPLES 262144" in section
    for word in ("HASH.", "COUNT.", "EPOCHS.", "SCORE.", "SELECTION.", "ASSEMBLY.", "WRITES:", "Scratch:",
                 "Not provided:", "0x9E3779B185EBCA87", ">> 44", "d = 8", "K = 64", "F = 20", "W = K - d + 1 = 57",
                 "16382", "256 MiB", "only enqueues", "Neither call sets the dictionary", "CRC-32 is 0",
                 "lowest i, then the lowest q", "s_{m-1} || .. || s_1 || s_0", "plan_dict_train",
                 "store's extents", "group, slab and server wrappers", "rotation", "sample weighting"):
        assert word in section, word
