"""The ranged-read entry points (include/pmc_codec.h "ranged reads") validate before any HIP call: a NULL
context, a NULL store, a NULL array (n > 0) or a frame outside PMC_FRAME_* gives PMC_E_ARG.

On the CPU the handle is a dummy: the argument check answers before it looks into a handle, so a block of zero
bytes stands for a context or a store, and every array is NULL in turn, one at a time, beside valid others.  On the
GPU the same cases run with a real Context and Store, next to the all-valid call, which is served: so each
PMC_E_ARG there is the one NULL's doing, and the counters show that it enqueued nothing."""
import ctypes
import os

import numpy as np
import pytest

import pmc_codec

RANGE_ARRAYS = (1, 2, 3, 4, 5, 7, 8, 9, 10, 11)  # src src_off src_len range_off range_len | dst dst_off dst_cap dst_len rc
STORE_ARRAYS = (1, 2, 3, 6, 7, 8)                # ext range_off range_len | resp resp_len rc
BAD_FRAMES = (-1, pmc_codec.FRAME_RESP + 1, 255)


def each_null(args, positions):
    """(position, args with that one argument NULL) for every array position."""
    for k in positions:
        a = list(args)
        a[k] = None
        yield k, a


def test_ranged_calls_reject_bad_arguments_without_touching_a_device():
    L = pmc_codec.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    fn = L.pmc_gzip_decompress_range_batch
    assert fn(None, p, p, p, p, p, 1, p, p, p, p, p, None) == pmc_codec.E_ARG
    assert fn(None, None, None, None, None, None, 0, None, None, None, None, None, None) == pmc_codec.E_ARG
    assert L.pmc_ctx_range_counts(None, (ctypes.c_uint64 * 3)()) == pmc_codec.E_ARG
    assert L.pmc_ctx_range_counts(None, None) == pmc_codec.E_ARG
    g = L.pmc_store_get_range_batch
    assert g(None, p, p, p, 1, pmc_codec.FRAME_RAW, p, p, p) == pmc_codec.E_ARG
    assert g(None, None, None, None, 0, pmc_codec.FRAME_RAW, None, None, None) == pmc_codec.E_ARG
    assert pmc_codec.E_NO_INDEX == -103
    assert "pmc_gzip_decompress_range_batch" in pmc_codec.SIGNATURES


def test_null_array_is_rejected_behind_a_non_null_handle():
    L = pmc_codec.lib()
    handle = ctypes.create_string_buffer(4096)  # never looked into: the check answers first
    h = ctypes.addressof(handle)
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    for k, a in each_null([h, p, p, p, p, p, 1, p, p, p, p, p, None], RANGE_ARRAYS):
        assert L.pmc_gzip_decompress_range_batch(*a) == pmc_codec.E_ARG, k
    assert L.pmc_ctx_range_counts(h, None) == pmc_codec.E_ARG
    for k, a in each_null([h, p, p, p, 1, pmc_codec.FRAME_RAW, p, p, p], STORE_ARRAYS):
        assert L.pmc_store_get_range_batch(*a) == pmc_codec.E_ARG, k
    for frame in BAD_FRAMES:
        assert L.pmc_store_get_range_batch(h, p, p, p, 1, frame, p, p, p) == pmc_codec.E_ARG, frame
        assert L.pmc_store_get_range_batch(h, None, None, None, 0, frame, None, None, None) == pmc_codec.E_ARG, frame
    assert bytes(handle) == bytes(4096) and bytes(buf) == bytes(64)


@pytest.mark.gpu
def test_null_array_is_rejected_with_a_real_context_and_store():
    import torch
    L = pmc_codec.lib()
    ctx = pmc_codec.Context(0)
    try:
        # a request that is valid in every argument: one member of 0 bytes, which has no index
        t = [torch.zeros(64, dtype=torch.uint8, device="cuda") for _ in range(9)]
        rc = torch.full((1,), 77, dtype=torch.int32, device="cuda")
        d = [x.data_ptr() for x in t]
        args = [ctx.handle, *d[:5], 1, *d[5:], rc.data_ptr(), None]
        before = ctx.range_counts()
        for k, a in each_null(args, RANGE_ARRAYS):
            assert L.pmc_gzip_decompress_range_batch(*a) == pmc_codec.E_ARG, k
        assert ctx.range_counts() == before and int(rc[0]) == 77
        assert L.pmc_gzip_decompress_range_batch(*args) == 0
        assert int(rc[0]) == pmc_codec.E_NO_INDEX
        assert ctx.range_counts() == dict(before, declined=before["declined"] + 1)
        assert L.pmc_ctx_range_counts(ctx.handle, None) == pmc_codec.E_ARG

        st = pmc_codec.Store(ctx, 1 << 20)
        try:
            value = os.urandom(16) * 8
            ext, prc = st.put([value])
            assert prc == [0]
            roff, rlen = np.array([3], dtype=np.uint32), np.array([5], dtype=np.uint32)
            resp, plen, grc = (ctypes.c_void_p * 1)(), np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.int32)
            args = [st.handle, ext, roff.ctypes.data, rlen.ctypes.data, 1, pmc_codec.FRAME_RAW, resp, plen.ctypes.data,
                    grc.ctypes.data]
            before = ctx.range_counts()
            for k, a in each_null(args, STORE_ARRAYS):
                assert L.pmc_store_get_range_batch(*a) == pmc_codec.E_ARG, k
            for frame in BAD_FRAMES:
                a = list(args)
                a[5] = frame
                assert L.pmc_store_get_range_batch(*a) == pmc_codec.E_ARG, frame
            assert resp[0] is None and int(plen[0]) == 0 and ctx.range_counts() == before
            assert L.pmc_store_get_range_batch(*args) == 0
            assert int(grc[0]) == 0 and ctypes.string_at(resp[0], int(plen[0])) == value[3:8]
        finally:
            st.close()
    finally:
        ctx.close()


def test_header_states_the_contract():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    h = open(os.path.join(root, "include", "pmc_codec.h")).read()
    assert "#define PMC_E_NO_INDEX (-103)" in h
    for name in ("pmc_gzip_decompress_range_batch", "pmc_ctx_range_counts", "pmc_store_get_range_batch"):
        assert name + "(" in h, name
