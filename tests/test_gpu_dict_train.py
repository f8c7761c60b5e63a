"""GPU: dictionary training (include/pmc_codec.h "dictionary training").

pmc_dict_train_batch and pmc_dict_train_host give the bytes of tests/dict_train_model.py on every case of
tests/dict_train_values.py -- one by one, and as one sequence of calls on one context with a single synchronisation;
nothing but dict[0 .. 64 m) and dict_len is written; a compress call on another stream behind a training call is
ordered with it; and a trained dictionary, once set, marks and round-trips every fast-level member of the two
baseline sets of tests/golden/dict_baseline.json."""
import json
import os
import zlib

import numpy as np
import pytest

from dict_train_model import train
from dict_train_values import all_cases
from dict_values import BASELINE_SETS, baseline_values

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GUARD = 0xA5
FRONT = 64  # canary bytes in front of dict


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401
    import pmc_codec
    c = pmc_codec.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def table(golden):
    """[(case, the model's dictionary)], computed once."""
    return [(c, train(c.samples, c.D)) for c in all_cases(golden.corpus)]


class Call:
    """The device tensors of one training call: the case's buffer as it is, a canaried dict, a prefilled dict_len."""

    def __init__(self, case):
        import torch
        self.case = case
        self.src = torch.from_numpy(np.frombuffer(case.src or b"\0", dtype=np.uint8).copy()).cuda()
        self.off = torch.from_numpy(np.array(case.offs, dtype=np.int64)).cuda()
        self.len = torch.from_numpy(np.array(case.lens, dtype=np.uint32).view(np.int32).copy()).cuda()
        self.buf = torch.full((FRONT + case.D + 64,), GUARD, dtype=torch.uint8, device="cuda")
        self.dlen = torch.full((1,), 12345, dtype=torch.int32, device="cuda")

    def enqueue(self, ctx, stream):
        ctx.train_dictionary_device(self.src, self.off, self.len, self.case.D, self.buf.data_ptr() + FRONT, self.dlen,
                                    stream)

    def check(self, want):
        name, got_len, buf = self.case.name, int(self.dlen.cpu()[0]), self.buf.cpu().numpy()
        assert got_len == len(want), (name, got_len, len(want))
        assert buf[FRONT:FRONT + got_len].tobytes() == want, name
        assert (buf[:FRONT] == GUARD).all() and (buf[FRONT + got_len:] == GUARD).all(), name


def test_device_call_gives_the_models_bytes_and_writes_nothing_else(ctx, table):
    import torch
    st = torch.cuda.current_stream().cuda_stream
    for case, want in table:
        call = Call(case)
        call.enqueue(ctx, st)
        torch.cuda.synchronize()
        call.check(want)


def test_the_whole_table_as_one_sequence_of_calls(ctx, table):
    """No synchronisation between the calls: each finds the scratch as the one before left it, table included; twice
    over, in both orders."""
    import torch
    st = torch.cuda.current_stream().cuda_stream
    for order in (table, table[::-1]):
        calls = [Call(case) for case, _ in order]
        torch.cuda.synchronize()
        for call in calls:
            call.enqueue(ctx, st)
        torch.cuda.synchronize()
        for call, (_, want) in zip(calls, order):
            call.check(want)


def test_host_call_gives_the_models_bytes(ctx, table):
    for case, want in table:
        assert ctx.train_dictionary(case.samples, case.D) == want, case.name


def test_host_call_writes_nothing_behind_the_dictionary(ctx, table):
    import ctypes
    import pmc_codec
    case, want = next((c, w) for c, w in table if c.name == "zero_identical")
    assert 0 < len(want) < case.D
    src = b"".join(case.samples)
    lens = np.array(case.lens, dtype=np.uint32)
    offs = np.concatenate([[0], np.cumsum(lens[:-1])]).astype(np.uint64)
    buf = np.full(FRONT + case.D + 64, GUARD, dtype=np.uint8)
    n = ctypes.c_uint32(12345)
    r = pmc_codec.lib().pmc_dict_train_host(ctx.handle, src, offs.ctypes.data, lens.ctypes.data, len(lens), case.D,
                                            buf.ctypes.data + FRONT, ctypes.byref(n))
    assert r == 0 and n.value == len(want) and buf[FRONT:FRONT + n.value].tobytes() == want
    assert (buf[:FRONT] == GUARD).all() and (buf[FRONT + n.value:] == GUARD).all()
    with pytest.raises(ValueError):
        ctx.train_dictionary(case.samples, 100)
    with pytest.raises(ValueError):
        ctx.train_dictionary([], 2048)


def test_training_and_compress_calls_on_two_streams(ctx, table, golden):
    """A training call on one stream, a compress call of the same context on another, with no host synchronisation
    between them, and then the other way round: the library orders them (they share the compress direction's lock
    and event), and both results are right.  The context is warmed with both shapes first, so that no call grows
    scratch, which would synchronise the device."""
    import torch
    import pmc_codec
    from oracle import pyoracle as O
    from pmc_codec import device as D
    case, want = next((c, w) for c, w in table if c.name == "seeded_8192")
    values = baseline_values(golden.corpus, "1k")
    members = [O.compress(v) for v in values]
    b = D.pack(values)
    caps = [pmc_codec.gzip_bound(len(v)) for v in values]

    def compress(stream):
        dst, doff, dcap = D.slots_for(caps)
        dlen = torch.zeros(b.n, dtype=torch.int32, device="cuda")
        rc = torch.full((b.n,), 7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        return (lambda: ctx.compress_device(b.data, b.off, b.len, dst, doff, dcap, dlen, rc, b.max_len, stream),
                lambda: (rc.cpu().numpy().tolist(), D.Batch(dst, doff, dlen, b.n, max(caps)).host_items()))

    null = torch.cuda.current_stream().cuda_stream
    Call(case).enqueue(ctx, null)
    compress(null)[0]()
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for first in ("train", "compress"):
        call = Call(case)
        run, result = compress(s2.cuda_stream)
        if first == "train":
            call.enqueue(ctx, s1.cuda_stream)
            run()
        else:
            run()
            call.enqueue(ctx, s1.cuda_stream)
        torch.cuda.synchronize()
        call.check(want)
        rcs, got = result()
        assert rcs == [0] * b.n and got == members, first


def test_trained_dictionary_end_to_end(ctx, table, golden):
    """Train on the seeded set, set the result, compress both baseline sets at the fast level: every member carries
    the trained id and round-trips, and the members sum to at most zlib level 1's total with the same zdict
    (tests/golden/dict_train_baseline.json), the rule tests/test_gpu_dict.py applies to the baseline dictionary."""
    import torch
    import pmc_codec
    from pmc_codec import device as D
    case, want = next((c, w) for c, w in table if c.name == "seeded_2048")
    d = ctx.train_dictionary(case.samples, 2048)
    assert d == want
    with open(os.path.join(GOLDEN, "dict_train_baseline.json")) as f:
        doc = json.load(f)
    assert doc["dict_crc32"] == zlib.crc32(d)
    ctx.set_dictionary(d)
    ctx.level = pmc_codec.LEVEL_FAST
    try:
        assert ctx.dictionary_id == zlib.crc32(d)
        for name in BASELINE_SETS:
            vals = baseline_values(golden.corpus, name)
            out, rc = D.compress(ctx, D.pack(vals))
            back, rc2 = D.decompress(ctx, out, [len(v) for v in vals])
            torch.cuda.synchronize()
            assert int((rc != 0).sum()) == 0 and int((rc2 != 0).sum()) == 0
            mem = out.host_items()
            assert all(int.from_bytes(m[4:8], "little") == zlib.crc32(d) and m[8] == 4 for m in mem), name
            assert back.host_items() == vals, name
            for m, v in zip(mem, vals):  # zlib reads them with the same zdict
                assert zlib.decompressobj(-15, zdict=d).decompress(m[10:-8]) == v
            total, bound = sum(map(len, mem)), doc["sets"][name]["level1_dict_total"]
            print(f"trained dict {name}: {total} B, level 1 + zdict {bound} ({total / bound:.4f}), level 9 + zdict "
                  f"{doc['sets'][name]['level9_dict_total']}")
            assert total <= bound, (name, total, bound)
    finally:
        ctx.set_dictionary(None)
        ctx.level = pmc_codec.LEVEL_EXACT
