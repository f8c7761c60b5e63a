"""GPU: the device store (pmc_store_*) held to a model over many rounds, with a damaged heap, and with a put
and a get running at the same moment.

tests/store_model.py restates the allocator in plain Python and generates the churn script with the oracle's
member sizes; tests/test_store_model.py (CPU) holds that script to a full heap in at least two rounds, at least
two rounds served by the free lists alone and at least three extent sizes above 8192.  Expected bytes are the
oracle's members and the values the model holds; the store is never asked for its own expectation."""
import ctypes
import threading

import numpy as np
import pytest

import store_model as M

pytestmark = pytest.mark.gpu

FRAMES = (0, 1, 2)


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401
    import pmc_codec
    c = pmc_codec.Context(0)
    yield c
    c.close()


def ext_array(exts):
    """A pmc_extent array holding copies of exts."""
    import pmc_codec
    arr = (pmc_codec.Extent * max(len(exts), 1))()
    for i, e in enumerate(exts):
        arr[i] = e
    return arr


def ext_copy(e):
    import pmc_codec
    return pmc_codec.Extent(e.off, e.cap, e.len, e.raw_len, e.flags)


def fields(e):
    return (e.off, e.cap, e.len, e.raw_len, e.flags)


def check_get(st, exts, values, frames, tag):
    """One get of exts (frames: one PMC_FRAME_* or one per extent): every response is its value, framed."""
    per = [frames] * len(exts) if isinstance(frames, int) else list(frames)
    got = st.get(ext_array(exts), len(exts), frames)
    bad = [(i, got[i][0], len(got[i][1])) for i, v in enumerate(values) if got[i] != (0, M.wrap(per[i], v))]
    assert not bad, (tag, len(bad), bad[:8])


def test_store_churn_against_model(ctx, golden):
    import pmc_codec
    rounds, al = M.plan(golden.corpus)
    st = pmc_codec.Store(ctx, M.HEAP)
    holds = {}  # key -> the extent the store gave for it (a copy)
    for r, rd in enumerate(rounds):
        ext, rc = st.put([v for _, v in rd.puts])
        assert rc == rd.put_rc, (r, [(i, a, b) for i, (a, b) in enumerate(zip(rc, rd.put_rc)) if a != b][:8])
        fresh = {}
        for i, ((key, v), e) in enumerate(zip(rd.puts, rd.put_ext)):
            if e is None:  # an empty value (INVALID_INPUT) or a full heap (Z_MEM_ERROR): no extent
                assert fields(ext[i]) == (0, 0, 0, 0, 0), (r, i, fields(ext[i]))
                continue
            assert ext[i].len == len(M.member_of(v)) and ext[i].cap == M.extent_cap(ext[i].len), (r, i, fields(ext[i]))
            assert fields(ext[i]) == (e[0], e[1], e[2], len(v), 1), (r, i, fields(ext[i]), e)
            fresh[key] = ext_copy(ext[i])
        # the old extents of overwritten keys are still live here
        spans = [(e.off, e.cap) for e in holds.values()] + [(e.off, e.cap) for e in fresh.values()]
        assert M.disjoint_inside(spans, M.HEAP), r
        s = st.stats()
        assert (s["used"], s["reserved"], s["heap"]) == rd.after_put + (M.HEAP,), (r, s, rd.after_put)
        assert [k for k in fresh if k in holds] == rd.replaced
        st.free(ext_array([holds[k] for k in rd.replaced]), len(rd.replaced))
        holds.update(fresh)
        gone = ext_array([holds.pop(k) for k in rd.deletes])
        st.free(gone, len(rd.deletes))
        s = st.stats()
        assert (s["used"], s["reserved"]) == rd.after_round, (r, s, rd.after_round)
        if rd.deletes:  # the structs were marked empty: freeing them again changes nothing
            assert all(gone[i].flags == 0 for i in range(len(rd.deletes)))
            st.free(gone, len(rd.deletes))
            assert st.stats() == s, r
        assert M.disjoint_inside([(e.off, e.cap) for e in holds.values()], M.HEAP), r
        # every live key holds the model's value, in each frame and with a frame per extent
        keys = sorted(holds)
        assert keys == sorted(rd.live)
        exts, vals = [holds[k] for k in keys], [rd.live[k] for k in keys]
        for frame in FRAMES:
            check_get(st, exts, vals, frame, (r, frame))
        check_get(st, exts, vals, [(i + r) % 3 for i in range(len(keys))], (r, "frames"))
        if r == 5:  # one extent three times in a batch, not adjacent, in three frames
            big = max(range(len(keys)), key=lambda i: len(vals[i]))
            order = [big, 0, 1, big, 2, 3, 4, big, 5]
            check_get(st, [exts[i] for i in order], [vals[i] for i in order], [0, 2, 1, 1, 0, 2, 1, 2, 0], (r, "thrice"))
            check_get(st, [exts[i] for i in order], [vals[i] for i in order], 2, (r, "thrice RESP"))
        if r == 6:  # a freed extent and a zeroed one between live ones
            batch = ext_array([exts[0], gone[0], exts[1], pmc_codec.Extent(), exts[2]])
            assert gone[0].len > 0 and gone[0].flags == 0
            for frames in (0, 1, 2, [2, 2, 1, 0, 2]):
                per = [frames] * 5 if isinstance(frames, int) else frames
                got = st.get(batch, 5, frames)
                assert [got[1], got[3]] == [(pmc_codec.E_ARG, b"")] * 2, (frames, got[1], got[3])
                assert [got[i] for i in (0, 2, 4)] == [(0, M.wrap(per[i], vals[j])) for i, j in ((0, 0), (2, 1), (4, 2))]
        if r in (4, 9):  # the heap holds the oracle's members
            mem = st.members(ext_array(exts), len(exts))
            bad = [keys[i] for i, v in enumerate(vals) if mem[i] != M.member_of(v)]
            assert not bad, (r, bad[:8])
    # free everything, then put the last round's values again: from the free lists, or refused as before
    last = rounds[-1]
    keys = sorted(holds)
    for k in keys:
        al.release(holds[k].off)
    st.free(ext_array([holds[k] for k in keys]), len(keys))
    s = st.stats()
    assert (s["used"], s["reserved"]) == (0, last.after_round[1]) == (al.used, al.reserved)
    again = [v for _, v in last.puts if v]
    want = [al.alloc(len(M.member_of(v))) for v in again]
    al.check()
    ext, rc = st.put(again)
    assert rc == [0 if w else M.Z_MEM_ERROR for w in want] and rc.count(0) >= len(rc) - 4
    assert [(ext[i].off, ext[i].cap) for i, w in enumerate(want) if w] == [w for w in want if w]
    s = st.stats()
    assert (s["used"], s["reserved"]) == (al.used, al.reserved) and s["reserved"] == last.after_round[1]
    ok = [i for i, w in enumerate(want) if w]
    check_get(st, [ext[i] for i in ok], [again[i] for i in ok], 0, "again")
    st.close()


def _h2d(ptr, data):
    """Copy host bytes to device memory at ptr (HIP runtime through ctypes)."""
    hip = ctypes.CDLL("libamdhip64.so")
    buf = ctypes.create_string_buffer(bytes(data), len(data))
    assert hip.hipMemcpy(ctypes.c_void_p(ptr), buf, ctypes.c_size_t(len(data)), 1) == 0  # hipMemcpyHostToDevice


def oracle_verdict(damaged, raw_len):
    """What a read of a damaged member must answer: the oracle's rc at the extent's capacity, Z_DATA_ERROR
    where it decodes without error to another length than the extent records."""
    from oracle import pyoracle as O
    import pmc_codec
    rc, out = O.decompress(damaged, cap=raw_len, grow=False)
    return pmc_codec.Z_DATA_ERROR if rc == 0 and len(out) != raw_len else rc


def test_store_damaged_member(ctx, golden):
    """Four of 24 members damaged in the heap -- one bit in the deflate body, the CRC-32, ISIZE and the magic:
    every read of them answers the oracle's verdict and no bytes, and their 20 neighbours stay byte-exact."""
    import pmc_codec
    vals = [v for v in M.value_pool(golden.corpus) if len(v) <= 40000][:24]
    assert len(vals) == 24
    st = pmc_codec.Store(ctx, 4 << 20)
    ext, rc = st.put(vals)
    assert rc == [0] * 24
    mem = st.members(ext, 24)
    assert mem == [M.member_of(v) for v in vals]
    at = {len(v): i for i, v in enumerate(vals) if v[:2] != b"aa"}  # (the runs of b"a" share lengths with JSON slices)
    rng = np.random.default_rng(5)
    victims = {}  # index -> (position in the member, xor mask)
    # body: a seeded bit of the deflate stream that the oracle answers with a verdict
    i = at[4096]
    for _ in range(64):
        pos, bit = int(rng.integers(10, len(mem[i]) - 8)), 1 << int(rng.integers(8))
        d = bytearray(mem[i])
        d[pos] ^= bit
        if oracle_verdict(bytes(d), 4096) in (pmc_codec.Z_DATA_ERROR, pmc_codec.Z_BUF_ERROR):
            victims[i] = (pos, bit)
            break
    assert i in victims
    victims[at[1024]] = (len(mem[at[1024]]) - 6, 0x10)   # CRC-32 trailer
    victims[at[16383]] = (len(mem[at[16383]]) - 4, 0x01)  # ISIZE
    victims[at[8170]] = (0, 0x01)                         # magic
    want_rc = {}
    for i, (pos, bit) in victims.items():
        d = bytearray(mem[i])
        d[pos] ^= bit
        want_rc[i] = oracle_verdict(bytes(d), len(vals[i]))
        assert want_rc[i] in (pmc_codec.Z_DATA_ERROR, pmc_codec.Z_BUF_ERROR), (i, want_rc[i])
        assert pos < ext[i].len and ext[i].off + ext[i].len <= 4 << 20
        _h2d(st.data_ptr() + ext[i].off + pos, bytes([d[pos]]))
    assert len(want_rc) == 4
    after = st.members(ext, 24)
    assert [i for i in range(24) if after[i] != mem[i]] == sorted(victims)
    ranges = [(len(v) // 3, len(v) // 2 + 1) for v in vals]
    cut = [v[o:o + n] for v, (o, n) in zip(vals, ranges)]
    assert all(c for c in cut)
    for frame in FRAMES:
        for tag, got, whole in (("get", st.get(ext, 24, frame), vals), ("get_range", st.get_range(ext, ranges, 24, frame), cut)):
            want = [(want_rc[i], b"") if i in victims else (0, M.wrap(frame, whole[i])) for i in range(24)]
            bad = [(i, len(vals[i]), got[i][0], len(got[i][1])) for i in range(24) if got[i] != want[i]]
            assert not bad, (tag, frame, bad)
    st.close()


def test_store_put_and_get_from_two_threads(ctx, golden):
    """A put and a get of one store at the same moment from two threads (include/pmc_codec.h allows it and the
    server does it every iteration): 20 put batches of 100 fresh values beside 20 gets of 200 resident ones."""
    import pmc_codec
    corpus = golden.corpus
    rng = np.random.default_rng(77)

    def piece(n):
        o = int(rng.integers(0, len(corpus) - n + 1))
        return corpus[o:o + n]

    resident = [piece((17, 256, 1024, 4096, 4097, 700, 16383, 90)[i % 8]) for i in range(200)]
    batches = [[piece(int(rng.integers(64, 2001))) for _ in range(100)] for _ in range(20)]
    members = [[M.member_of(v) for v in b] for b in batches]  # (the oracle, before the threads start)
    al = M.Allocator(64 << 20)
    st = pmc_codec.Store(ctx, 64 << 20)
    rext, rc = st.put(resident)
    assert rc == [0] * 200
    for v in resident:
        al.alloc(len(M.member_of(v)))
    barrier = threading.Barrier(2)
    put_out, get_out, errors = [], [], []

    def putter():
        try:
            barrier.wait(30)
            for b in batches:
                put_out.append(st.put(b))
        except Exception as e:  # noqa: BLE001
            errors.append(("put", repr(e)))

    def getter():
        try:
            barrier.wait(30)
            for k in range(20):
                frames = k % 4 if k % 4 < 3 else [(i + k) % 3 for i in range(200)]
                get_out.append((frames, st.get(rext, 200, frames)))
        except Exception as e:  # noqa: BLE001
            errors.append(("get", repr(e)))

    threads = [threading.Thread(target=putter, daemon=True), threading.Thread(target=getter, daemon=True)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(60)
    if any(t.is_alive() for t in threads):
        pytest.fail("a store call did not return within 60 s: no further device work is started")
    assert not errors, errors
    assert len(put_out) == 20 and len(get_out) == 20
    for k, (frames, got) in enumerate(get_out):
        per = [frames] * 200 if isinstance(frames, int) else frames
        bad = [i for i, v in enumerate(resident) if got[i] != (0, M.wrap(per[i], v))]
        assert not bad, ("get", k, bad[:8])
    for k, (ext, rc) in enumerate(put_out):
        assert rc == [0] * 100, ("put", k)
        for v in batches[k]:
            al.alloc(len(M.member_of(v)))
        assert st.members(ext, 100) == members[k], ("members", k)
    every = [ext[i] for ext, _ in put_out for i in range(100)]
    check_get(st, every, [v for b in batches for v in b], [i % 3 for i in range(2000)], "all of the putter's")
    spans = [(e.off, e.cap) for ext, _ in put_out for e in ext] + [(rext[i].off, rext[i].cap) for i in range(200)]
    assert M.disjoint_inside(spans, 64 << 20)
    al.check()
    s = st.stats()
    assert (s["used"], s["reserved"]) == (al.used, al.reserved)
    st.close()
