"""CPU: the allocator model of tests/store_model.py and the churn script built on it.

The device test (tests/test_gpu_store_churn.py) holds the store to this script round by round; here the script
is held to the cases it is meant to reach, so the device test cannot pass by never meeting a full heap, a round
served by the free lists alone or an extent above the 8 KiB step."""
import re

import pytest

import store_model as M


@pytest.fixture(scope="module")
def planned(golden):
    return M.plan(golden.corpus)


def test_extent_cap_rule():
    """cap = round16(len); above 8192 rounded up to 1/8 of the largest power of two <= it."""
    want = {1: 16, 16: 16, 17: 32, 8176: 8176, 8177: 8192, 8192: 8192, 8193: 9216, 9216: 9216, 9217: 10240,
            16383: 16384, 16384: 16384, 16385: 18432, 20028: 20480, 32768: 32768, 32769: 36864, 70001: 73728,
            (1 << 20) + 1: (1 << 20) + (1 << 17)}
    assert {n: M.extent_cap(n) for n in want} == want
    for n in list(range(1, 600)) + list(range(8000, 40000, 7)):
        c = M.extent_cap(n)
        assert c >= n and c % 16 == 0 and M.extent_cap(c) == c
        assert c - n < (16 if c <= 8192 else 16 + c // 8)  # the waste is bounded by an eighth


def test_header_states_the_rule():
    """include/pmc_codec.h's store paragraph carries the rule the model restates."""
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"[\s*]+", " ", open(os.path.join(root, "include", "pmc_codec.h")).read())
    for phrase in ("rounded up to 16 B", "above 8192", "1/8 of the largest power of two", "last in, first out",
                   "PMC_Z_MEM_ERROR"):
        assert phrase in text, phrase


def test_allocator_model():
    al = M.Allocator(64 * 1024)
    a = al.alloc(100)
    b = al.alloc(9000)
    c = al.alloc(100)
    assert (a, b, c) == ((0, 112), (112, 9216), (9328, 112)) and al.used == al.reserved == 9440
    al.release(a[0])
    al.release(c[0])
    assert al.used == 9216 and al.reserved == 9440
    assert al.alloc(97) == c and al.alloc(112) == a  # last in, first out, by exact cap
    assert al.alloc(50000) == (9440, 53248)
    assert al.alloc(3000) is None and al.used == 9440 + 53248  # 62688 + 3008 > 65536: neither list nor bump
    assert al.alloc(2848) == (62688, 2848) and al.reserved == 65536
    al.release(b[0])
    assert al.alloc(8200) == b
    al.check()


def test_churn_script_reaches_its_cases(planned, golden):
    rounds, al = planned
    assert len(rounds) == M.ROUNDS and 100 <= M.KEYS <= 200
    full = [r for r, rd in enumerate(rounds) if M.Z_MEM_ERROR in rd.put_rc]
    lists_only = [r for r, rd in enumerate(rounds) if rd.from_lists and not rd.from_bump and M.Z_MEM_ERROR not in rd.put_rc]
    big = {e[1] for rd in rounds for e in rd.put_ext if e and e[1] > 8192}
    print("rounds with Z_MEM_ERROR", full, "from the free lists alone", lists_only, "caps above 8192", sorted(big))
    assert len(full) >= 2
    assert len(lists_only) >= 2
    assert all(rounds[r].after_put[1] == rounds[r - 1].after_round[1] for r in lists_only)
    assert len(big) >= 3
    # a full heap fails some values of a batch, not all, and a later value of the batch may still fit
    for r in full:
        rc = rounds[r].put_rc
        assert 0 in rc[rc.index(M.Z_MEM_ERROR):], r
    # every length of the issue's list is stored at least once, and an empty value is refused in most rounds
    stored = {len(v) for rd in rounds for (_, v), rc in zip(rd.puts, rd.put_rc) if rc == 0}
    assert stored >= set(M.JSON_LENS) | set(M.A_LENS) | set(M.STRADDLE_LENS) | set(M.NOISE_LENS)
    assert sum(M.INVALID_INPUT in rd.put_rc for rd in rounds) >= 8
    # the stored members straddle the 8192 step
    caps = {M.extent_cap(len(M.member_of(v))) for v in M.value_pool(golden.corpus) if len(v) in M.STRADDLE_LENS}
    assert caps == {8176, 8192, 9216}
    assert any(rd.replaced for rd in rounds) and any(rd.deletes for rd in rounds)


def test_churn_script_model_invariants(planned):
    rounds, al = planned
    reserved = 0
    live = {}
    for r, rd in enumerate(rounds):
        assert len(rd.puts) == len(rd.put_rc) == len(rd.put_ext)
        keys = [k for k, v in rd.puts if v]
        assert len(set(keys)) == len(keys), "the keys of a put batch are distinct"
        for (key, v), rc, e in zip(rd.puts, rd.put_rc, rd.put_ext):
            assert (rc == 0) == (e is not None) and (rc == M.INVALID_INPUT) == (not v)
            if e:
                assert e[2] == len(M.member_of(v)) and e[1] == M.extent_cap(e[2])
                live[key] = (v, e)
        for k in rd.deletes:
            del live[k]
        assert {k: v for k, (v, _) in live.items()} == rd.live
        assert M.disjoint_inside([(e[0], e[1]) for _, e in live.values()], M.HEAP), r
        assert rd.after_round[0] == sum(e[1] for _, e in live.values())
        assert reserved <= rd.after_put[1] == rd.after_round[1] <= M.HEAP
        assert rd.after_put[0] >= rd.after_round[0]
        reserved = rd.after_round[1]
    assert (al.used, al.reserved) == rounds[-1].after_round
    al.check()
