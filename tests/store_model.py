"""A plain model of the device store's host allocator (csrc/pmc_store_plan.hpp StoreHeap) and the churn script
that the store tests follow (tests/test_store_model.py and, through StoreHeap itself, tests/test_host_store.py on
the CPU, tests/test_gpu_store_churn.py on the device).

The allocator, as the header comment of pmc_store.hip and the store paragraph of include/pmc_codec.h state it:
an extent reserves cap = the member's length rounded up to 16 bytes; a cap above 8192 is rounded up again to a
multiple of 1/8 of the largest power of two that is <= it.  Freed extents go to a free list per exact cap, last
in first out; a request takes the newest entry of its cap's list, else bump-allocates at `reserved`, else -- the
list empty and the bump past the heap -- fails with Z_MEM_ERROR and changes nothing.

The script is a seeded sequence of rounds over KEYS keys.  A round is one put batch (new keys and overwrites,
an overwritten key's old extent is freed after the put, in batch order), one free batch (deletes, in order)
and a get of every live key.  It is generated with the model in the loop, with the member sizes of the oracle
(oracle/pyoracle.py compress), so every round carries what the store must answer: rc and extent per value,
`used` and `reserved` after the put and after the frees, and the value every key holds.  Nothing here calls
the library under test."""
import numpy as np

Z_MEM_ERROR = -4
INVALID_INPUT = -999
E_ARG = -102

KEYS = 150
ROUNDS = 12
SEED = 0x57A7E
# Chosen for the three conditions of tests/test_store_model.py: the script reserves 711,968 bytes up to round 7
# and would reserve 846,480 in all, so a heap of 704 KiB fits the first eight rounds and is full in the later ones.
HEAP = 720896

JSON_LENS = (1, 17, 255, 256, 257, 512, 513, 1024, 4096, 4097, 16382, 16383, 40000, 70001)
A_LENS = (1, 257, 4096, 16383, 70001)
# random bytes become one stored block: a member of len + 23 bytes, so 8169 is the last length whose extent
# is 8192 and 8170 the first that takes the 1/8 step above it (9216)
STRADDLE_LENS = (8150, 8160, 8169, 8170, 8177, 8210)
NOISE_LENS = (9000, 20000)
REFILL_ROUNDS = (3, 7, 10)  # put back exactly what the round before deleted: free lists only


def round16(n):
    return (n + 15) & ~15


def extent_cap(member_len):
    c = round16(member_len)
    if c > 8192:
        step = (1 << (c.bit_length() - 1)) // 8
        c = -(-c // step) * step
    return c


class Allocator:
    def __init__(self, heap):
        self.heap, self.reserved, self.used = heap, 0, 0
        self.free = {}  # cap -> offsets, newest last
        self.live = {}  # offset -> cap

    def alloc(self, member_len):
        """-> (off, cap), or None where neither a free list nor the bump can serve."""
        cap = extent_cap(member_len)
        lst = self.free.get(cap)
        if lst:
            off = lst.pop()
        elif self.reserved + cap <= self.heap:
            off = self.reserved
            self.reserved += cap
        else:
            return None
        self.used += cap
        self.live[off] = cap
        return off, cap

    def release(self, off):
        cap = self.live.pop(off)
        self.free.setdefault(cap, []).append(off)
        self.used -= cap

    def check(self):
        """The model's own invariants: live extents disjoint and inside the heap, used = their caps' sum,
        live and free extents together tile [0, reserved)."""
        assert self.used == sum(self.live.values())
        assert self.reserved <= self.heap
        spans = sorted(self.live.items())
        assert all(o + c <= o2 for (o, c), (o2, _) in zip(spans, spans[1:])), "live extents overlap"
        assert all(o + c <= self.reserved for o, c in spans)
        every = sorted(spans + [(o, c) for c, lst in self.free.items() for o in lst])
        at = 0
        for o, c in every:
            assert o == at, (o, at)
            at += c
        assert at == self.reserved


def disjoint_inside(extents, heap):
    """extents: (off, cap) pairs -> True where they are pairwise disjoint and inside [0, heap)."""
    spans = sorted(extents)
    return all(o + c <= o2 for (o, c), (o2, _) in zip(spans, spans[1:])) and all(0 <= o and o + c <= heap for o, c in spans)


def value_pool(corpus):
    rng = np.random.default_rng(SEED)
    vals = []
    for n in JSON_LENS:
        o = int(rng.integers(0, len(corpus) - n + 1))
        vals.append(corpus[o:o + n])
    vals += [b"a" * n for n in A_LENS]
    vals += [bytes(rng.integers(0, 256, n, dtype=np.uint8)) for n in STRADDLE_LENS + NOISE_LENS]
    return vals


_members = {}


def member_of(value):
    """The oracle's member of a value (kept: the script's values repeat)."""
    m = _members.get(value)
    if m is None:
        from oracle import pyoracle as O
        m = _members[value] = O.compress(value)
    return m


def wrap(frame, v):
    """The response of value v in frame 0 (raw), 1 (custom protocol) or 2 (RESP bulk string)."""
    return v if frame == 0 else v + b"\x1f" if frame == 1 else b"$%d\r\n" % len(v) + v + b"\r\n"


class Round:
    def __init__(self):
        self.puts = []       # (key, value)
        self.put_rc = []     # per put
        self.put_ext = []    # per put: (off, cap, len) or None
        self.replaced = []   # keys whose old extent is freed after the put, in order
        self.after_put = None    # (used, reserved)
        self.deletes = []    # live keys freed after that, in order
        self.after_round = None
        self.live = {}       # key -> value after the round
        self.from_lists = 0  # allocations served by a free list
        self.from_bump = 0


def plan(corpus, heap=HEAP):
    """-> (rounds, allocator after the last round).  Deterministic in (SEED, corpus, the oracle's sizes)."""
    rng = np.random.default_rng(SEED + 1)
    pool = value_pool(corpus)
    al = Allocator(heap)
    holds = {}  # key -> (value, off)
    rounds = []
    for r in range(ROUNDS):
        rd = Round()
        if r == 0:
            rd.puts = [(k, pool[(7 * k) % len(pool)]) for k in range(KEYS)]
            ndel = 30
        elif r in REFILL_ROUNDS:
            rd.puts = list(rounds[-1].deleted_values)
            ndel = 0
        else:
            keys = rng.choice(KEYS, 45, replace=False)
            rd.puts = [(int(k), pool[int(rng.integers(len(pool)))]) for k in keys]
            ndel = 30
        if r not in REFILL_ROUNDS:
            rd.puts.insert(int(rng.integers(len(rd.puts))), (int(rng.integers(KEYS)), b""))
        fresh = {}
        for key, v in rd.puts:
            if not v:
                rd.put_rc.append(INVALID_INPUT)
                rd.put_ext.append(None)
                continue
            before = al.reserved
            a = al.alloc(len(member_of(v)))
            if a is None:
                rd.put_rc.append(Z_MEM_ERROR)
                rd.put_ext.append(None)
                continue
            if al.reserved == before:
                rd.from_lists += 1
            else:
                rd.from_bump += 1
            rd.put_rc.append(0)
            rd.put_ext.append((a[0], a[1], len(member_of(v))))
            fresh[key] = (v, a[0])
        al.check()
        rd.after_put = (al.used, al.reserved)
        for key in fresh:
            if key in holds:
                rd.replaced.append(key)
                al.release(holds[key][1])
            holds[key] = fresh[key]
        cand = rng.permutation(KEYS)
        rd.deletes = [int(k) for k in cand if int(k) in holds][:ndel]
        rd.deleted_values = [(k, holds[k][0]) for k in rd.deletes]
        for k in rd.deletes:
            al.release(holds.pop(k)[1])
        al.check()
        rd.after_round = (al.used, al.reserved)
        rd.live = {k: v for k, (v, _) in holds.items()}
        rounds.append(rd)
    return rounds, al
