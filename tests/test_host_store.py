"""CPU: the host arithmetic of the device store (csrc/pmc_store_plan.hpp: the staging layouts, the wire framer, the
fallback round cutter and the heap allocator, which pmc_store.hip and pmc_group.hip turn into copies and launches),
printed by tests/host/store_check.cpp -- a stand-alone program built with the address and undefined-behaviour
sanitizers -- equals the statement of it here and the allocator model of tests/store_model.py."""
import json
import os
import subprocess
import tempfile

import pytest

import store_model as M

HERE = os.path.dirname(os.path.abspath(__file__))

# every staging layout: its u64 arrays, then its u32 arrays, in order; and the pairs one copy fetches
LAYOUTS = {
    "put": ("soff doff poff", "slen dcap dlen rc", ("dlen_rc",)),
    "get": ("soff doff", "slen dcap dlen rc", ("dlen_rc",)),
    "range_get": ("soff doff", "slen roff rlen dcap dlen rc", ("dlen_rc",)),
    "range_get_round": ("soff doff cut poff", "slen dcap dlen rc clen", ("dlen_rc",)),
    "range_set": ("soff poff doff noff", "slen plen roff dcap dlen rc", ()),
    "range_set_round": ("soff voff cut poff doff", "slen vcap vlen vrc plen dcap dlen rc", ("vlen_vrc", "dlen_rc")),
    "members": ("soff poff", "len rc", ()),
}
# what the call sites asked for before the layouts were named: meta = a * al256(8 m) + b * al256(4 m)
META = {"put": (3, 4), "get": (2, 4), "range_get": (2, 6), "range_get_round": (4, 5), "range_set": (4, 6),
        "range_set_round": (5, 8), "members": (2, 2)}
FALLBACK_BUDGET = 64 << 20


def al256(x):
    return (x + 255) & ~255


@pytest.fixture(scope="module")
def exe():
    d = tempfile.mkdtemp(prefix="pmc_store_")
    out = os.path.join(d, "store_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", out, os.path.join(HERE, "host", "store_check.cpp")])
    return out


def run(exe, *args, stdin=None):
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, input=stdin)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    return [json.loads(ln) for ln in out.stdout.splitlines()]


def test_layouts(exe):
    ms = [1, 31, 32, 33, 63, 64, 65, 1000, 40000]  # 8 m crosses 256 at 32, 4 m at 64
    got = run(exe, "layout", *ms)
    assert [g["m"] for g in got] == ms
    for m, g in zip(ms, got):
        assert g["bound_ok"] == 1, m  # host pointer = host base + offset, device pointer = device base + offset
        assert set(g) == set(LAYOUTS) | {"m", "bound_ok"}
        for name, (u64s, u32s, spans) in LAYOUTS.items():
            want, at, sizes = {}, 0, {}
            for width, names in ((8, u64s.split()), (4, u32s.split())):
                for a in names:
                    want[a], sizes[a] = at, m * width
                    at += al256(m * width)
            want["meta"] = at
            for sp in spans:
                want[sp] = 2 * al256(4 * m)
            assert g[name] == want, (m, name)
            assert list(g[name])[1:1 + len(sizes)] == list(sizes), (m, name)  # declaration order
            a8, a4 = META[name]
            assert g[name]["meta"] == a8 * al256(8 * m) + a4 * al256(4 * m), (m, name)
            # 256-aligned, disjoint, inside meta
            ends = sorted((g[name][a], g[name][a] + sizes[a]) for a in sizes)
            assert all(o % 256 == 0 for o, _ in ends), (m, name)
            assert all(e <= o2 for (_, e), (o2, _) in zip(ends, ends[1:])) and ends[-1][1] <= at, (m, name)
            # a span's two arrays are adjacent: the second starts where the first one's aligned bytes end
            for sp in spans:
                first, second = (sp.split("_")[0], sp.split("_")[1])
                assert g[name][second] == g[name][first] + al256(4 * m), (m, name, sp)


def test_framer(exe):
    Ls = [0, 1, 9, 10, 99, 100, 999999999, 1000000000, 4294967295]
    for frame in (0, 1, 2):
        got = run(exe, "frame", frame, *Ls)
        assert len(got) == len(Ls)
        for L, g in zip(Ls, got):
            head = b"$%d\r\n" % L if frame == 2 else b""
            tail = b"\r\n" if frame == 2 else b"\x1f" if frame == 1 else b""
            assert g == {"frame": frame, "L": L, "head": len(head), "tail": len(tail), "head_hex": head.hex(),
                         "tail_hex": tail.hex(), "touched_outside": 0}, (frame, L)


def rounds_of(lens, budget):
    """The rule, restated: values while their 16-byte-rounded lengths fit the budget, and the first one always."""
    out, w0 = [], 0
    while w0 < len(lens):
        w1, b = w0, 0
        while w1 < len(lens) and (w1 == w0 or b + M.round16(lens[w1]) <= budget):
            b += M.round16(lens[w1])
            w1 += 1
        out.append({"start": w0, "end": w1, "bytes": b, "max_raw": max([1] + lens[w0:w1])})
        w0 = w1
    return out


def test_cutter(exe):
    cases = {
        "all fit": [16, 16, 16],
        "sum equal to the budget": [16, 32, 16],
        "one more unit": [16, 32, 16, 16],
        "over budget first": [100, 16, 16],
        "over budget in the middle": [16, 100, 16],
        "over budget last": [16, 16, 100],
        "not multiples of 16": [1, 17, 15, 33, 48, 47, 2],
        "every one over": [65, 80, 1000],
        "empty": [],
    }
    want_ends = {"all fit": [3], "sum equal to the budget": [3], "one more unit": [3, 4], "over budget first": [1, 3],
                 "over budget in the middle": [1, 2, 3], "over budget last": [2, 3], "every one over": [1, 2, 3],
                 "not multiples of 16": [3, 4, 5, 7], "empty": []}
    for name, lens in cases.items():
        (g,) = run(exe, "cut", 64, *lens)
        assert g == {"budget": 64, "rounds": rounds_of(lens, 64)}, name
        assert [r["end"] for r in g["rounds"]] == want_ends[name], name
        # every item in exactly one round, in order; a round of more than one item is within the budget
        at = 0
        for r in g["rounds"]:
            assert r["start"] == at < r["end"], name
            assert r["bytes"] == sum(M.round16(x) for x in lens[at:r["end"]]), name
            assert r["end"] - at == 1 or r["bytes"] <= 64, name
            at = r["end"]
        assert at == len(lens), name
    assert want_ends["empty"] == [] and run(exe, "cut", 64)[0]["rounds"] == []
    # the library's budget: 64 values of 1 MiB fill it, the 65th opens a second round
    (g,) = run(exe, "cut", 0, *[1 << 20] * 65)
    assert g["budget"] == FALLBACK_BUDGET
    assert [(r["start"], r["end"], r["bytes"]) for r in g["rounds"]] == [(0, 64, 64 << 20), (64, 65, 1 << 20)]


def test_allocator_follows_the_model(exe, golden):
    """The churn script of tests/store_model.py as alloc and release operations through StoreHeap: after every
    operation offset, cap, used and reserved are the model's, and the allocs the model fails fail here too."""
    rounds, _ = M.plan(golden.corpus)
    al = M.Allocator(M.HEAP)
    ops, want = [], []
    holds = {}
    for rd in rounds:
        fresh = {}
        for (key, v), e in zip(rd.puts, rd.put_ext):
            if not v:
                continue
            n = len(M.member_of(v))
            before = (al.used, al.reserved)
            a = al.alloc(n)
            ops.append("a %d" % n)
            if a is None:
                assert e is None and (al.used, al.reserved) == before
                want.append({"ok": 0, "off": 0, "cap": M.extent_cap(n), "used": before[0], "reserved": before[1]})
                continue
            assert e == (a[0], a[1], n)
            want.append({"ok": 1, "off": a[0], "cap": a[1], "used": al.used, "reserved": al.reserved})
            fresh[key] = a[0]
        assert (al.used, al.reserved) == rd.after_put
        for off in [holds[k] for k in rd.replaced] + [fresh.get(k, holds.get(k)) for k in rd.deletes]:
            al.release(off)
            ops.append("r %d" % off)
            want.append({"used": al.used, "reserved": al.reserved})
        holds.update(fresh)
        for k in rd.deletes:
            del holds[k]
        assert (al.used, al.reserved) == rd.after_round
    assert sum(1 for w in want if w.get("ok") == 0) >= 2 and len(ops) > 500
    got = run(exe, "heap", M.HEAP, stdin="\n".join(ops) + "\n")
    assert len(got) == len(want)
    bad = [(i, ops[i], g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, bad[:4]
