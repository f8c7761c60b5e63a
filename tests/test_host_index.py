"""CPU: the member index's host arithmetic (csrc/pmc_plan.hpp idx_plan and idx_parse, the rules of
pmc_gzip_index_info and of the decoder's scan), printed by tests/host/index_check.cpp -- a stand-alone program
built with the address and undefined-behaviour sanitizers -- equals tests/indexed_model.py's statement."""
import json
import os
import subprocess
import tempfile

import pytest

from indexed_model import C, MAX_CHUNKS, header, header_len, is_indexed, parse_index

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def exe():
    d = tempfile.mkdtemp(prefix="pmc_index_")
    out = os.path.join(d, "index_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", out, os.path.join(HERE, "host", "index_check.cpp")])
    return out


def run(exe, *args):
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    return [json.loads(ln) for ln in out.stdout.splitlines()]


def test_plan(exe):
    lens = [1, C - 1, C, C + 1, 2 * C - 1, 2 * C, 2 * C + 1, 100000, 1 << 20, MAX_CHUNKS * C - 1, MAX_CHUNKS * C,
            MAX_CHUNKS * C + 1, 4294967295]
    for got in run(exe, "plan", C, *lens):
        n = got["len"]
        want_k = -(-n // C) if is_indexed(n) else 1
        assert got == {"len": n, "indexed": int(is_indexed(n)), "K": want_k, "hdr": header_len(n)}, n
    rows = {r["len"]: r for r in run(exe, "plan", C, C, C + 1, MAX_CHUNKS * C, MAX_CHUNKS * C + 1)}
    assert rows[C] == {"len": C, "indexed": 0, "K": 1, "hdr": 10}
    assert rows[C + 1] == {"len": C + 1, "indexed": 1, "K": 2, "hdr": 24}
    assert rows[MAX_CHUNKS * C]["indexed"] == 1 and rows[MAX_CHUNKS * C]["hdr"] == 12 + 8 + 4 * (MAX_CHUNKS - 1)
    assert rows[MAX_CHUNKS * C + 1] == {"len": MAX_CHUNKS * C + 1, "indexed": 0, "K": 1, "hdr": 10}
    # the switch off, and another chunk size
    assert all(r["indexed"] == 0 and r["hdr"] == 10 for r in run(exe, "plan", 0, C + 1, 1 << 20))
    assert run(exe, "plan", 16384, 16385, 1 << 20) == [{"len": 16385, "indexed": 1, "K": 2, "hdr": 24},
                                                       {"len": 1 << 20, "indexed": 1, "K": 64, "hdr": 20 + 4 * 63}]


def test_parse(exe):
    """Headers with a dummy stream behind them: the parser reads the header, the offsets and ISIZE only."""
    def member(n, offsets, total, **kw):
        h = header(n, offsets, **kw)
        return h + bytes(total - len(h) - 8) + bytes(4) + (n & 0xFFFFFFFF).to_bytes(4, "little")

    good = member(2 * C + 5, [100, 200], 300)
    cases = {
        "good": good, "two_chunks": member(C + 1, [40], 60), "log2c_12": member(3 * 4096, [50, 70], 90, log2c=12),
        "log2c_24": member((1 << 24) + 1, [40], 60, log2c=24), "last_is_len-9": member(2 * C + 5, [100, 291], 300),
        "log2c_11": member(3 * 2048, [50, 70], 90, log2c=11), "log2c_25": member((1 << 25) + 1, [40], 60, log2c=25),
        "version2": member(2 * C + 5, [100, 200], 300, version=2), "id": member(2 * C + 5, [100, 200], 300, sid=b"IP"),
        "first_at_header": member(2 * C + 5, [28, 200], 300), "equal": member(2 * C + 5, [100, 100], 300),
        "decreasing": member(2 * C + 5, [200, 100], 300), "last_is_len-8": member(2 * C + 5, [100, 292], 300),
        "beyond": member(2 * C + 5, [100, 4000], 300), "k_low": member(3 * C + 5, [100, 200], 300),
        "k_high": member(C + 5, [100, 200], 300), "one_chunk": member(C, [], 60), "plain": b"\x1f\x8b\x08\x00" + bytes(60),
        "short": good[:27], "header_only": good[:28], "empty": b"", "no_room_for_trailer": good[:36],
    }
    names = list(cases)
    got = run(exe, "parse", *[cases[n].hex() if cases[n] else "" for n in names])
    for name, g in zip(names, got):
        want = parse_index(cases[name])
        if want is None:
            assert g["ok"] == 0, name
        else:
            isize = int.from_bytes(cases[name][-4:], "little")
            assert g == {"ok": 1, "chunk": want[0], "K": want[1], "isize": isize, "hdr": want[3]}, name
    ok = [n for n, g in zip(names, got) if g["ok"]]
    assert ok == ["good", "two_chunks", "log2c_12", "log2c_24", "last_is_len-9"], ok
