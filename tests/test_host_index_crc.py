"""CPU: the chunk CRCs' host arithmetic (csrc/pmc_plan.hpp idx_plan with the CRC switch and idx_crc_parse, the
rules of pmc_gzip_index_crc_info and of the ranged read's scan), printed by tests/host/index_crc_check.cpp -- a
stand-alone program built with the address and undefined-behaviour sanitizers -- equals
tests/indexed_crc_model.py's statement."""
import json
import os
import subprocess
import tempfile

import pytest

from indexed_crc_model import CRC_MAX_CHUNKS, assemble_crc, chunk_crcs, crc_defects, crc_subfield, parse_chunk_crcs, plan
from indexed_model import C, MAX_CHUNKS, assemble

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def exe():
    d = tempfile.mkdtemp(prefix="pmc_index_crc_")
    out = os.path.join(d, "index_crc_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", out, os.path.join(HERE, "host", "index_crc_check.cpp")])
    return out


def run(exe, *args):
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    return [json.loads(ln) for ln in out.stdout.splitlines()]


def row(n, chunk, crc):
    indexed, k, hdr, crcs, at = plan(n, chunk, crc)
    return {"len": n, "indexed": int(indexed), "K": k, "hdr": hdr, "crcs": int(crcs), "crc_at": at}


def test_plan(exe):
    lens = [1, C, C + 1, 2 * C, 2 * C + 3, 100000, 1 << 20, (CRC_MAX_CHUNKS - 1) * C + 1, CRC_MAX_CHUNKS * C,
            CRC_MAX_CHUNKS * C + 1, MAX_CHUNKS * C, MAX_CHUNKS * C + 1, 4294967295]
    for crc in (0, 1):
        assert run(exe, "plan", C, crc, *lens) == [row(n, C, bool(crc)) for n in lens]
    on = {r["len"]: r for r in run(exe, "plan", C, 1, *lens)}
    # K = 8190 carries CRCs (XLEN = 65532); 8191 and 16382 are the plain indexed member; 16383 is not indexed
    assert on[CRC_MAX_CHUNKS * C] == {"len": CRC_MAX_CHUNKS * C, "indexed": 1, "K": 8190, "hdr": 12 + 65532, "crcs": 1,
                                      "crc_at": 20 + 4 * 8189 + 8}
    assert on[CRC_MAX_CHUNKS * C + 1] == {"len": CRC_MAX_CHUNKS * C + 1, "indexed": 1, "K": 8191, "hdr": 20 + 4 * 8190,
                                          "crcs": 0, "crc_at": 0}
    assert on[MAX_CHUNKS * C] == {"len": MAX_CHUNKS * C, "indexed": 1, "K": 16382, "hdr": 20 + 4 * 16381, "crcs": 0, "crc_at": 0}
    assert on[MAX_CHUNKS * C + 1] == {"len": MAX_CHUNKS * C + 1, "indexed": 0, "K": 1, "hdr": 10, "crcs": 0, "crc_at": 0}
    assert on[C + 1] == {"len": C + 1, "indexed": 1, "K": 2, "hdr": 40, "crcs": 1, "crc_at": 32}
    # the index switch off, and another chunk size
    assert all(r["indexed"] == 0 and r["crcs"] == 0 and r["hdr"] == 10 for r in run(exe, "plan", 0, 1, C + 1, 1 << 20))
    assert run(exe, "plan", 16384, 1, 16385, 1 << 20) == [row(16385, 16384, True), row(1 << 20, 16384, True)]


def test_parse(exe, golden):
    # (chunks of 4 KiB keep the byte strings short enough for a command line)
    c4 = 4096
    v = (golden.corpus * 4)[100:100 + 2 * c4 + 3]
    good = assemble_crc(v, c4)
    cases = {"good": good, "four_chunks": assemble_crc(v + v[:c4 - 2], c4), "two_chunks": assemble_crc(v[:c4 + 1], c4),
             "bytes_behind_it": assemble_crc(v, c4, sub=crc_subfield(chunk_crcs(v, c4)) + b"ZZ\x01\x00!"),
             "plain": assemble(v, c4)}
    for name, sub in crc_defects(v, c4).items():
        cases["defect:" + name] = assemble_crc(v, c4, sub=sub)
    cases.update({"index_version2": good[:16] + b"\x02" + good[17:], "flg0": good[:3] + b"\x00" + good[4:], "empty": b"",
                  "header_only": good[:48], "short": good[:30], "zeros": bytes(64)})
    names = list(cases)
    got = run(exe, "parse", *[cases[n].hex() for n in names])
    for name, g in zip(names, got):
        want = parse_chunk_crcs(cases[name])
        if want is None:
            assert g == {"ok": 0, "K": 0, "crc_at": 0, "crcs": []}, name
        else:
            assert g == {"ok": 1, "K": len(want), "crc_at": 16 + 4 * len(want) + 8, "crcs": want}, name
    ok = [n for n, g in zip(names, got) if g["ok"]]
    assert ok == ["good", "four_chunks", "two_chunks", "bytes_behind_it"], ok
