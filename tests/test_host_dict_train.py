"""CPU: dictionary training in plain C++ (tests/host/dict_train_check.cpp, written from the header's text) -- a
stand-alone program built with the address and undefined-behaviour sanitizers -- gives the model's bytes
(tests/dict_train_model.py) on the whole corpus of tests/dict_train_values.py, and csrc/pmc_plan.hpp plan_dict_train
keeps its bounds over a grid of sample counts, dictionary sizes and device sizes."""
import json
import os
import subprocess
import tempfile

import pytest

from dict_train_model import MAX_SAMPLES, train, valid
from dict_train_values import all_cases, case_file

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def exe():
    d = tempfile.mkdtemp(prefix="pmc_dict_train_")
    out = os.path.join(d, "dict_train_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", out, os.path.join(HERE, "host", "dict_train_check.cpp")])
    return out


def test_the_cpp_check_gives_the_models_bytes_on_every_case(exe, golden):
    cases = all_cases(golden.corpus)
    path = os.path.join(os.path.dirname(exe), "cases.bin")
    with open(path, "wb") as f:
        f.write(case_file(cases))
    out = subprocess.run([exe, "train", path], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    got = out.stdout.split()
    assert len(got) == len(cases)
    for c, g in zip(cases, got):
        assert bytes.fromhex("" if g == "-" else g) == train(c.samples, c.D), c.name


def test_plan_dict_train_keeps_its_bounds(exe):
    grid = [(n, D, cus) for n in (1, 2, 63, 64, 65, 127, 128, 129, 2048, 4097, 65536, MAX_SAMPLES - 1, MAX_SAMPLES)
            for D in (64, 128, 2048, 8128, 8192) for cus in (0, 1, 8, 256, 304)]
    bad = [(0, 64, 256), (MAX_SAMPLES + 1, 64, 256), (1, 0, 256), (1, 32, 256), (1, 100, 256), (1, 8256, 256)]
    out = subprocess.run([exe, "plan"] + [str(x) for t in grid + bad for x in t], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    got = [json.loads(ln) for ln in out.stdout.splitlines()]
    assert len(got) == len(grid) + len(bad)
    for (n, D, cus), g in zip(grid + bad, got):
        assert g["ok"] == int(valid(n, D)), (n, D, cus)
        if not g["ok"]:
            continue
        E, resident = D // 64, 16 * max(cus, 1)
        assert g == {"ok": 1, "fine": 1, "E": E, "count_blocks": min(n, resident),
                     "max_blocks": min(-(-n // E), resident), "bytes": g["bytes"]}, (n, D, cus)
        assert (4 << 20) + 256 + 16 * g["max_blocks"] + D <= g["bytes"] < (4 << 20) + 512 + 16 * resident + 8192 + 256
