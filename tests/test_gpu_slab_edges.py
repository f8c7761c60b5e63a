"""GPU: the edges of the fixed-slot slab (pmc_slab_*): a failed set clears its slot and touches no other, and
a get writes only what its capacity allows.

Expected bytes are the oracle's members and the source values."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 0xA5
SLOTS, MAX_LEN = 64, 4096


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401
    import pmc_codec
    c = pmc_codec.Context(0)
    yield c
    c.close()


def _d2h(ptr, nbytes):
    """Copy nbytes of device memory at ptr into host bytes (HIP runtime through ctypes)."""
    hip = ctypes.CDLL("libamdhip64.so")
    buf = ctypes.create_string_buffer(nbytes)
    assert hip.hipMemcpy(buf, ctypes.c_void_p(ptr), ctypes.c_size_t(nbytes), 2) == 0  # hipMemcpyDeviceToHost
    return buf.raw


def slab_image(slab):
    import torch
    torch.cuda.synchronize()
    lens = np.frombuffer(_d2h(slab.lengths_ptr(), 4 * SLOTS), dtype=np.uint32)
    data = np.frombuffer(_d2h(slab.data_ptr(), slab.stride * SLOTS), dtype=np.uint8).reshape(SLOTS, slab.stride)
    return lens, data


def slab_set(slab, values, slots):
    import torch
    from pmc_codec import device as D
    b = D.pack(values)
    rc = torch.full((len(values),), 7, dtype=torch.int32, device="cuda")
    slab.set(b.data, b.off, b.len, torch.from_numpy(np.asarray(slots, dtype=np.int32)).cuda(), rc, D.stream_handle())
    torch.cuda.synchronize()
    return rc.cpu().numpy()


def slab_get(slab, slots, caps, seed):
    """One get into 0xA5-filled, unaligned slots with 1 to 7 guard bytes between them -> rc, dst_len, the
    destination after the call, the slots' offsets."""
    import torch
    from pmc_codec import device as D
    rng = np.random.default_rng(seed)
    n = len(slots)
    off = np.zeros(n, dtype=np.int64)
    pos = 3
    for i in range(n):
        off[i] = pos
        pos += int(caps[i]) + int(rng.integers(1, 8))
    dst = torch.full((pos + 64,), GUARD, dtype=torch.uint8, device="cuda")
    dlen = torch.full((n,), 12345, dtype=torch.int32, device="cuda")
    rc = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    slab.get(torch.from_numpy(np.asarray(slots, dtype=np.int32)).cuda(), dst, torch.from_numpy(off).cuda(),
             torch.from_numpy(np.asarray(caps, dtype=np.int32)).cuda(), dlen, rc, D.stream_handle())
    torch.cuda.synchronize()
    return rc.cpu().numpy(), dlen.cpu().numpy(), dst.cpu().numpy(), off


def test_slab_failed_set_and_short_get(ctx, golden):
    import pmc_codec
    from oracle import pyoracle as O
    rng = np.random.default_rng(21)
    corpus = golden.corpus
    lens32 = [1, 17, 255, 256, 257, 512, 513, 1024, 4095, 4096] + [int(x) for x in rng.integers(2, 4097, 22)]
    vals = [corpus[o:o + n] for n in lens32 for o in [int(rng.integers(0, len(corpus) - n + 1))]]
    members = [O.compress(v) for v in vals]
    slots = [int(s) for s in rng.permutation(SLOTS)[:32]]
    slab = pmc_codec.Slab(ctx, SLOTS, MAX_LEN)
    assert (slab_set(slab, vals, slots) == 0).all()
    lens0, data0 = slab_image(slab)
    for s, m in zip(slots, members):
        assert lens0[s] == len(m) and data0[s, :len(m)].tobytes() == m, s
    unused = sorted(set(range(SLOTS)) - set(slots))
    assert (lens0[unused] == 0).all()
    # values longer than max_value_len into 8 of the slots: E_ARG, the slots become empty, nothing else changes
    hit = slots[3:27:3]
    assert len(hit) == 8
    long_vals = [corpus[100 * k:100 * k + n] for k, n in enumerate([4097, 5000] + [int(x) for x in rng.integers(4097, 5001, 6)])]
    assert (slab_set(slab, long_vals, hit) == pmc_codec.E_ARG).all()
    lens1, data1 = slab_image(slab)
    assert (lens1[hit] == 0).all()
    kept = [s for s in slots if s not in hit]
    assert len(kept) == 24 and (lens1[kept] == lens0[kept]).all() and (lens1[unused] == 0).all()
    assert (data1[kept + unused] == data0[kept + unused]).all()
    # a get of the emptied slots and of never-written ones: INVALID_INPUT, no byte written
    rc, dlen, out, off = slab_get(slab, hit + unused[:4], [64] * 12, 1)
    assert (rc == pmc_codec.INVALID_INPUT).all() and (out == GUARD).all(), (rc, dlen)
    # capacities cycling over raw_len, raw_len - 1, 0 and raw_len + 5
    for turn in range(4):
        raw = [len(vals[slots.index(s)]) for s in kept]
        caps = [(r, r - 1, 0, r + 5)[(i + turn) % 4] for i, r in enumerate(raw)]
        rc, dlen, out, off = slab_get(slab, kept, caps, 2 + turn)
        untouched = np.ones(len(out), dtype=bool)
        bad = []
        for i, s in enumerate(kept):
            o, v = int(off[i]), vals[slots.index(s)]
            untouched[o:o + min(caps[i], raw[i])] = False
            if caps[i] < raw[i]:
                if rc[i] != pmc_codec.E_CAPACITY:
                    bad.append((i, s, caps[i], raw[i], int(rc[i]), int(dlen[i])))
            elif rc[i] != 0 or dlen[i] != raw[i] or out[o:o + raw[i]].tobytes() != v:
                bad.append((i, s, caps[i], raw[i], int(rc[i]), int(dlen[i])))
        assert not bad, (turn, bad)
        changed = np.flatnonzero(untouched & (out != GUARD))
        assert len(changed) == 0, (turn, len(changed), int(changed[0]), [int(o) for o in off])
    slab.close()
