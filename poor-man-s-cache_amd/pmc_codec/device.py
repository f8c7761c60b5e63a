"""Device-batch plumbing for the codec: torch supplies HBM buffers and streams only.

A batch is SoA: one uint8 byte buffer plus per-value offsets (int64 = uint64 bits) and
lengths (int32 = uint32 bits), exactly the layout pmc_gzip_*_batch consume.
"""
from dataclasses import dataclass

import numpy as np
import torch

from . import Context, decompress_capacity, gzip_bound


@dataclass
class Batch:
    data: torch.Tensor  # uint8
    off: torch.Tensor   # int64
    len: torch.Tensor   # int32
    n: int
    max_len: int

    def host_items(self, lens=None):
        lens = (lens if lens is not None else self.len).cpu().numpy().astype(np.int64)
        off = self.off.cpu().numpy()
        data = self.data.cpu().numpy()
        return [data[off[i]:off[i] + lens[i]].tobytes() for i in range(self.n)]


def pack(values, device="cuda", align=4):
    n = len(values)
    lens = np.array([len(v) for v in values], dtype=np.int64)
    slots = (lens + align - 1) // align * align
    off = np.zeros(n, dtype=np.int64)
    if n > 1:
        off[1:] = np.cumsum(slots[:-1])
    buf = np.zeros(int(slots.sum()) + 16, dtype=np.uint8)
    for i, v in enumerate(values):
        buf[off[i]:off[i] + lens[i]] = np.frombuffer(v, dtype=np.uint8)
    return Batch(torch.from_numpy(buf).to(device), torch.from_numpy(off).to(device),
                 torch.from_numpy(lens.astype(np.int32)).to(device), n, int(lens.max()) if n else 0)


def slots_for(caps, device="cuda", align=4):
    caps = np.asarray(caps, dtype=np.int64)
    slots = (caps + align - 1) // align * align
    off = np.zeros(len(caps), dtype=np.int64)
    if len(caps) > 1:
        off[1:] = np.cumsum(slots[:-1])
    total = int(slots.sum()) + 16
    return (torch.empty(total, dtype=torch.uint8, device=device), torch.from_numpy(off).to(device),
            torch.from_numpy(caps.astype(np.int32)).to(device))


def stream_handle():
    return torch.cuda.current_stream().cuda_stream


def compress(ctx: Context, b: Batch):
    caps = [gzip_bound(int(x)) for x in b.len.cpu().numpy()]
    dst, doff, dcap = slots_for(caps, b.data.device)
    dlen = torch.zeros(b.n, dtype=torch.int32, device=b.data.device)
    rc = torch.zeros(b.n, dtype=torch.int32, device=b.data.device)
    ctx.compress_device(b.data, b.off, b.len, dst, doff, dcap, dlen, rc, b.max_len, stream_handle())
    return Batch(dst, doff, dlen, b.n, int(max(caps) if caps else 0)), rc


def decompress(ctx: Context, b: Batch, caps=None):
    if caps is None:
        caps = [decompress_capacity(x) for x in b.host_items()]
    dst, doff, dcap = slots_for(caps, b.data.device)
    dlen = torch.zeros(b.n, dtype=torch.int32, device=b.data.device)
    rc = torch.zeros(b.n, dtype=torch.int32, device=b.data.device)
    ctx.decompress_device(b.data, b.off, b.len, dst, doff, dcap, dlen, rc, int(max(caps) if len(caps) else 0),
                          stream_handle())
    return Batch(dst, doff, dlen, b.n, int(max(caps) if len(caps) else 0)), rc


def decompress_range(ctx: Context, b: Batch, offs, lens, align=1):
    """Bytes [offs[i], offs[i] + lens[i]) of member i of the batch, clamped to its value as Redis GETRANGE does
    (Context.decompress_range_device): slots of exactly the clamped lengths, `align` apart."""
    dev = b.data.device
    # the members' ISIZE trailers, gathered on the device: 4 n bytes come back, not the members
    # (a member of under 4 bytes has none: its index is kept inside the buffer and its size taken as 0)
    at = (b.off + b.len.to(torch.int64) - 4).unsqueeze(1) + torch.arange(4, device=dev)
    tr = b.data[at.clamp_(0, max(b.data.numel() - 1, 0))].cpu().numpy().astype(np.int64)
    ok = b.len.cpu().numpy() >= 4
    isz = np.where(ok, tr[:, 0] | tr[:, 1] << 8 | tr[:, 2] << 16 | tr[:, 3] << 24, 0)
    caps = [min(int(ln), int(s) - min(int(o), int(s))) for s, o, ln in zip(isz, offs, lens)]
    dst, doff, dcap = slots_for(caps, dev, align)
    roff = torch.from_numpy(np.asarray(offs, dtype=np.uint32).view(np.int32).copy()).to(dev)
    rlen = torch.from_numpy(np.asarray(lens, dtype=np.uint32).view(np.int32).copy()).to(dev)
    dlen = torch.zeros(b.n, dtype=torch.int32, device=dev)
    rc = torch.zeros(b.n, dtype=torch.int32, device=dev)
    ctx.decompress_range_device(b.data, b.off, b.len, roff, rlen, dst, doff, dcap, dlen, rc, stream_handle())
    return Batch(dst, doff, dlen, b.n, int(max(caps) if len(caps) else 0)), rc
