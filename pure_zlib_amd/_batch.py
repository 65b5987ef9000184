"""What the batch readers share (private): the packing rule of every batch buffer, the one loader of a source, and the owner of the
buffers of a decode-then-stages chain on the device.  Plain numpy and Python; torch is imported where a device is needed."""
import os
from typing import Dict, Optional, Sequence, Tuple

import numpy as np


def pack(lengths, slack: int = 0) -> Tuple[np.ndarray, int]:
    """(offsets u64[n], total): extents of lengths[i] + slack bytes, one behind the other in a buffer of `total` bytes.  It guarantees
    that every extent starts on a multiple of 16, the alignment of the kernels' wide stores, and that a launch may read 16 bytes past
    the last extent.  slack=4: the guard dword of a decode destination (a stream that decodes to MORE than its capacity claims no
    neighbour's dword)."""
    extents = (np.asarray(lengths, dtype=np.uint64) + np.uint64(slack + 15)) & ~np.uint64(15)
    offsets = np.zeros(len(extents), dtype=np.uint64)
    offsets[1:] = np.cumsum(extents)[:-1]
    return offsets, int(extents.sum()) + 16


def load(src) -> Tuple[Optional[str], bytes]:
    if isinstance(src, (bytes, bytearray, memoryview)):
        return None, bytes(src)
    with open(src, "rb") as f:
        return os.fspath(src), f.read()


class DeviceChain:
    """Owns the buffers of one decode launch and of the stage launches behind it on the context's stream, as torch tensors: the
    streams = [(buffer, start, length)] packed into a pinned arena and uploaded, the decode destination with the exact capacities
    dec_cap (pack(dec_cap, slack=4)), the out_len array, and a zeroed status/detail block per launch ("decode" is the chain's own).
    codecs = [(codec, count)]: contiguous runs of streams, each run decoded by its codec's launch -- "deflate": pzg_decompress_many,
    "lzw": pzg_unlzw_many (TIFF's early change) -- into the same destination, out_len array and "decode" block; an empty run issues
    nothing.  None: every stream is a zlib stream.
    The caller uploads and allocates everything BEFORE decode(), which waits for torch's copies and fills, issues its stage launches
    itself with sync=False, and finish() is the one sync.  A context manager: the arena is closed on every path.  Device pointers
    are integers (data_ptr()); the tensors behind them live as long as the chain."""

    def __init__(self, ctx, streams: Sequence[Tuple[bytes, int, int]], dec_cap, codecs: Optional[Sequence[Tuple[str, int]]] = None):
        import torch
        from .zlib import PinnedArena
        self._torch, self.ctx, self.n = torch, ctx, len(streams)
        self._codecs = [("deflate", self.n)] if codecs is None else [(c, int(k)) for c, k in codecs]
        if sum(k for _c, k in self._codecs) != self.n or any(c not in ("deflate", "lzw") for c, _k in self._codecs):
            raise ValueError("codecs: runs of 'deflate' or 'lzw' streams that add up to the streams")
        self._dev = torch.device("cuda", ctx.device)
        self._keep, self._blocks = [], {}
        self.dec_cap = np.ascontiguousarray(dec_cap, dtype=np.uint64)
        in_len = np.array([length for _b, _s, length in streams], dtype=np.uint64)
        in_off, tot_in = pack(in_len)
        self.dec_off, tot_dec = pack(self.dec_cap, slack=4)
        self._arena = PinnedArena(tot_in)
        try:
            for o, (buf, start, length) in zip(in_off.tolist(), streams):
                self._arena.a[o:o + length] = np.frombuffer(buf, dtype=np.uint8, count=length, offset=start)
            self._in = [self.upload(a) for a in (self._arena.a[:tot_in], in_off, in_len)]
            self.dec_off_ptr, self._dec_cap_ptr = self.upload(self.dec_off), self.upload(self.dec_cap)
            self.dec_ptr = self.scratch(tot_dec).data_ptr()
            self._d_out_len = torch.zeros(8 * self.n, dtype=torch.uint8, device=self._dev)
            self.out_len_ptr = self._d_out_len.data_ptr()
            self._decode = self.results("decode", self.n)
        except BaseException:
            self._arena.close()
            raise

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self._arena.close()

    def upload(self, array) -> int:
        """The array's bytes on the device; returns their address."""
        t = self._torch.from_numpy(np.ascontiguousarray(array).view(np.uint8)).to(self._dev)
        self._keep.append(t)
        return t.data_ptr()

    def scratch(self, nbytes: int):
        """An uninitialised uint8 tensor on the device."""
        t = self._torch.empty(nbytes, dtype=self._torch.uint8, device=self._dev)
        self._keep.append(t)
        return t

    def results(self, name: str, n: int) -> Tuple[int, int]:
        """(status, detail) addresses of a launch's own n zeroed status words and n detail pairs, one tensor, downloaded by finish()."""
        t = self._torch.zeros(12 * n, dtype=self._torch.uint8, device=self._dev)
        self._blocks[name] = (t, n)
        return t.data_ptr(), t.data_ptr() + 4 * n

    def decode(self) -> None:
        """Enqueues the decode of every stream, behind everything torch was asked to copy and fill so far."""
        self._torch.cuda.synchronize(self._dev)
        first = 0
        for codec, count in self._codecs:
            if count:
                args = (self._in[0], self._in[1] + 8 * first, self._in[2] + 8 * first, self.dec_ptr, self.dec_off_ptr + 8 * first,
                        self._dec_cap_ptr + 8 * first, self.out_len_ptr + 8 * first, self._decode[0] + 4 * first, self._decode[1] + 8 * first)
                if codec == "lzw":
                    self.ctx.unlzw_many_device(*args, count, early_change=True, sync=False)
                else:
                    self.ctx.decompress_many_device(*args, 0, 0, count, sync=False)
            first += count

    def finish(self) -> Dict[str, Tuple[np.ndarray, np.ndarray]]:
        """The one sync.  {launch: (status i32[n], detail u32[n, 2])} of every result block."""
        self.ctx.sync()
        out = {}
        for name, (t, n) in self._blocks.items():
            host = t.cpu().numpy()
            out[name] = (host[:4 * n].view(np.int32), host[4 * n:].view(np.uint32).reshape(n, 2))
        return out

    def out_len(self) -> np.ndarray:
        """u64[n]: what every stream decoded to (after finish())."""
        return self._d_out_len.cpu().numpy().view(np.uint64)
