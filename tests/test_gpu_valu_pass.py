"""GPU: the streams of tests/valu_pass_cases.py (the edges of strip_step_b and seq_group that the VALU pass touches) on the device,
256 streams per launch in PACKED arenas -- extents back to back, inputs at every address modulo 4, outputs at every address modulo
16, 0xCD around and between them --, two launches in a row over the same arenas; and level-6 text of one, two and three spans per
stream with binary records (the inject path of strip_step_b) beside it.  the edge streams once more as gzip members.  status, out_len, in_used, checksum and every byte against
the oracle, nothing written outside the extents."""
import zlib

import pytest

import corpus
import valu_pass_cases as V
from devbatch import PackedBatch

pytestmark = pytest.mark.gpu
N = 256


def _spread(items, n):
    """n streams out of the distinct ones, round robin -- one byte more of capacity for every second copy, so that the extents'
    addresses go through every residue"""
    streams, caps, idx = [], [], []
    for i in range(n):
        k = i % len(items)
        z, d = items[k]
        streams.append(z)
        caps.append(len(d) + (i // len(items)) % 2)
        idx.append(k)
    return streams, caps, idx


@pytest.fixture(scope="module")
def edge_cases(oracle):
    out = {}
    for rb in (11, 15):
        items = [(V.zlib_wrap(d, raw), d) for _, d, raw in V.cases(rb)]
        streams, caps, idx = _spread(items, N)
        memo = {}
        expect = []
        for z, cap, k in zip(streams, caps, idx):
            if (k, cap) not in memo:
                memo[(k, cap)] = oracle.decompress(z, cap)
                assert memo[(k, cap)][0].status == 0 and memo[(k, cap)][1] == items[k][1]
            expect.append(memo[(k, cap)])
        out[rb] = (streams, caps, expect)
    return out


@pytest.fixture(scope="module")
def edge_cases_gzip(oracle):
    """the ring-11 cases as gzip members: the gzip instance is a kernel of its own with the same reader"""
    items = [(V.gzip_wrap(d, raw), d) for _, d, raw in V.cases(11)]
    streams, caps, idx = _spread(items, N)
    memo, expect = {}, []
    for z, cap, k in zip(streams, caps, idx):
        if (k, cap) not in memo:
            memo[(k, cap)] = oracle.gzip_decompress(z, cap)
            assert memo[(k, cap)][0].status == 0 and memo[(k, cap)][1] == items[k][1]
        expect.append(memo[(k, cap)])
    return streams, caps, expect


@pytest.fixture(scope="module")
def text_cases(oracle):
    # (odd lengths: the packed extents then start at every address)
    datas = [corpus.zipf_text(n + 7 * i + 1, 50 + i) for n in (2048, 8192, 40960) for i in range(64)]
    datas += [corpus.binary_records(16384 + 5 * i + 3, 70 + i) for i in range(64)]
    streams = [zlib.compress(d, 6) for d in datas]
    expect = [oracle.decompress(z, len(d)) for z, d in zip(streams, datas)]
    assert all(r.status == 0 and o == d for (r, o), d in zip(expect, datas))
    return streams, [len(d) for d in datas], expect


@pytest.mark.parametrize("rb", [11, 15])
def test_edge_streams_packed_two_launches(gpu_ctx, edge_cases, rb):
    streams, caps, expect = edge_cases[rb]
    b = PackedBatch(streams, caps, gap=0)
    try:
        for launch in range(2):
            b.run(gpu_ctx, rb)
            status = b.check(expect, tag=("edges", rb, launch))
            assert (status == 0).all()
    finally:
        gpu_ctx.set_ring_bits(11)


def test_edge_streams_packed_gzip(gpu_ctx, edge_cases_gzip):
    """... and one launch of them through the gzip instance (the checksum field holds the CRC-32, as the oracle's does)"""
    streams, caps, expect = edge_cases_gzip
    b = PackedBatch(streams, caps, gap=0)
    b.reset()
    gpu_ctx.set_ring_bits(11)
    gpu_ctx.decompress_many_device(n=b.n, gzip=True, **b.ptrs())
    status = b.check(expect, tag=("edges", "gzip"))
    assert (status == 0).all()


@pytest.mark.parametrize("rb", [11, 15])
def test_text_spans_and_binary_records_packed(gpu_ctx, text_cases, rb):
    streams, caps, expect = text_cases
    b = PackedBatch(streams, caps, gap=0)
    try:
        for launch in range(2):
            b.run(gpu_ctx, rb)
            status = b.check(expect, tag=("text", rb, launch))
            assert (status == 0).all()
    finally:
        gpu_ctx.set_ring_bits(11)
