"""GPU: the bundles (pzg_bundle_kernel.h, bundle_core.h) on PACKED extents -- inputs at every address modulo 4, outputs at every
address modulo 16, guard bytes between them -- over the streams of tests/bundle_cases.py, which are written token by token at the
lanes' edges (the near/far switch of the 512-byte window, self-overlap, the far landing registers, 49-bit steps, blocks ending at
every bit offset, cut tails, capacities inside a token, the size limits).  Against the oracle through the product library; and through
a lab build that stops behind the bundle kernel (build/lab_bundlesonly/libpzg.so), where a stream no lane decoded keeps status 103:
the lanes must decode exactly what the host model's lanes decode (tests/test_model_bundles.py), bit for bit -- the ordinary kernel,
which redoes a handed-back stream from byte 0, cannot hide a lane that is wrong or one that gives up.
Reference semantics: Deflate.hs:79-82, 106-120, 241-251."""
import json
import os
import random
import subprocess
import sys

import pytest

import bundle_cases
from conftest import ROOT
from devbatch import PackedBatch
from test_gpu_bundles import _mixed_pool

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pool(oracle):
    """(stream, capacity) of every bundle case and of test_gpu_bundles' mixed pool, and the oracle's result for each."""
    items = [(c.stream, c.cap) for c in bundle_cases.all_cases()]
    texts, zs = _mixed_pool(random.Random(0xB0))
    items += [(z, len(t)) for t, z in zip(texts, zs)]
    return items, [oracle.decompress(z, cap) for z, cap in items]


def _batch(pool, n, seed, gap):
    """n streams or more: every pool entry, then seeded picks, in seeded order (neighbours differ)."""
    items, expect = pool
    rng = random.Random(seed)
    pick = list(range(len(items))) + [rng.randrange(len(items)) for _ in range(max(0, n - len(items)))]
    rng.shuffle(pick)
    return PackedBatch([items[p][0] for p in pick], [items[p][1] for p in pick], gap=gap), [expect[p] for p in pick]


@pytest.mark.parametrize("gap", [0, 7])
def test_packed_extents_with_bundles_always_on(gpu_ctx, pool, gap):
    """PZG_OPT_BUNDLES = 2, rings 11 and 15, three launches each with the output refilled in between; then PZG_ASYNC | PZG_LPT_ORDER
    (the bundles follow the launch order)."""
    b, expect = _batch(pool, 4096, 0xE0 + gap, gap)
    assert b.n >= 4096
    try:
        gpu_ctx.set_bundles(2)
        for ring in (11, 15):
            for launch in range(3):
                b.run(gpu_ctx, ring)
                b.check(expect, tag=(gap, ring, launch))
        b.run(gpu_ctx, 11, sync=False, lpt=True)
        b.check(expect, tag=(gap, "async lpt"))
    finally:
        gpu_ctx.set_bundles(1)
        gpu_ctx.set_ring_bits(11)


def test_packed_extents_through_the_sharded_call(pool):
    """pzg_decompress_many_sharded on a context of two shards of device 0: one packed batch each."""
    import pure_zlib_amd as P
    halves = [_batch(pool, 4096, 0xE8 + s, 7 * s) for s in range(2)]
    ctx = P.Context(devices=[0, 0])
    try:
        ctx.set_bundles(2)
        for ring in (11, 15):
            ctx.set_ring_bits(ring)
            for b, _ in halves:
                b.reset()
            ctx.decompress_many_sharded([dict(shard=s, n=b.n, **b.ptrs()) for s, (b, _) in enumerate(halves)])
            for s, (b, expect) in enumerate(halves):
                b.check(expect, tag=("shard", s, ring))
    finally:
        ctx.close()


def test_packed_extents_at_the_default_setting(gpu_ctx, pool):
    """PZG_OPT_BUNDLES = 1 takes launches of 32,768 streams or more: one such launch, packed, the option set right before it."""
    b, expect = _batch(pool, 32768, 0xEA, 0)
    assert b.n >= 32768
    gpu_ctx.set_bundles(1)
    b.run(gpu_ctx, 11)
    b.check(expect, tag="default")


CHILD = r'''
import json, os, sys
sys.path.insert(0, os.path.join(os.environ["PZG_ROOT"], "tests")); sys.path.insert(0, os.environ["PZG_ROOT"])
import torch; torch.cuda.init()
import bundle_cases
from devbatch import PackedBatch
import pure_zlib_amd as P
from pure_zlib_amd import _ffi
from oracle import oracle as O
assert _ffi.LIB_PATH.endswith("build/lab_bundlesonly/libpzg.so"), _ffi.LIB_PATH
clean = set(json.load(open(sys.argv[1])))
cases = bundle_cases.all_cases()
assert clean <= set(c.name for c in cases) and len(clean) >= 3900
ctx = P.Context(0)
ctx.set_bundles(2)
for gap in (0, 7):
    import random
    order = list(cases)
    random.Random(0xEC + gap).shuffle(order)
    b = PackedBatch([c.stream for c in order], [c.cap for c in order], gap=gap)
    expect = [O.decompress(c.stream, c.cap) if c.name in clean else None for c in order]
    mine = [k for k, c in enumerate(order) if c.name in clean]
    for ring in (11, 15):
        b.run(ctx, ring)
        status = b.check(expect, only=mine, tag=("lanes alone", gap, ring))  # (and the guard bytes of every extent)
        got = set(c.name for k, c in enumerate(order) if status[k] != 103)
        assert got == clean, ("lanes that gave up", sorted(clean - got)[:10], "lanes that should have", sorted(got - clean)[:10])
ctx.close()
print("lanes alone ok", len(cases), len(clean))
'''


def test_lanes_alone_decode_what_the_model_calls_clean(tmp_path):
    """The lab library ends a launch behind the bundle kernel.  The streams whose status is not 103 must be exactly those the host
    model's lanes decode (a lane's outcome depends on its own stream alone), each the oracle's result bit for bit, on packed extents
    with their guard bytes intact -- in a child process (PZG_LIB), which fails the test with its status."""
    from test_exotic_streams import BUNDLESONLY_FLAGS, lab_library
    from test_model_bundles import expected_clean, model_clean_set
    so = lab_library("bundlesonly", BUNDLESONLY_FLAGS)
    cases = bundle_cases.all_cases()
    clean = model_clean_set(cases)
    assert clean == {c.name for c in cases if expected_clean(c)}
    names = tmp_path / "clean.json"
    names.write_text(json.dumps(sorted(clean)))
    env = dict(os.environ, PZG_LIB=so, PZG_ROOT=ROOT)
    out = subprocess.run([sys.executable, "-c", CHILD, str(names)], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0 and "lanes alone ok" in out.stdout, (out.returncode, out.stdout[-1500:], out.stderr[-3000:])
