"""GPU: the host-pointer form of the three image stages -- pzg_unfilter_many, pzg_adam7_many, pzg_expand_many -- pinned where the launcher
does arithmetic of its own: the spans it stages, their places modulo 16, the metadata block, the copy-back of the delivered rows.
Batches of 3 to 6 tiny images from pngcases, adam7cases and expandcases, against their references and the device-pointer form.
src and dst are views that start 1 and 15 bytes behind a 16-byte boundary of larger buffers, the extents another GUARD bytes into dst:
both spans are staged off the boundary, at different places, and every byte around them is checked to be what it was."""
import dataclasses

import numpy as np
import pytest

import adam7cases as A
import expandcases as X
import pngcases as PC
import test_gpu_adam7
import test_gpu_expand
import test_gpu_png

pytestmark = pytest.mark.gpu

FILL = PC.FILL
assert FILL == A.FILL == X.FILL
GUARD = 3     # bytes of dst in front of the first extent
FAR = 1 << 40  # an offset no span may reach to


def view_in(data, lead):
    """(a larger buffer of FILL, where the view starts in it, a view of len(data) bytes that starts `lead` bytes behind a 16-byte boundary
    and holds data)"""
    big = np.full(len(data) + 64, FILL, np.uint8)
    at = (-big.ctypes.data) % 16 + lead
    view = big[at:at + len(data)]
    view[:] = data
    assert view.ctypes.data % 16 == lead
    return big, at, view


def moved(b, stage):
    """The batch with every destination extent GUARD bytes further into dst."""
    want = np.concatenate([np.full(GUARD, FILL, np.uint8), b.dst_want])
    if stage == "expand":
        desc = b.desc.copy()
        desc["dst_off"] += GUARD
        return dataclasses.replace(b, desc=desc, dst_want=want, loose=np.concatenate([np.zeros(GUARD, bool), b.loose]), dst_off=b.dst_off + np.uint64(GUARD))
    return dataclasses.replace(b, dst_want=want, dst_off=b.dst_off + np.uint64(GUARD))


def host_call(ctx, stage, b, src, dst, with_detail=True):
    """A raw call of the stage's entry point on host pointers: (rc, status, detail or None)."""
    from pure_zlib_amd import _ffi
    L, h, n = _ffi.lib(), ctx.handle, len(b.cases)
    status = np.full(n, -1, np.int32)
    detail = np.full((n, 2), 0xABABABAB, np.uint32) if with_detail else None
    d = detail.ctypes.data if with_detail else None
    p = lambda a: a.ctypes.data  # noqa: E731
    if stage == "unfilter":
        rc = L.pzg_unfilter_many(h, p(src), p(b.src_off), p(b.src_len), p(dst), p(b.dst_off), p(b.stride), p(b.row_bytes), p(b.height), p(b.bpp),
                                 p(status), d, n, 0)
    elif stage == "adam7":
        rc = L.pzg_adam7_many(h, p(src), p(b.src_off), p(dst), p(b.dst_off), p(b.stride), p(b.width), p(b.height), p(b.bits), p(status), d, n, 0)
    else:
        rc = L.pzg_expand_many(h, p(src), p(dst), p(b.palette), p(b.desc), p(status), d, n, 0)
    return rc, status, detail


DEVICE = {"unfilter": test_gpu_png.run_device, "adam7": test_gpu_adam7.run_device, "expand": test_gpu_expand.run_device}
DIFFERENCE = {"unfilter": PC.first_difference, "adam7": A.first_difference, "expand": X.first_difference}


def spans(stage, b):
    """(s_lo, d_lo): where the spans of the images that have pixels start."""
    if stage == "expand":
        live = [i for i, c in enumerate(b.cases) if c.width and c.height]
        return min(int(b.desc["src_off"][i]) for i in live), min(int(b.desc["dst_off"][i]) for i in live)
    if stage == "adam7":
        live = [i for i, c in enumerate(b.cases) if c.width and c.height]
        return min(int(b.src_off[i]) for i in live), min(int(b.dst_off[i]) for i in live)
    live = [i for i, c in enumerate(b.cases) if c.row_bytes and c.height]
    return min(int(b.src_off[i]) for i in live if b.src_len[i]), min(int(b.dst_off[i]) for i in live)


def run_unaligned(ctx, stage, b, with_detail=True, skews=True):
    """The host-pointer form on the unaligned views; checks the return value, the statuses and details against the cases', every byte of
    dst against the reference and every byte around src's and dst's views against what it was.  Returns (dst, status, detail)."""
    from pure_zlib_amd import _ffi
    big_s, at_s, src = view_in(b.src, 1)
    big_d, at_d, dst = view_in(np.full(len(b.dst_want), FILL, np.uint8), 15)
    before = big_s.copy()
    if skews:
        s_lo, d_lo = spans(stage, b)
        s_skew, d_skew = (src.ctypes.data + s_lo) % 16, (dst.ctypes.data + d_lo) % 16
        assert s_skew and d_skew and s_skew != d_skew, (s_skew, d_skew)
    rc, status, detail = host_call(ctx, stage, b, src, dst, with_detail)
    assert rc == _ffi.RC_OK, ctx._L.pzg_last_error(ctx.handle)
    for i, c in enumerate(b.cases):
        assert int(status[i]) == c.status, c.name
        if with_detail:
            assert (int(detail[i, 0]), int(detail[i, 1])) == (c.d0, c.d1), c.name
    assert DIFFERENCE[stage](dst, b) is None, DIFFERENCE[stage](dst, b)
    if stage == "expand":  # the host form delivers nothing of a failed image: its rows are as they were, too
        assert (dst[b.loose] == FILL).all()
    assert (big_d[:at_d] == FILL).all() and (big_d[at_d + len(dst):] == FILL).all()
    assert np.array_equal(big_s, before)
    return dst, status, detail


def against_device(ctx, stage, b, host):
    device = DEVICE[stage](ctx, b)
    keep = ~b.loose if stage == "expand" else slice(None)
    assert np.array_equal(host[0][keep], device[0][keep])
    assert np.array_equal(host[1], device[1]) and np.array_equal(host[2], device[2])


# ---- the batches: 3 to 6 tiny images each ------------------------------------------------------------------------------------------------
def _unfilter_cases():
    pick = [c for c in PC.shape_cases() if c.height <= 2 and c.row_bytes <= 65]
    return [pick[3], pick[40], PC.empty_case(), pick[21], pick[58]]


def _adam7_cases():
    s = A.small_cases()
    return [s[40], s[200], A.empty_cases()[0], s[411], s[728]]


def _expand_cases():
    pick = [c for c in X.shape_cases() if c.width <= 17 and c.height <= 2]
    pal = next(c for c in pick if c.ct == 3 and c.depth == 4)
    return [pick[5], pal, X.empty_cases()[0], pick[131], next(c for c in pick if c.depth == 16 and c.fmt == X.RGB8)]


BATCHES = {"unfilter": lambda cases: PC.batch(cases, stride_extra=5), "adam7": lambda cases: A.batch(cases, stride_extra=5), "expand": lambda cases: X.batch(cases, 2)}
CASES = {"unfilter": _unfilter_cases, "adam7": _adam7_cases, "expand": _expand_cases}
EMPTY = {"unfilter": lambda: [PC.empty_case(), PC.Case("no bytes", 1, 0, 5, b"", 0, 0, 0, []), PC.empty_case()],
         "adam7": lambda: A.empty_cases() + A.empty_cases()[:1], "expand": X.empty_cases}
STAGES = ("unfilter", "adam7", "expand")


def _batch(stage, cases):
    assert 3 <= len(cases) <= 6
    return moved(BATCHES[stage](cases), stage)


@pytest.mark.parametrize("stage", STAGES)
def test_unaligned_base_pointers_and_an_empty_image_in_the_middle(gpu_ctx, stage):
    b = _batch(stage, CASES[stage]())
    if stage != "expand":
        assert (b.stride > (b.row_bytes if stage == "unfilter" else [c.row_bytes for c in b.cases])).all()  # padding between the rows
    else:
        assert any(int(d["dst_stride"]) > c.orb for d, c in zip(b.desc, b.cases) if c.orb)
    host = run_unaligned(gpu_ctx, stage, b)
    against_device(gpu_ctx, stage, b, host)
    assert gpu_ctx.last_kernel_ms() > 0.0


@pytest.mark.parametrize("stage", STAGES)
def test_a_batch_of_only_empty_images(gpu_ctx, stage):
    b = _batch(stage, EMPTY[stage]())
    _dst, status, detail = run_unaligned(gpu_ctx, stage, b, skews=False)  # (it checks dst: FILL everywhere)
    assert (status == 0).all() and (detail == 0).all()
    _dst, status, _none = run_unaligned(gpu_ctx, stage, b, with_detail=False, skews=False)
    assert (status == 0).all()


@pytest.mark.parametrize("stage", STAGES)
def test_without_a_detail_array(gpu_ctx, stage):
    cases = CASES[stage]()
    if stage == "unfilter":
        cases[1] = next(c for c in PC.error_cases() if c.name.startswith("filter-byte 5 row 64 bpp1 rb1 h65"))
    if stage == "expand":
        cases[3] = X.bad_index_cases()[7]
    b = _batch(stage, cases)
    with_detail = run_unaligned(gpu_ctx, stage, b)
    without = run_unaligned(gpu_ctx, stage, b, with_detail=False)
    assert without[2] is None and np.array_equal(with_detail[1], without[1]) and np.array_equal(with_detail[0], without[0])


def test_unfilter_delivers_the_rows_in_front_of_a_failure_and_a_wild_offset_without_bytes_widens_nothing(gpu_ctx):
    good = _unfilter_cases()
    part = next(c for c in PC.error_cases() if c.name.startswith("filter-byte 255 row 64 bpp1 rb1 h65"))
    cut = next(c for c in PC.error_cases() if c.name.startswith("cut at 63+1 bpp1 rb1 h65"))
    none = next(c for c in PC.error_cases() if c.name.startswith("cut at 0+0 bpp1 rb1 h65"))
    assert (part.status, part.d0, len(part.rows)) == (PC.E_FILTER, 64, 64) and len(cut.rows) == 63
    assert (none.status, none.d0, none.d1, len(none.stream), none.rows) == (PC.E_TRUNCATED, 0, 0, 0, [])
    b = _batch("unfilter", [good[0], part, good[1], none, cut, good[3]])
    b.src_off[3] = FAR  # no byte of it is read: it must not count for the span
    host = run_unaligned(gpu_ctx, "unfilter", b)
    # (the rows behind the failures: run_unaligned holds them to FILL with everything else that is not delivered)
    want = b.dst_want
    for i, rows in ((1, 64), (4, 63), (3, 0)):
        lo, stride = int(b.dst_off[i]), int(b.stride[i])
        assert (want[lo + rows * stride:lo + 65 * stride] == FILL).all() and (host[0][lo + rows * stride:lo + 65 * stride] == FILL).all()
        assert rows == 0 or (want[lo:lo + rows * stride:stride] != FILL).any()
    against_device(gpu_ctx, "unfilter", dataclasses.replace(b, src_off=np.where(b.src_len == 0, np.uint64(0), b.src_off)), host)


def test_expand_leaves_an_image_with_a_bad_palette_index_untouched(gpu_ctx):
    good = _expand_cases()
    bad = [X.bad_index_cases()[7], X.bad_index_cases()[5]]  # in the last row's last pixel but one; in row 1 of 2, mid-row
    assert all(c.status == X.E_PALETTE for c in bad)
    b = _batch("expand", [good[0], bad[0], good[1], bad[1], good[4]])
    assert b.loose.any()
    host = run_unaligned(gpu_ctx, "expand", b)  # (it holds the bytes of b.loose to FILL)
    against_device(gpu_ctx, "expand", b, host)


def test_adam7_delivers_all_rows_of_every_image_or_refuses_the_call(gpu_ctx):
    """The deinterlacing has one failure, illegal geometry, and the host-pointer form refuses it with its return value
    (test_gpu_adam7.test_bad_arguments): what is left is that every image with pixels arrives whole beside images without."""
    s = A.small_cases()
    b = _batch("adam7", [A.empty_cases()[1], s[80], A.edge_cases()[0], A.empty_cases()[0], s[8], s[700]])
    host = run_unaligned(gpu_ctx, "adam7", b)
    assert (host[1] == 0).all() and (host[2] == 0).all()
    against_device(gpu_ctx, "adam7", b, host)
