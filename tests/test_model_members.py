"""CPU: the member finder and the layout of pzg_gzip_find_members / pzg_gzip_layout (pure_zlib_amd/csrc/member_core.h) as a host
program (tests/model/model_members.cpp) against their specification restated in plain Python and numpy (tests/memberscheck.py).
The GPU suite (tests/test_gpu_members.py) then asks the device for exactly what the model gives."""
import numpy as np
import pytest

import memberscheck as M


@pytest.fixture(scope="module")
def model():
    return M.MembersModel()


def all_files():
    return [(name, z) for name, z, _d, _f in M.sound_files()] + M.finder_files()


@pytest.mark.parametrize("chunk", M.CHUNKS)
def test_finder_equals_the_plain_python_finder(model, chunk):
    for name, z in all_files():
        want = M.find(z)
        for mis in ((0, 1, 2, 3) if chunk == 64 else (chunk % 3,)):
            n, starts, bsize = model.find(z, chunk, mis=mis)
            assert (n, starts, bsize) == (len(want[0]), want[0], want[1]), (name, chunk, mis)


def test_what_the_files_are_meant_to_hold():
    """The builders build what their names say: the cases of the finder are really there."""
    files = dict(M.finder_files())
    starts, _ = M.find(files["edges"])
    assert starts == [0] + [4096 * k - k for k in range(1, 11)] + [len(files["edges"]) - 10]
    assert M.find(files["nine"])[0] == [0] and M.find(files["one"])[0] == [0] and M.find(files["empty"])[0] == [0]
    for name in ("xlen-past-input", "bc-past-xlen"):
        starts, bsize = M.find(files[name])
        assert len(starts) == 2 and bsize == [0, 0], name
    sound = {name: (z, d, f) for name, z, d, f in M.sound_files()}
    assert [sound[k][2] for k in ("one", "two", "bgzf", "bc-behind-another", "empty-members")] == [0] * 5
    assert sound["bare-header-inside"][2] == 1 and sound["member-inside"][2] == 1  # one drop repairs each
    starts, bsize = M.find(sound["bgzf"][0])
    assert len(starts) == 3 and [s + b for s, b in zip(starts, bsize)] == starts[1:] + [len(sound["bgzf"][0])]
    starts, bsize = M.find(sound["bc-behind-another"][0])
    assert len(starts) == 2 and starts[0] + bsize[0] == starts[1] and starts[1] + bsize[1] == len(sound["bc-behind-another"][0])
    assert len(M.find(sound["empty-members"][0])[0]) == 9 and len(sound["empty-members"][0]) == 9 * 20
    assert len(M.find(sound["thirty-seven"][0])[0]) - sound["thirty-seven"][2] == 37
    # pruning by the stated sizes keeps a BGZF file's members and nothing else
    z = sound["bgzf"][0]
    inside = z[:100] + M.BARE_HEADER + z[110:]
    assert len(M.find(inside)[0]) == 4 and M.prune(*M.find(inside)) == M.find(z)[0]


@pytest.mark.parametrize("chunk", M.CHUNKS)
def test_more_members_than_room(model, chunk):
    name, z, _d, _f = [f for f in M.sound_files() if f[0] == "thirty-seven"][0]
    want = M.find(z)
    for room in (0, 1, 5, len(want[0]) - 1):
        n, starts, bsize = model.find(z, chunk, max_members=room)  # (the guard slot behind the room is checked in there)
        assert n == len(want[0]) and starts == want[0][:room] and bsize == want[1][:room], (chunk, room)


def test_layout_equals_numpy(model):
    for name, z in all_files():
        cands = M.find(z)[0]
        for starts in (cands, cands[:1], cands[::2]):
            for base, mis in ((0, 0), (12345678901, 3)):
                want = M.layout(z, starts, base)
                got = model.layout(z, starts, base, mis)
                for w, g, what in zip(want[:4], got[:4], ("in_off", "in_len", "out_off", "out_cap")):
                    assert np.array_equal(w, g), (name, what, len(starts), base)
                assert got[4] == want[4], (name, len(starts))


def test_layout_of_many_members(model):
    """More members than one tile of the prefix sums holds, and a sum past 2^32."""
    one = M.gz(b"") + M.wrap(M.stored(b"x" * 3), b"x" * 3)
    big = M.BARE_HEADER + M.stored(b"") + bytes(4200000) + (0xfffffff0).to_bytes(4, "little")  # claims 4 GiB, and is long enough for it
    z = one * 5000 + big + big
    starts = M.find(z)[0]
    assert len(starts) == 10002
    want, got = M.layout(z, starts, 7), model.layout(z, starts, 7)
    for w, g in zip(want[:4], got[:4]):
        assert np.array_equal(w, g)
    assert got[4] == want[4] == 5000 * 3 + 2 * 0xfffffff0
    n, got_starts, _b = model.find(z, 4096)
    assert n == 10002 and got_starts == starts
