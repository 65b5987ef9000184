"""CPU: the three passes of pzg_index_scan_many as a host program (tests/model/model_scan_many.cpp) through the code the kernels call
(pure_zlib_amd/csrc/scan_core.h, ScanMany over Scan).  The contract is per stream: every field is what the one-stream scan
(scancheck.ScanModel, checked by tests/test_model_scan.py against a plain-Python finder and system zlib) gives for that stream alone."""
import os
import random
import re
import subprocess

import numpy as np
import pytest

import indexcheck as X
import scancheck as S
import scanmanycheck as SM

CHUNKS = [256, 1024]
SPANS = [1, 4096]


@pytest.fixture(scope="module")
def one_model():
    return S.ScanModel()


@pytest.fixture(scope="module")
def many_model():
    return SM.ScanManyModel()


@pytest.fixture(scope="module")
def batch():
    sound = X.model_inputs()
    return SM.Batch([(name, d, None) for name, d, _data in sound] + SM.extra_cases(sound, CHUNKS))


@pytest.fixture(scope="module")
def scanned(one_model, many_model, batch):
    """(chunk, span) -> (the references, point_off, the many-stream model's run)"""
    got = {}
    for chunk in CHUNKS:
        for span in SPANS:
            refs = SM.reference(one_model, batch, chunk, span)
            point_off = batch.point_off(refs)
            got[chunk, span] = (refs, point_off, many_model.scan_many(batch, chunk, span, point_off))
    return got


def test_the_batch_holds_the_cases(batch, scanned):
    assert {batch.mis(i) for i in range(batch.n)} == {0, 1, 2, 3}
    at = {name: i for i, name in enumerate(batch.names)}
    refs = scanned[1024, 4096][0]
    assert len(batch.streams[at["empty"]]) == 0 and len(batch.streams[at["short"]]) < 256
    for chunk in CHUNKS:
        assert len(batch.streams[at["three_chunks_%d" % chunk]]) == 3 * chunk
    for name in ("fixed", "stored"):  # no candidates: one segment
        assert all(c is None for c in refs[at[name]]["cand"][1:]) and refs[at[name]]["status"] == 0, name
    assert refs[at["false_candidate"]]["cand"][1] == 8 * 1024 and refs[at["false_candidate"]]["next"][1] & S.NEXT_FAIL
    cut = refs[at["cut"]]
    assert (cut["status"], cut["d0"]) == (S.E_SCAN, S.E_TRUNCATED) and at["before_cut"] + 1 == at["cut"] == at["after_cut"] - 1
    assert refs[at["before_cut"]]["status"] == 0 == refs[at["after_cut"]]["status"]
    two = refs[at["two_slots"]]
    assert two["status"] == 0 and two["npoints"] > 2 == len(two["points"])  # the full count, two stored
    assert all(r["npoints"] < 1024 for r in refs)


def test_every_stream_is_its_own_scan(batch, scanned):
    for (chunk, span), (refs, point_off, got) in scanned.items():
        first = batch.first_chunk(chunk)
        for i, ref in enumerate(refs):
            what = (batch.names[i], chunk, span)
            a, b = int(first[i]), int(first[i + 1])
            assert b - a == len(ref["cand"]), what
            assert [None if c == S.NONE else int(c) for c in got["cand"][a:b]] == ref["cand"], what
            assert got["next"][a:b].tolist() == ref["next"] and got["count"][a:b].tolist() == ref["count"], what
            assert got["endbit"][a:b].tolist() == ref["endbit"], what
            lo, hi = int(point_off[i]), int(point_off[i + 1])
            SM.check_stream(what, ref, got["results"][i], got["points"][lo:hi], got["windows"][lo:hi])


def test_locate(many_model):
    rng = random.Random(5)
    tables = [[0, 1], [0, 7], [0, 0, 3], [0, 2, 2, 2, 5, 5, 6], [0, 1, 2, 3, 4], [0, 0, 0, 1]]
    for _ in range(40):
        n = rng.randint(1, 200)
        tables.append(np.concatenate(([0], np.cumsum([rng.choice((0, 0, 1, 1, 2, 9, 300)) for _ in range(n)]))).tolist())
    asked = 0
    for t in tables:
        for g in (range(t[-1]) if t[-1] < 500 else sorted(rng.sample(range(t[-1]), 300)) + [0, t[-1] - 1]):
            want = max(s for s in range(len(t) - 1) if t[s] <= g)  # the linear search: the last stream that starts at or before g
            assert t[want] <= g < t[want + 1]
            assert many_model.locate(t, g) == want, (t, g)
            asked += 1
    assert asked > 3000


def test_sanitized_program(many_model, batch, scanned, tmp_path):
    """model_scan_many.cpp as a program of its own under AddressSanitizer and UBSan, over the same batch: the same results."""
    exe = str(tmp_path / "model_scan_many_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-DPZSM_MAIN", "-Wno-unknown-pragmas", "-o", exe, many_model.src])
    # one set of slots for all four runs: what the largest of them needs
    rooms = np.max([np.diff(scanned[c, s][1].astype(np.int64)) for c in CHUNKS for s in SPANS], axis=0)
    rooms = [r if batch.rooms[i] is None else batch.rooms[i] for i, r in enumerate(rooms.tolist())]
    point_off = np.concatenate(([0], np.cumsum(rooms))).astype(np.uint32)
    path = str(tmp_path / "batch.bin")
    batch.write(path, point_off)
    out = subprocess.run([exe, path], capture_output=True, text=True)  # (the runtimes are linked in: the environment stays as it is)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = re.findall(r"chunk (\d+) span (\d+) stream (\d+): status (-?\d+) d0 (\d+) d1 (\d+) npoints (\d+) out_len (\d+) in_used (\d+)", out.stdout)
    assert len(lines) == len(CHUNKS) * len(SPANS) * batch.n
    for line in lines:
        chunk, span, i, *vals = [int(x) for x in line]
        ref = scanned[chunk, span][0][i]
        assert tuple(vals) == tuple(ref[f] for f in SM.RESULT_FIELDS), (batch.names[i], chunk, span)
