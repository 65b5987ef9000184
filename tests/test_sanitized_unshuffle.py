"""CPU: the byte-plane stage of unshuffle_core.h under AddressSanitizer and UBSan as a stand-alone program
(tests/cxx/san_unshuffle.cpp with tests/model/model_unshuffle.cpp), the way tests/test_sanitized_unpredict.py runs the Predictor 2 stage.
The kernel's READ contract -- "nothing is read but the aligned dwords that hold bytes of src_off .. + min(src_len, rows *
src_row_bytes)", from B planes with a misalignment each -- and its stores -- "aligned dwords or wider inside the window, bytes at its
two ends" -- show nowhere on the device; here every source is a heap block of exactly those dwords and every destination one of
exactly the window's bytes, so an access one byte outside is a report.  The program compares what it gets with the reference's result
in its case file, and the test asserts that it ran as many cases as were written.  Nothing loaded into Python is sanitized."""
import fpcases as F
import sancases as S


def test_unshuffle_core(tmp_path_factory):
    """The whole case list at its layouts, at shifted ones with the waves in the other order, and as one and as very many slices."""
    d = tmp_path_factory.mktemp("san_unshuffle")
    exe = S.build(str(d / "san_unshuffle"), ["tests/cxx/san_unshuffle.cpp", "tests/model/model_unshuffle.cpp"])
    every = F.all_cases()
    runs = [(c, i, 4, 0) for i, c in enumerate(every)]
    runs += [(c, i + 5, 3, 1) for i, c in enumerate(every[::2])]
    runs += [(c, i + 2, 1, 0) for i, c in enumerate(every[::5])]
    runs += [(c, i + 3, 4096, 1) for i, c in enumerate(every[::9])]
    cases = []
    for c, i, slices, descending in runs:
        desc, src, mis, want = F.single(c, i)
        cases.append(["%s layout %d" % (c.name, i), desc.tobytes(), src.tobytes(), c.slen, mis, slices, descending, c.status, c.d0, c.d1, want.tobytes()])
    n = S.write_cases(str(d / "cases.bin"), cases)
    assert n == len(every) + len(every[::2]) + len(every[::5]) + len(every[::9]) and len(every) > 500
    S.run(exe, str(d / "cases.bin"), n)
