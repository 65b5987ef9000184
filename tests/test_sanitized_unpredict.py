"""CPU: the Predictor 2 / window stage of unpredict_core.h under AddressSanitizer and UBSan as a stand-alone program
(tests/cxx/san_unpredict.cpp with tests/model/model_unpredict.cpp), the way tests/test_sanitized_expand.py runs the pixel expansion.
The kernel's READ contract -- "nothing is read but the aligned dwords that hold bytes of src_off .. + min(src_len, rows *
src_row_bytes)" -- and its stores -- "aligned dwords or wider inside the window, bytes at its two ends" -- show nowhere on the device;
here every source is a heap block of exactly those dwords and every destination one of exactly the window's bytes, so an access one
byte outside is a report.  The program compares what it gets with the reference's result in its case file, and the test asserts that
it ran as many cases as were written.  Nothing loaded into Python is sanitized."""
import sancases as S
import tiffcases as T


def test_unpredict_core(tmp_path_factory):
    """The whole case list at its layouts, at shifted ones with the waves in the other order, and as one and as very many slices."""
    d = tmp_path_factory.mktemp("san_unpredict")
    exe = S.build(str(d / "san_unpredict"), ["tests/cxx/san_unpredict.cpp", "tests/model/model_unpredict.cpp"])
    runs = [(c, i, 4, 0) for i, c in enumerate(T.all_cases())]
    runs += [(c, i + 5, 3, 1) for i, c in enumerate(T.all_cases()[::2])]
    runs += [(c, i + 2, 1, 0) for i, c in enumerate(T.all_cases()[::5])]
    runs += [(c, i + 3, 4096, 1) for i, c in enumerate(T.all_cases()[::9])]
    cases = []
    for c, i, slices, descending in runs:
        desc, src, mis, want = T.single(c, i)
        cases.append(["%s layout %d" % (c.name, i), desc.tobytes(), src.tobytes(), c.slen, mis, slices, descending, c.status, c.d0, c.d1, want.tobytes()])
    n = S.write_cases(str(d / "cases.bin"), cases)
    assert n == 595 + 298 + 119 + 67
    S.run(exe, str(d / "cases.bin"), n)
