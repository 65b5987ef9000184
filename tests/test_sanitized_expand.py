"""CPU: the pixel expansion of expand_core.h under AddressSanitizer and UBSan as a stand-alone program (tests/cxx/san_expand.cpp with
tests/model/model_expand.cpp), the way tests/test_sanitized_adam7.py runs the Adam7 gather.  The kernel's READ contract -- "nothing is
read but the aligned dwords that hold bytes of the image's source rows, and its palette entries" -- and its stores -- "one 16-byte
store where a unit lies wholly inside the row, dwords and single bytes at the row's two ends" -- show nowhere on the device; here
every source is a heap block of exactly those dwords, every palette one of exactly its pal_len entries and every destination one of
exactly the image's bytes, so an access one byte outside is a report.  The program compares what it gets with the reference's result
in its case file, and the test asserts that it ran as many cases as were written.  Nothing loaded into Python is sanitized."""
import expandcases as X
import sancases as S


def test_expand_core(tmp_path_factory):
    """The whole case list at its layouts and at shifted ones; the bad palette indices with the waves in either order."""
    d = tmp_path_factory.mktemp("san_expand")
    exe = S.build(str(d / "san_expand"), ["tests/cxx/san_expand.cpp", "tests/model/model_expand.cpp"])
    runs = [(c, i, X.ROW_SLICES, 0) for i, c in enumerate(X.all_cases())]
    runs += [(c, i + 7, 3, 1) for i, c in enumerate(X.all_cases()[::2])]
    runs += [(c, i + 1, X.ROW_SLICES, 1) for i, c in enumerate(X.bad_index_cases())]
    cases = []
    for c, i, slices, descending in runs:
        desc, src, mis, pal, want, loose = X.single(c, i)
        cases.append(["%s layout %d" % (c.name, i), desc.tobytes(), src.tobytes(), mis, pal.tobytes() if pal is not None else b"", slices, descending,
                      c.status, c.d0, c.d1, want.tobytes(), loose.astype("u1").tobytes()])
    n = S.write_cases(str(d / "cases.bin"), cases)
    assert n == 1304 + 652 + 10
    S.run(exe, str(d / "cases.bin"), n)
