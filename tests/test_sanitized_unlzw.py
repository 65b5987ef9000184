"""CPU: the LZW decoder of unlzw_core.h under AddressSanitizer and UBSan as a stand-alone program (tests/cxx/san_unlzw.cpp with
tests/model/model_unlzw.cpp), the way tests/test_sanitized_unshuffle.py runs the byte-plane stage.  The kernel's READ contract --
"nothing is read but the aligned dwords that hold bytes of the stream" -- and its WRITE contract -- "nothing is ever written past
out_cap" -- show nowhere on the device; here every source is a heap block of exactly those dwords and every output one of exactly
out_cap bytes, so an access one byte outside is a report.  The output is also what the decoder copies its strings FROM: a read of a
byte it has not delivered yet would pass the sanitizer and fail the comparison with the reference's bytes in the case file.  The test
asserts that the program ran as many cases as were written.  Nothing loaded into Python is sanitized."""
import lzwcases as L
import sancases as S


def test_unlzw_core(tmp_path_factory):
    """The whole case list at its layouts and at shifted ones."""
    d = tmp_path_factory.mktemp("san_unlzw")
    exe = S.build(str(d / "san_unlzw"), ["tests/cxx/san_unlzw.cpp", "tests/model/model_unlzw.cpp"])
    every = L.all_cases()
    runs = [(c, i) for i, c in enumerate(every)] + [(c, i + 1) for i, c in enumerate(every[::2])] + [(c, i + 2) for i, c in enumerate(every[::3])]
    cases = []
    for c, i in runs:
        mis, out_off, _ = L.layout(c, i)
        cases.append(["%s layout %d" % (c.name, i), c.stream, mis, out_off, c.cap, c.early_change, c.status, len(c.out), c.d0, c.d1,
                      L.expected_dst(c, i).tobytes()])
    n = S.write_cases(str(d / "cases.bin"), cases)
    assert n == len(every) + len(every[::2]) + len(every[::3]) and len(every) > 200
    S.run(exe, str(d / "cases.bin"), n)
