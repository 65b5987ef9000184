"""CPU: the Adam7 gather of adam7_core.h under AddressSanitizer and UBSan as a stand-alone program (tests/cxx/san_adam7.cpp with
tests/model/model_adam7.cpp), the way tests/test_sanitized_cores.py runs the other cores.  The kernel's READ contract -- "nothing is
read but the aligned dwords that hold bytes of the image's source extent" -- and its stores -- "a dword where it lies wholly inside
the row, single bytes at the row's two ends" -- show nowhere on the device; here every source is a heap block of exactly those
dwords and every destination one of exactly the image's bytes, so an access one byte outside is a report.  The program compares what
it gets with the reference's result in its case file, and the test asserts that it ran as many cases as were written.  Nothing
loaded into Python is sanitized."""
import numpy as np

import adam7cases as A
import sancases as S


def test_adam7_core(tmp_path_factory):
    """The whole case list, the empty images and the illegal geometries at the two layouts of test_model_adam7.check()."""
    d = tmp_path_factory.mktemp("san_adam7")
    exe = S.build(str(d / "san_adam7"), ["tests/cxx/san_adam7.cpp", "tests/model/model_adam7.cpp"])
    cases = []
    group = A.all_cases() + A.empty_cases() + A.bad_geometry_cases()
    for i, c in enumerate(group):
        for mis, dst_off, extra in ((i % 4, (1, 7, 12, 3, 0)[i % 5], 5), ((i + 1) % 4, 16, 0)):
            stride = A.stride_of(c, extra)
            want = np.full(dst_off + len(c.rows) * stride + 9, A.FILL, np.uint8)
            for r, row in enumerate(c.rows):
                want[dst_off + r * stride:dst_off + r * stride + len(row)] = np.frombuffer(row, np.uint8)
            cases.append(["%s mis %d off %d" % (c.name, mis, dst_off), c.src, mis, dst_off, stride, c.width, c.height, c.bits, A.ROW_SLICES,
                          c.status, c.d0, c.d1, want.tobytes()])
    n = S.write_cases(str(d / "cases.bin"), cases)
    assert n == 2 * (757 + 2 + 8)
    S.run(exe, str(d / "cases.bin"), n)
