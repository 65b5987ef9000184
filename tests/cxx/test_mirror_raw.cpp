// test_mirror_raw.cpp -- rawDecompress / rawDecompressMany of the C++ module mirror (pure_zlib_amd/cxx/codec_compression_zlib.hpp):
// the reference's nine .z/.gold cases with their zlib wrapper stripped (2 bytes of header, 4 of trailer), the chunk rule and two
// error values.  Usage: test_mirror_raw <dir with name.z/name.gold pairs>.  Needs a GPU.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../pure_zlib_amd/cxx/codec_compression_zlib.hpp"

using namespace Codec::Compression::Zlib;

static ByteString readFile(const std::string &path)
{
    ByteString s;
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path.c_str());
        exit(2);
    }
    char buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) s.append(buf, n);
    fclose(f);
    return s;
}

static int failures = 0;
#define CHECK(cond, name)                                      \
    do {                                                       \
        const bool ok_ = (cond);                               \
        printf("%-62s %s\n", name, ok_ ? "OK" : "FAILED");     \
        if (!ok_) ++failures;                                  \
    } while (0)

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    const std::string dir = argv[1];
    const char *cases[] = {"randtest1", "randtest2", "randtest3", "rfctest1", "rfctest2", "rfctest3", "zerotest1", "zerotest2", "zerotest3"};
    std::vector<LazyByteString> all;
    std::vector<ByteString> golds;
    try {
        for (const char *tc : cases) {
            const ByteString z = readFile(dir + "/" + tc + ".z"), gold = readFile(dir + "/" + tc + ".gold");
            const ByteString raw = z.substr(2, z.size() - 6);
            const Either r = rawDecompress(fromChunksOf(raw, 1000));
            CHECK(r.is_right && r.right == gold, (std::string("rawDecompress (strip ") + tc + ".z) == " + tc + ".gold").c_str());
            all.push_back(fromStrict(raw));
            golds.push_back(gold);
        }
        const std::vector<Either> rs = rawDecompressMany(all);
        bool ok = rs.size() == all.size();
        for (size_t i = 0; ok && i < rs.size(); ++i) ok = rs[i].is_right && rs[i].right == golds[i];
        CHECK(ok, "rawDecompressMany [nine cases] == map Right golds");
        const ByteString raw1 = toStrict(all[3]);
        // trailing bytes inside the last chunk are ignored, a whole chunk behind the final block is not (Zlib.hs:46-49)
        const Either t1 = rawDecompress(LazyByteString{raw1 + "tail"});
        CHECK(t1.is_right && t1.right == golds[3], "bytes behind the final block, same chunk: Right");
        const Either t2 = rawDecompress(LazyByteString{raw1, "tail"});
        CHECK(!t2.is_right && t2.left.show() == "Decompression error: Finished with data remaining.", "a whole chunk behind it: Left");
        const Either t3 = rawDecompress(fromStrict(raw1.substr(0, raw1.size() / 2)));
        CHECK(!t3.is_right && t3.left.show() == "Decompression error: Ran out of data mid-decompression 2.", "half a stream: Left, ran out of data");
        const Either t4 = rawDecompress(LazyByteString{});
        CHECK(!t4.is_right, "no input at all: Left");
        const Either t5 = rawDecompress(fromStrict(ByteString("\x07", 1)));
        CHECK(!t5.is_right && t5.left.show() == "Block format error: Unacceptable BTYPE: 3", "BTYPE 3: Left FormatError");
        // a zlib stream is not a raw stream (and the reverse): 0x78 reads as a stored block header with garbage lengths
        const Either t6 = decompress(all[3]);
        CHECK(!t6.is_right, "decompress on a raw stream: Left");
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}
