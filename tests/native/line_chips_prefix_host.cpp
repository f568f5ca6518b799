// Stand-alone driver of the line chip decoder (mosaic_amd/csrc/line_chips_build.h) for the sanitizer
// run of tests/test_line_join.py: every non-empty proper prefix of a valid MULTILINESTRING and of a
// valid MULTIPOINT, in both byte orders and with Z ordinates, is handed to the decoder in a heap block
// of exactly its length, so a read past the prefix is a sanitizer report.  Prints one line per
// geometry: "<name> <prefixes> <prefixes answered MOSAIC_E_WKB> <status of the whole> <pieces> <status
// of the empty row>".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "line_chips_build.h"

using namespace mosaic;

namespace {

struct Writer {
    std::vector<uint8_t> b;
    bool le;
    void u8(uint8_t v) { b.push_back(v); }
    void u32(uint32_t v) {
        for (int i = 0; i < 4; i++) b.push_back((uint8_t)(v >> (8 * (le ? i : 3 - i))));
    }
    void f64(double d) {
        uint64_t u;
        memcpy(&u, &d, 8);
        for (int i = 0; i < 8; i++) b.push_back((uint8_t)(u >> (8 * (le ? i : 7 - i))));
    }
    void head(uint32_t type, bool z) {
        u8(le ? 1 : 0);
        u32(type + (z ? 1000 : 0));
    }
};

std::vector<uint8_t> multilinestring(bool le, bool z) {
    Writer w{{}, le};
    w.head(5, z);
    w.u32(3);
    const int n[3] = {2, 0, 4};  // an empty member in the middle
    for (int k = 0; k < 3; k++) {
        w.head(2, z);
        w.u32((uint32_t)n[k]);
        for (int i = 0; i < n[k]; i++) {
            w.f64(10.0 * k + i);
            w.f64(0.5 * i - k);
            if (z) w.f64(7.0);
        }
    }
    return w.b;
}

std::vector<uint8_t> multipoint(bool le, bool z) {
    Writer w{{}, le};
    w.head(4, z);
    w.u32(3);
    for (int k = 0; k < 3; k++) {
        w.head(1, z);
        w.f64(1.5 * k);
        w.f64(-2.0 * k);
        if (z) w.f64(7.0);
    }
    return w.b;
}

int decode(const uint8_t* p, size_t len, size_t* pieces) {
    const uint8_t core = 0;
    const int64_t cell = 1;
    const int32_t key = 0;
    const int64_t off[2] = {0, (int64_t)len};
    LineChipBuilder b;
    std::string err;
    const int rc = build_line_chips(1, &core, &cell, &key, off, 0, p, b, err);
    *pieces = b.piece_bbox.size();
    return rc;
}

int run(const char* name, const std::vector<uint8_t>& g) {
    int64_t n = 0, refused = 0;
    size_t pieces = 0;
    for (size_t len = 1; len < g.size(); len++) {
        uint8_t* block = (uint8_t*)malloc(len);
        memcpy(block, g.data(), len);
        n++;
        if (decode(block, len, &pieces) == MOSAIC_E_WKB) refused++;
        free(block);
    }
    const int whole = decode(g.data(), g.size(), &pieces);
    size_t none = 0;
    const int empty = decode(nullptr, 0, &none);
    printf("%s %lld %lld %d %zu %d\n", name, (long long)n, (long long)refused, whole, pieces, empty);
    return 0;
}

}  // namespace

int main() {
    for (int le = 0; le < 2; le++)
        for (int z = 0; z < 2; z++) {
            const std::string tag = std::string(le ? "le" : "be") + (z ? "_z" : "");
            run(("multilinestring_" + tag).c_str(), multilinestring(le, z));
            run(("multipoint_" + tag).c_str(), multipoint(le, z));
        }
    return 0;
}
