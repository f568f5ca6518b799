// Host side of k_tess_clip_ll's records (mosaic_amd/csrc/tess_records.h) on a hand-made ClipResult:
// records of finished tasks in shuffled order beside records of a task that went to the host, a
// sentinel, records naming no task, and records that name a finished task but point outside verts
// (what a slot reserved and never written holds when the buffers carry an earlier launch's records).
// Prints what filter_records keeps and what ClippedChips::index / chip read, for
// tests/test_clip_records.py to compare; vertices no valid record covers are NaN, so a chip built from
// them shows.  Also built by hand with -fsanitize=address,undefined: a read outside verts aborts there.
//   g++ -O1 -g -std=c++17 -I mosaic_amd/csrc -o clip_records tests/native/clip_records_host.cpp
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <limits>
#include <vector>

#include "tess_records.h"

using namespace mosaic::tessclip;

struct Tokens {  // ClippedChips::chip's writer: the WKB fields as text
    void u8(uint8_t v) { printf(" b%u", (unsigned)v); }
    void u32(uint32_t v) { printf(" u%u", (unsigned)v); }
    void f64(double v) {
        if (isnan(v)) printf(" nan");
        else printf(" %.1f", v);
    }
};

int main() {
    const int64_t n_cand = 32, n_verts = 40;
    const std::vector<int64_t> tasks = {3, 7, 10, 12, 20, 25, 28, 30};
    ClippedChips cc;
    ClipResult& r = cc.r;
    r.status = {0, 2, 1, 0, 0, 0, 0, 2};
    r.verts.assign((size_t)n_verts * 2, std::numeric_limits<double>::quiet_NaN());
    auto fill = [&](int64_t off, int32_t n) {
        for (int64_t v = off; v < off + n; v++) r.verts[2 * v] = (double)v, r.verts[2 * v + 1] = -(double)v - 0.5;
    };
    fill(0, 5), fill(5, 4), fill(9, 4), fill(13, 7), fill(24, 4), fill(28, 4), fill(36, 4);
    const int64_t big = std::numeric_limits<int64_t>::max();
    r.rings = {
        {25, 1, 0, 36, 4, 0},   // valid, ends exactly at verts' end
        {12, 0, 1, 38, 5, 0},   // live task, off + n past verts: demotes 12
        {3, 1, 0, 9, 4, 0},     // valid (second part of 3, before its first: index sorts)
        {-1, 0, 0, 0, 0, 0},    // sentinel
        {10, 0, 0, 20, 4, 0},   // a task that went to the host
        {3, 0, 1, 5, 4, 0},     // valid (hole)
        {20, 0, 0, -3, 4, 0},   // live task, negative off: demotes 20
        {7, 0, 0, 13, 7, 0},    // valid (status 2: the chip equals its cell)
        {99, 0, 0, 0, 4, 0},    // no such candidate
        {5, 0, 0, 0, 4, 0},     // a candidate that is no task
        {12, 0, 0, 24, 4, 0},   // valid on its own, but its task is demoted: dropped too
        {3, 0, 0, 0, 5, 0},     // valid (shell)
        {20, 1, 0, big, 3, 0},  // off + n overflows int64
        {30, 0, 0, 13, 0, 0},   // live task, n = 0: demotes 30
        {25, 0, 0, 28, 4, 0},   // valid
    };
    r.parts = {
        {25, 1, 1}, {10, 0, 1}, {3, 1, 1}, {-1, 0, 0}, {12, 0, 1}, {28, -2, 1} /* demotes 28 */,
        {7, 0, 1},  {3, 0, 1},  {20, 0, 1}, {99, 0, 1}, {25, 0, 1}, {30, 0, 1},
    };
    const int64_t demoted = filter_records(tasks, &r);
    printf("demoted %lld\nstatus", (long long)demoted);
    for (uint8_t s : r.status) printf(" %u", (unsigned)s);
    printf("\n");
    cc.index(n_cand, tasks);
    for (const ClipRing& q : r.rings)
        printf("ring %lld %d %d %lld %d\n", (long long)q.cand, q.part, q.ring, (long long)q.off, q.n);
    for (const ClipPart& q : r.parts) printf("part %lld %d %d\n", (long long)q.cand, q.part, q.keep);
    // every record left points into verts
    for (const ClipRing& q : r.rings)
        if (q.off < 0 || q.n < 1 || q.off + q.n > n_verts) return 2;
    for (int64_t k = 0; k < n_cand; k++) {
        if (cc.redo(k)) continue;
        printf("chip %lld cell %d:", (long long)k, (int)cc.is_cell(k));
        Tokens w;
        if (!cc.chip(k, w)) printf(" none");
        printf("\n");
    }
    return 0;
}
