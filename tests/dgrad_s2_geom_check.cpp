// Stand-alone CPU check of csrc/dgrad_s2_geom.h (built and run by
// tests/test_dgrad_s2_geom.py with -fsanitize=address,undefined; no GPU).
// For every H, W in 1..24, SAME and VALID, and every tile origin:
//  * every LDS chunk the kernel stages has a source that is inside the dy
//    image (16 aligned bytes below the buffer resource's num_records) or is
//    the zero-fill offset, and lands the pixel / channels halo_pix expects;
//  * every dx pixel is owned by exactly one (tile, phase, row, lane) slot;
//  * the tap sets per phase, read from the simulated LDS image, reproduce a
//    brute-force conv2d_transpose (integer data: exact).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dgrad_s2_geom.h"

static int fails = 0;
#define CHECK(c, ...)                                  \
    do {                                               \
        if (!(c)) {                                    \
            if (++fails < 20) { printf("FAIL %s: ", #c); printf(__VA_ARGS__); printf("\n"); } \
        }                                              \
    } while (0)

static void same_pads(int in, int* out, int* pb, int* pa) {
    *out = (in + 1) / 2;
    int total = (*out - 1) * 2 + 4 - in;
    if (total < 0) total = 0;
    *pb = total / 2;
    *pa = total - total / 2;
}

static long long dyv(int oh, int ow, int k) { return (oh * 31 + ow * 7 + k * 3) % 17 - 8; }
static long long wv(int r, int s, int k) { return (r * 5 + s * 11 + k) % 13 - 6; }

static long run(int H, int W, bool same, int K, int ldy) {
    int OH, OW, pt = 0, pl = 0, d0;
    if (same) {
        same_pads(H, &OH, &pt, &d0);
        same_pads(W, &OW, &pl, &d0);
    } else {
        if (H < 4 || W < 4) return 0;
        OH = (H - 4) / 2 + 1;
        OW = (W - 4) / 2 + 1;
    }
    CHECK(dg2::shape_ok(1, H, W, 32, OH, OW, K, 4, 4, 2, 2, 1, 1, pt, pl, 32, ldy), "H %d W %d", H, W);
    const long records = ((long)(OH * OW - 1) * ldy + K) * 2;      // the kernel's num_records
    const int rc = dg2::row_chunks(K), nchunk = dg2::lds_bytes(K) / 16;
    std::vector<int> owners(H * W, 0);
    std::vector<long long> lds((size_t)nchunk * 8);
    const int ty = dg2::tiles_y(H, pt), tx = dg2::tiles_x(W, pl);
    long checked = 0;
    for (int t = 0; t < ty * tx; ++t) {
        const int u0 = (t / tx) * dg2::TH, v0 = (t % tx) * dg2::TW;
        CHECK(u0 % 2 == 0 && v0 % 2 == 0, "origin");
        // ---- staging: what every lane of every 1 KiB piece reads
        for (int q = 0; q < nchunk; ++q) {
            const unsigned src = dg2::halo_src(q, u0, v0, OH, OW, ldy, K);
            const int hp = q / rc, kc = q % rc;
            long long* dst = &lds[(size_t)q * 8];
            if (src == dg2::OOB) {
                CHECK((long)src >= records, "OOB below num_records");
                for (int e = 0; e < 8; ++e) dst[e] = 0;
                // zero-fill only where the data is padding or outside the map
                if (hp < dg2::HPIX && kc < K / 8) {
                    const int oh = (u0 >> 1) - 1 + hp / dg2::HWD, ow = (v0 >> 1) - 1 + hp % dg2::HWD;
                    CHECK(oh < 0 || oh >= OH || ow < 0 || ow >= OW, "in-map pixel zero-filled (%d,%d)", oh, ow);
                }
                continue;
            }
            CHECK(src % 16 == 0 && (long)src + 16 <= records, "src %u records %ld", src, records);
            CHECK(hp < dg2::HPIX && kc < K / 8, "chunk %d", q);
            const int el = (int)(src / 2), pix = el / ldy, k0 = el % ldy;
            const int oh = pix / OW, ow = pix % OW;
            CHECK(oh == (u0 >> 1) - 1 + hp / dg2::HWD && ow == (v0 >> 1) - 1 + hp % dg2::HWD && k0 == kc * 8,
                  "chunk %d lands (%d,%d,%d)", q, oh, ow, k0);
            CHECK(oh >= 0 && oh < OH && ow >= 0 && ow < OW && k0 + 8 <= K, "range");
            for (int e = 0; e < 8; ++e) dst[e] = dyv(oh, ow, k0 + e);
            ++checked;
        }
        // ---- the four phases' taps from that image
        for (int ph = 0; ph < 2; ++ph)
            for (int pw = 0; pw < 2; ++pw)
                for (int i = 0; i < dg2::PH; ++i)
                    for (int j = 0; j < dg2::PW; ++j) {
                        const int ih = dg2::slot_ih(u0, ph, i, pt), iw = dg2::slot_iw(v0, pw, j, pl);
                        if (ih < 0 || ih >= H || iw < 0 || iw >= W) continue;
                        ++owners[ih * W + iw];
                        CHECK(((ih + pt) & 1) == ph && ((iw + pl) & 1) == pw, "phase");
                        long long got = 0;
                        for (int jr = 0; jr < 2; ++jr)
                            for (int js = 0; js < 2; ++js) {
                                const int hp = dg2::halo_pix(i, j, jr, js);
                                CHECK(hp >= 0 && hp < dg2::HPIX, "halo_pix %d", hp);
                                for (int k = 0; k < K; ++k) {
                                    const size_t a = (size_t)(hp * rc + k / 8) * 8 + k % 8;
                                    CHECK(a < lds.size(), "lds read");
                                    got += lds[a] * wv(ph + 2 * jr, pw + 2 * js, k);
                                }
                            }
                        long long ref = 0;      // brute-force conv2d_transpose
                        for (int oh = 0; oh < OH; ++oh)
                            for (int ow = 0; ow < OW; ++ow)
                                for (int r = 0; r < 4; ++r)
                                    for (int s = 0; s < 4; ++s)
                                        if (2 * oh + r - pt == ih && 2 * ow + s - pl == iw)
                                            for (int k = 0; k < K; ++k) ref += dyv(oh, ow, k) * wv(r, s, k);
                        CHECK(got == ref, "dx(%d,%d) H %d W %d same %d: %lld vs %lld", ih, iw, H, W, (int)same, got, ref);
                    }
    }
    for (int i = 0; i < H * W; ++i) CHECK(owners[i] == 1, "pixel %d of %dx%d owned %d times", i, H, W, owners[i]);
    return checked;
}

int main() {
    long checked = 0;
    for (int H = 1; H <= 24; ++H)
        for (int W = 1; W <= 24; ++W)
            for (int same = 0; same < 2; ++same) checked += run(H, W, same != 0, 32, H % 2 ? 40 : 32);
    // wider tiles in x (more than one tile column), K = 64 / the LDS maximum
    checked += run(13, 70, true, 64, 64);
    checked += run(19, 67, false, 64, 72);
    checked += run(9, 33, true, dg2::KMAX, dg2::KMAX);
    // what the shape predicate must refuse
    CHECK(!dg2::shape_ok(1, 8, 8, 32, 4, 4, 32, 3, 3, 2, 2, 1, 1, 0, 0, 32, 32), "3x3");
    CHECK(!dg2::shape_ok(1, 8, 8, 32, 4, 4, 32, 4, 4, 2, 2, 2, 2, 1, 1, 32, 32), "dilation");
    CHECK(!dg2::shape_ok(1, 8, 8, 32, 4, 4, 24, 4, 4, 2, 2, 1, 1, 1, 1, 32, 24), "K % 32");
    CHECK(!dg2::shape_ok(1, 8, 8, 24, 4, 4, 32, 4, 4, 2, 2, 1, 1, 1, 1, 24, 32), "C = 24");
    CHECK(!dg2::shape_ok(1, 8, 8, 32, 4, 4, dg2::KMAX + 32, 4, 4, 2, 2, 1, 1, 1, 1, 32, dg2::KMAX + 32), "K max");
    CHECK(!dg2::shape_ok(1, 70000, 70000, 32, 35000, 35000, 32, 4, 4, 2, 2, 1, 1, 1, 1, 32, 32), "31-bit offsets");
    CHECK(dg2::lds_bytes(dg2::KMAX) <= 160 * 1024, "LDS");
    printf("%s: %ld staged chunks checked, %d failures\n", fails ? "FAILED" : "ok", checked, fails);
    return fails ? 1 : 0;
}
