// Stand-alone sanitizer program for the host twins of the foreground masks and the erase (csrc/foreground.hip,
// fusg_foreground_masks_host and fusg_erase_boxes_host: the header's per-box code on one thread).  CPU only - it never touches a GPU:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined tests/sanitize/foreground_host_main.cpp \
//       future_urban_scene_generation_amd/csrc/foreground.hip -o foreground_asan && ./foreground_asan
// Frames of exactly h x w pixels with ONE box that is the whole frame (widths 1 .. 130 across the word seams, heights 1, 2, 37), so
// that any read outside the box is a read outside an exactly-sized heap buffer; radii at their largest (3 / 7 / 15) and at 0; a
// mask buffer of exactly the bytes the accepted boxes take, with refused boxes (out of the frame, over the bound, out of the
// buffer) between them.  Every mask byte is 0 or 255, n_mask counts the 255s, a refused box is flagged and nothing else; the erase
// equals the rule written out here, overlapping boxes included; bad arguments are refused.
#include <cstdint>
#include <cstdio>
#include <vector>
#include "fusg_stubs.h"

static uint32_t rnd(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 8; }

// a background, and a frame that differs from it by 60 on one channel in blocks of 3 x 3 with some single pixels flipped
static void images(int H, int W, uint32_t seed, std::vector<uint8_t>& fr, std::vector<uint8_t>& bg) {
    fr.assign((size_t)H * W * 3, 0);
    bg.assign((size_t)H * W * 3, 0);
    std::vector<uint8_t> coarse((size_t)(H / 3 + 1) * (W / 3 + 1));
    for (auto& c : coarse) c = rnd(seed) % 10 < 6;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            bool on = coarse[(size_t)(y / 3) * (W / 3 + 1) + x / 3] != 0;
            if (rnd(seed) % 32 == 0) on = !on;
            for (int c = 0; c < 3; ++c) {
                const uint8_t b = (uint8_t)(10 + rnd(seed) % 90);
                bg[((size_t)y * W + x) * 3 + c] = b;
                fr[((size_t)y * W + x) * 3 + c] = (uint8_t)(b + (on && c == 1 ? 60 : rnd(seed) % 5));
            }
        }
}

int main() {
    long total = 0, refused = 0;
    const int params[3][4] = {{24, 1, 3, 0}, {24, 3, 7, 15}, {0, 0, 0, 0}};
    for (int w : {1, 31, 32, 33, 63, 64, 65, 130})
        for (int h : {1, 2, 37})
            for (const auto& p : params) {
                std::vector<uint8_t> fr, bg;
                images(h, w, (uint32_t)(w * 131 + h), fr, bg);
                const void* fp[1] = {fr.data()};
                const void* gp[1] = {bg.data()};
                const int32_t rows[2] = {0, 1};
                std::vector<int32_t> box = {0, 0, w, h}, core = {w / 4, h / 4, w - w / 4, h - h / 4}, stats(4, -1);
                std::vector<int64_t> offs = {0};
                std::vector<uint8_t> mask((size_t)w * h, 7);
                if (fusg_foreground_masks_host(fp, gp, rows, 1, h, w, box.data(), core.data(), offs.data(), 1, p[0], p[1], p[2], p[3], 1, h, w,
                                               mask.data(), (int64_t)mask.size(), stats.data()) != FUSG_OK) return 1;
                long n = 0;
                for (uint8_t m : mask) {
                    if (m != 0 && m != 255) return 2;
                    n += m == 255;
                }
                if (stats[2] != n || (stats[3] & 4) || stats[0] < 0 || stats[0] > w * h || stats[1] > w * h) return 3;
                total += n;
            }
    // several boxes over two frames, refused ones between them; the mask buffer holds exactly the accepted boxes' bytes
    {
        const int H = 40, W = 70;
        std::vector<uint8_t> f0, b0, f1, b1;
        images(H, W, 5u, f0, b0);
        images(H, W, 6u, f1, b1);
        const void* fp[2] = {f0.data(), f1.data()};
        const void* gp[2] = {b0.data(), b1.data()};
        const int32_t rows[3] = {0, 4, 8};
        std::vector<int32_t> box = {0, 0, 70, 40,  5, 5, 71, 20,  -1, 0, 10, 10,  30, 10, 65, 40,
                                    0, 0, 33, 33,  10, 10, 10, 30,  60, 30, 70, 40,  0, 0, 20, 41};
        std::vector<int32_t> core = {20, 10, 50, 30,  0, 0, 9, 9,  0, 0, 9, 9,  -100, -100, 1000, 1000,
                                     5, 5, 20, 20,  0, 0, 70, 40,  100, 100, 120, 120,  0, 0, 5, 5};
        const long sz[8] = {70 * 40, 0, 0, 35 * 30, 33 * 33, 0, 10 * 10, 0};
        std::vector<int64_t> offs(8);
        long at = 0;
        for (int b = 0; b < 8; ++b) { offs[b] = at; at += sz[b]; }
        offs[1] = -5;
        offs[6] = at - 99;                                                  // box 6 of 100 bytes: one byte past the end - refused
        std::vector<uint8_t> mask((size_t)at - 100, 7);
        std::vector<int32_t> stats(32, -1);
        if (fusg_foreground_masks_host(fp, gp, rows, 2, H, W, box.data(), core.data(), offs.data(), 8, 24, 1, 3, 2, 1, 40, 70, mask.data(),
                                       (int64_t)mask.size(), stats.data()) != FUSG_OK) return 4;
        const bool want_refused[8] = {false, true, true, false, false, false, true, true};
        for (int b = 0; b < 8; ++b) {
            if (((stats[4 * b + 3] & 4) != 0) != want_refused[b]) return 5;
            if (want_refused[b] && (stats[4 * b] || stats[4 * b + 1] || stats[4 * b + 2] || stats[4 * b + 3] != 4)) return 6;
            refused += want_refused[b];
        }
        for (uint8_t m : mask) if (m != 0 && m != 255) return 7;          // every byte belongs to an accepted box
        // the same launch with a bound of 32 x 70: the 40-high and 33-high boxes are refused too, their bytes stay
        std::vector<uint8_t> mask2(mask.size(), 7);
        if (fusg_foreground_masks_host(fp, gp, rows, 2, H, W, box.data(), core.data(), offs.data(), 8, 24, 1, 3, 2, 1, 32, 70, mask2.data(),
                                       (int64_t)mask2.size(), stats.data()) != FUSG_OK) return 8;
        if (stats[3] != 4 || stats[4 * 4 + 3] != 4 || (stats[3 * 4 + 3] & 4)) return 9;
        for (long i = 0; i < sz[0]; ++i) if (mask2[(size_t)i] != 7) return 10;
        for (long i = 0; i < sz[3]; ++i) if (mask2[(size_t)(offs[3] + i)] != mask[(size_t)(offs[3] + i)]) return 11;
        // erase with the first launch's masks: boxes 0, 3, 4 overlap
        std::vector<uint8_t> dst((size_t)H * W * 3, 1), want(f0);
        const int32_t* bx = box.data();
        if (fusg_erase_boxes_host(f0.data(), b0.data(), H, W, mask.data(), (int64_t)mask.size(), offs.data(), bx, 8, dst.data()) != FUSG_OK) return 12;
        for (int b = 0; b < 8; ++b) {
            if (want_refused[b]) continue;
            const int x0 = bx[4 * b], y0 = bx[4 * b + 1], bw = bx[4 * b + 2] - x0, bh = bx[4 * b + 3] - y0;
            for (int i = 0; i < bh; ++i)
                for (int j = 0; j < bw; ++j)
                    if (mask[(size_t)(offs[b] + (long)i * bw + j)])
                        for (int c = 0; c < 3; ++c) want[((size_t)(y0 + i) * W + x0 + j) * 3 + c] = b0[((size_t)(y0 + i) * W + x0 + j) * 3 + c];
        }
        if (dst != want || dst == f0) return 13;
        if (fusg_erase_boxes_host(f0.data(), b0.data(), H, W, nullptr, 0, nullptr, nullptr, 0, dst.data()) != FUSG_OK || dst != f0) return 14;
        // bad arguments
        if (fusg_erase_boxes_host(f0.data(), b0.data(), H, W, mask.data(), (int64_t)mask.size(), offs.data(), bx, 8, f0.data()) != FUSG_ERR_INVALID) return 15;
        if (fusg_foreground_masks_host(fp, gp, rows, 2, H, W, box.data(), core.data(), offs.data(), 8, 255, 1, 3, 2, 1, 40, 70, mask.data(),
                                       (int64_t)mask.size(), stats.data()) != FUSG_ERR_INVALID) return 16;
        if (fusg_foreground_masks_host(fp, gp, rows, 2, H, W, box.data(), core.data(), offs.data(), 8, 24, 4, 3, 2, 1, 40, 70, mask.data(),
                                       (int64_t)mask.size(), stats.data()) != FUSG_ERR_INVALID) return 17;
        const int32_t bad_rows[3] = {0, 5, 7};
        if (fusg_foreground_masks_host(fp, gp, bad_rows, 2, H, W, box.data(), core.data(), offs.data(), 8, 24, 1, 3, 2, 1, 40, 70, mask.data(),
                                       (int64_t)mask.size(), stats.data()) != FUSG_ERR_INVALID) return 18;
        if (fusg_foreground_masks_host(nullptr, nullptr, nullptr, 0, H, W, nullptr, nullptr, nullptr, 0, 24, 1, 3, 2, 1, 0, 0, nullptr, 0,
                                       nullptr) != FUSG_OK) return 19;  // n = 0: nothing is read or written
    }
    std::printf("mask pixels %ld, refused boxes %ld\n", total, refused);
    return total > 0 && refused == 4 ? 0 : 20;
}
