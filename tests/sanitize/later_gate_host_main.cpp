// Stand-alone sanitizer program for the host twin of the later-frame gate (csrc/pose_geometry.hip, fusg_later_gate_host: the
// header's per-row code in a plain loop).  CPU only - it never touches a GPU:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined tests/sanitize/later_gate_host_main.cpp \
//       future_urban_scene_generation_amd/csrc/pose_geometry.hip -o later_gate_asan && ./later_gate_asan
// It runs J = 1, 9 and 200 rows at P = 5 and 7 with exactly-sized heap buffers (counts [J][7][2], covered [J], dst_vis [J][P],
// valid [J], box rows [J][8]), so that any read or write outside them is reported, compares every output with the rule written
// out here, and checks that J = 0 touches nothing and that bad arguments are refused.
#include <cstdint>
#include <cstdio>
#include <vector>
#include "fusg_stubs.h"

int main() {
    long visible = 0, invalid = 0;
    for (int P : {5, 7}) {
        for (int J : {1, 9, 200}) {
            std::vector<int32_t> counts((size_t)J * 14), covered((size_t)J), valid((size_t)J, -1), box((size_t)J * 8);
            std::vector<uint8_t> vis((size_t)J * P, 7);
            for (int j = 0; j < J; ++j) {
                covered[j] = (j % 4 == 1) ? 0 : 1 + 37 * j;
                for (int p = 0; p < 7; ++p) {
                    const int32_t a = (p == 6 && j % 5 == 0) ? INT32_MAX : 10 * ((j * 7 + p) % 92161);       // up to 921 600, a tie each
                    counts[((size_t)j * 7 + p) * 2] = a;
                    counts[((size_t)j * 7 + p) * 2 + 1] = a == INT32_MAX ? INT32_MAX - (j % 3) : (a ? 9 * (a / 10) + (j + p) % 3 - 1 : 0);
                }
                for (int k = 0; k < 8; ++k) box[(size_t)j * 8 + k] = 1 + j * 8 + k;
            }
            if (fusg_later_gate_host(counts.data(), covered.data(), J, P, vis.data(), valid.data(), box.data()) != FUSG_OK) return 1;
            for (int j = 0; j < J; ++j) {
                const bool ok = covered[j] > 0;
                if (valid[j] != (ok ? 1 : 0)) return 2;
                invalid += !ok;
                for (int p = 0; p < P; ++p) {
                    const volatile double lim = 0.9 * (double)counts[((size_t)j * 7 + p) * 2];
                    const bool want = ok && (double)counts[((size_t)j * 7 + p) * 2 + 1] > lim;
                    if (vis[(size_t)j * P + p] != (want ? 1 : 0)) return 3;
                    visible += want;
                }
                for (int k = 0; k < 8; ++k)
                    if (box[(size_t)j * 8 + k] != (ok ? 1 + j * 8 + k : 0)) return 4;
            }
            std::vector<uint8_t> vis2((size_t)J * P, 7);                                 // box rows are optional
            if (fusg_later_gate_host(counts.data(), covered.data(), J, P, vis2.data(), valid.data(), nullptr) != FUSG_OK || vis2 != vis) return 5;
        }
    }
    int32_t none = 0;
    uint8_t nov = 0;
    if (fusg_later_gate_host(&none, &none, 0, 5, &nov, &none, nullptr) != FUSG_OK) return 6;    // J = 0: nothing is read or written
    if (fusg_later_gate_host(nullptr, &none, 1, 5, &nov, &none, nullptr) != FUSG_ERR_INVALID) return 7;
    if (fusg_later_gate_host(&none, &none, 1, 0, &nov, &none, nullptr) != FUSG_ERR_INVALID) return 8;
    if (fusg_later_gate_host(&none, &none, 1, 8, &nov, &none, nullptr) != FUSG_ERR_INVALID) return 9;
    if (fusg_later_gate_host(&none, &none, -1, 5, &nov, &none, nullptr) != FUSG_ERR_INVALID) return 10;
    std::printf("visible planes %ld, invalid rows %ld\n", visible, invalid);
    return visible > 0 && invalid > 0 ? 0 : 11;
}
