// The background frame of a video - the per-pixel, per-channel lower median of the frames in which no tracker box covers the
// pixel - on the device (include/fusg.h: fusg_background_median_u8) with a host twin by the same code (background.h, which
// states the definition).  Off every product pass: nothing calls this unless asked.
//   one kernel   a workgroup of 256 owns 256 consecutive dwords of the frames' 3 H W bytes (about 341 pixels of a row).
//                1 cull: wave w takes frames w, w + 4, ..; lane l grows box l of the frame by the margin, cuts it to the image
//                  and keeps it if it meets the rectangle that holds the workgroup's pixels.  A wave's kept boxes go into its
//                  own list in LDS, each with its frame, packed by ballot + prefix count; the loads of all its frames are
//                  issued before the first test, so a workgroup waits for the table once.
//                2 cover: a lane's dword holds bytes of two pixels; it walks the four lists (uniform LDS addresses: its tile's
//                  boxes only, a few dozen of up to 4096) and sets, per pixel, bit f for every box of frame f that covers it.
//                3 select: the lane reads its dword of every frame (consecutive lanes, consecutive addresses), drops it into
//                  bit planes and selects the four bytes' lower medians in eight rounds (background.h: median4), all in
//                  registers: the kernel is a template on the frame count's bucket (8 / 16 / 32 / 64), every loop unrolled.
//                4 one dword of bg, and the count byte of every pixel whose first byte the dword holds.
//   byte kernel  the same body with byte loads and stores, for what dwords cannot reach: the last 3 H W mod 4 bytes, and
//                everything when a frame or bg is not 4-byte aligned (a slice of a [T, H, W, 3] stack with odd 3 H W).
// No atomics, no scratch memory: a pixel's bytes depend on its own samples and boxes only.
#include <vector>
#include "common.h"
#include "background.h"

namespace fusg {

struct BgK {
    const unsigned char* frames[bg::MAX_T];                       // entries past T repeat the last frame (read, never counted)
    int offs[bg::MAX_T + 1];                                      // frame f's boxes: rows [offs[f], offs[f + 1]) of `boxes`; past T: offs[T]
    const int32_t* boxes;
    unsigned char* bg;
    unsigned char* count;
    long n_bytes;                                                 // 3 H W
    int T, H, W, margin, min_valid;
};

// what a lane does once it knows its two pixels' covered-frame masks; load(f): its dword (the bytes from b on) of frame f
template <int TB, class Load>
FUSG_HD uint32_t lane_result(const BgK& k, long b, uint64_t cov_a, uint64_t cov_b, int& n_a, int& n_b, bool& has_b, Load load) {
    const int pa = (int)(b / 3);
    has_b = pa + 1 < k.H * k.W;
    const bg::Pick A = bg::pick(cov_a, k.T, k.min_valid), B = bg::pick(cov_b, k.T, k.min_valid);
    n_a = A.n;
    n_b = B.n;
    return bg::median4<TB>(k.T, A.mask, has_b ? B.mask : 0ull, bg::sel_a(b), load);
}

// dwords [d0, d0 + 256 gridDim.x) of the byte stream, cut at n_bytes; VEC: every one of them whole and 4-byte aligned
template <int TB, bool VEC>
__global__ __launch_bounds__(256) void background_median_kernel(const BgK k, long d0) {
    constexpr int J = TB / 4;                                     // frames per wave: wave w culls w, w + 4, ..
    __shared__ bg::Rect s_box[4][J * bg::MAX_BOXES];              // wave w's kept boxes, packed in (frame, lane) order ..
    __shared__ unsigned char s_frm[4][J * bg::MAX_BOXES];         // .. and the frame each belongs to
    __shared__ int s_n[4];
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const long b_lo = (d0 + (long)blockIdx.x * 256) * 4;
    const long b_hi = b_lo + 1024 < k.n_bytes ? b_lo + 1024 : k.n_bytes;
    int run = 0;
    if (k.offs[k.T] > 0) {
        const bg::Rect tile = bg::bytes_rect(b_lo, b_hi, k.W);
        int32_t raw[J][4];
        bool has[J];
#pragma unroll
        for (int j = 0; j < J; ++j) {                             // every load first (a row of the table that exists, used or not) ..
            const int f = wave + 4 * j, o = k.offs[f];            // (offs past T repeats offs[T]: no boxes)
            has[j] = lane < k.offs[f + 1] - o;
            const int32_t* row = k.boxes + 4L * (has[j] ? o + lane : 0);
#pragma unroll
            for (int q = 0; q < 4; ++q) raw[j][q] = row[q];
        }
#pragma unroll
        for (int j = 0; j < J; ++j) {                             // .. then the tests, packed by ballot and prefix count: no atomics
            bg::Rect r = {0, 0, 0, 0};
            const bool keep = has[j] && bg::grow(raw[j], k.margin, k.H, k.W, r) && bg::meets(r, tile);
            const unsigned long long kept = __ballot(keep);
            if (keep) {
                const int pos = run + __popcll(kept & ((1ull << lane) - 1ull));
                s_box[wave][pos] = r;
                s_frm[wave][pos] = (unsigned char)(wave + 4 * j);
            }
            run += __popcll(kept);
        }
    }
    if (lane == 0) s_n[wave] = run;
    __syncthreads();
    const long b = b_lo + 4L * t;
    if (VEC ? b + 4 > b_hi : b >= b_hi) return;                   // (the dword kernel leaves a last, partial dword to the byte kernel)
    const int pa = (int)(b / 3), ya = pa / k.W, xa = pa - ya * k.W;
    const int xb = xa + 1 < k.W ? xa + 1 : 0, yb = xa + 1 < k.W ? ya : ya + 1;
    uint64_t cov_a = 0, cov_b = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const int n = s_n[w];
#pragma unroll 4
        for (int i = 0; i < n; ++i) {                             // uniform addresses: every lane reads the same box
            const bg::Rect r = s_box[w][i];
            const int f = s_frm[w][i];
            cov_a |= (uint64_t)bg::inside(r, xa, ya) << f;
            cov_b |= (uint64_t)bg::inside(r, xb, yb) << f;
        }
    }
    int n_a, n_b;
    bool has_b;
    uint32_t res;
    if (VEC) {
        res = lane_result<TB>(k, b, cov_a, cov_b, n_a, n_b, has_b, [&](int f) { return *(const uint32_t*)(k.frames[f] + b); });
        *(uint32_t*)(k.bg + b) = res;
    } else {
        const int nbytes = (int)(k.n_bytes - b < 4 ? k.n_bytes - b : 4);
        res = lane_result<TB>(k, b, cov_a, cov_b, n_a, n_b, has_b, [&](int f) {
            const unsigned char* p = k.frames[f] + b;
            uint32_t v = p[0];
            if (nbytes > 1) v |= (uint32_t)p[1] << 8;
            if (nbytes > 2) v |= (uint32_t)p[2] << 16;
            if (nbytes > 3) v |= (uint32_t)p[3] << 24;
            return v;
        });
        for (int j = 0; j < nbytes; ++j) k.bg[b + j] = (unsigned char)(res >> (8 * j));
    }
    if (b % 3 == 0) k.count[pa] = (unsigned char)n_a;               // the pixels whose first byte is in this dword
    if (has_b) k.count[pa + 1] = (unsigned char)n_b;
}

template <int TB>
static void background_launch_tb(const BgK& k, bool vec, hipStream_t st) {
    const long dwords = (k.n_bytes + 3) / 4, whole = vec ? k.n_bytes / 4 : 0;
    if (whole > 0)
        hipLaunchKernelGGL((background_median_kernel<TB, true>), dim3((unsigned)((whole + 255) / 256)), dim3(256), 0, st, k, 0L);
    if (dwords > whole)
        hipLaunchKernelGGL((background_median_kernel<TB, false>), dim3((unsigned)((dwords - whole + 255) / 256)), dim3(256), 0, st, k, whole);
}

static int background_launch(BgK k, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    bool vec = (((uintptr_t)k.bg) & 3) == 0;
    for (int f = 0; f < k.T; ++f) vec = vec && (((uintptr_t)k.frames[f]) & 3) == 0;
    switch (bg::bucket(k.T)) {
        case 8: background_launch_tb<8>(k, vec, st); break;
        case 16: background_launch_tb<16>(k, vec, st); break;
        case 32: background_launch_tb<32>(k, vec, st); break;
        default: background_launch_tb<64>(k, vec, st); break;
    }
    FUSG_LAUNCH_CHECK("background_median_u8");
    return FUSG_OK;
}

// the host twin of one bucket: every dword by the kernel's lane code, the boxes of a frame tested one by one
template <int TB>
static void background_host_tb(const BgK& k) {
    std::vector<bg::Rect> rects;
    std::vector<int> first(k.T + 1, 0);
    for (int f = 0; f < k.T; ++f) {
        for (int i = k.offs[f]; i < k.offs[f + 1]; ++i) {
            bg::Rect r;
            if (bg::grow(k.boxes + 4L * i, k.margin, k.H, k.W, r)) rects.push_back(r);
        }
        first[f + 1] = (int)rects.size();
    }
    for (long b = 0; b < k.n_bytes; b += 4) {
        const int pa = (int)(b / 3), ya = pa / k.W, xa = pa - ya * k.W;
        const int xb = xa + 1 < k.W ? xa + 1 : 0, yb = xa + 1 < k.W ? ya : ya + 1;
        uint64_t cov_a = 0, cov_b = 0;
        for (int f = 0; f < k.T; ++f) {
            bool a = false, c = false;
            for (int i = first[f]; i < first[f + 1]; ++i) {
                a |= bg::inside(rects[i], xa, ya);
                c |= bg::inside(rects[i], xb, yb);
            }
            cov_a |= (uint64_t)a << f;
            cov_b |= (uint64_t)c << f;
        }
        const int nbytes = (int)(k.n_bytes - b < 4 ? k.n_bytes - b : 4);
        int n_a, n_b;
        bool has_b;
        const uint32_t res = lane_result<TB>(k, b, cov_a, cov_b, n_a, n_b, has_b, [&](int f) {
            uint32_t v = 0;
            for (int j = 0; j < nbytes; ++j) v |= (uint32_t)k.frames[f][b + j] << (8 * j);
            return v;
        });
        for (int j = 0; j < nbytes; ++j) k.bg[b + j] = (unsigned char)(res >> (8 * j));
        if (b % 3 == 0) k.count[pa] = (unsigned char)n_a;
        if (has_b) k.count[pa + 1] = (unsigned char)n_b;
    }
}

}  // namespace fusg

using namespace fusg;

// frame_ptrs and box_offs are HOST tables, read (and checked) here, before anything is launched
static int background_check(const void* const* frame_ptrs, int32_t T, int32_t H, int32_t W, const int32_t* boxes, const int32_t* box_offs,
                            int32_t margin, int32_t min_valid, uint8_t* bg_out, uint8_t* count, const char* what, BgK& k) {
    FUSG_CHECK(T >= 1 && T <= bg::MAX_T, "%s: T = %d frames (1..%d)", what, T, bg::MAX_T);
    if (const int rc = wg::check_frame_size(H, W, what)) return rc;
    FUSG_CHECK(margin >= 0 && margin <= bg::MAX_MARGIN, "%s: margin = %d (0..%d)", what, margin, bg::MAX_MARGIN);
    FUSG_CHECK(min_valid >= 1 && min_valid <= T, "%s: min_valid = %d (1..T = %d)", what, min_valid, T);
    FUSG_CHECK(frame_ptrs && bg_out && count, "%s: frame_ptrs, bg or count is null", what);
    memset(&k, 0, sizeof(k));
    for (int f = 0; f < bg::MAX_T; ++f) {
        const void* p = frame_ptrs[f < T ? f : T - 1];
        FUSG_CHECK(p != nullptr, "%s: frame %d is null", what, f);
        k.frames[f] = (const unsigned char*)p;
    }
    if (box_offs) {
        FUSG_CHECK(box_offs[0] == 0, "%s: the box offsets start at %d, not at 0", what, box_offs[0]);
        for (int f = 0; f < T; ++f) {
            const long nb = (long)box_offs[f + 1] - box_offs[f];
            FUSG_CHECK(nb >= 0 && nb <= bg::MAX_BOXES, "%s: frame %d has %ld boxes (0..%d)", what, f, nb, bg::MAX_BOXES);
            k.offs[f + 1] = box_offs[f + 1];
        }
        for (int f = T; f < bg::MAX_T; ++f) k.offs[f + 1] = box_offs[T];
        FUSG_CHECK(box_offs[T] == 0 || boxes != nullptr, "%s: %d boxes and a null box table", what, box_offs[T]);
    }
    k.boxes = boxes;
    k.bg = bg_out;
    k.count = count;
    k.n_bytes = 3L * H * W;
    k.T = T; k.H = H; k.W = W; k.margin = margin; k.min_valid = min_valid;
    return FUSG_OK;
}

extern "C" int fusg_background_median_u8(const void* const* frame_ptrs, int32_t T, int32_t H, int32_t W, const int32_t* boxes,
                                         const int32_t* box_offs, int32_t margin, int32_t min_valid, uint8_t* bg_out, uint8_t* count,
                                         void* stream) {
    BgK k;
    const int rc = background_check(frame_ptrs, T, H, W, boxes, box_offs, margin, min_valid, bg_out, count, "background_median_u8", k);
    if (rc != FUSG_OK) return rc;
    return fusg::plan_dispatch(background_launch, stream, k);
}

extern "C" int fusg_background_median_host(const void* const* frame_ptrs, int32_t T, int32_t H, int32_t W, const int32_t* boxes,
                                           const int32_t* box_offs, int32_t margin, int32_t min_valid, uint8_t* bg_out, uint8_t* count) {
    BgK k;
    const int rc = background_check(frame_ptrs, T, H, W, boxes, box_offs, margin, min_valid, bg_out, count, "background_median_host", k);
    if (rc != FUSG_OK) return rc;
    switch (bg::bucket(T)) {
        case 8: background_host_tb<8>(k); break;
        case 16: background_host_tb<16>(k); break;
        case 32: background_host_tb<32>(k); break;
        default: background_host_tb<64>(k); break;
    }
    return FUSG_OK;
}
