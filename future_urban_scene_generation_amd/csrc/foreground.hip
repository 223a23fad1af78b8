// Vehicle masks from the estimated background (include/fusg.h: fusg_foreground_masks_u8) and the erase that uses them
// (fusg_erase_boxes_u8), each with a host twin by the same code.  foreground.h states the definition, the plane layout and why
// the floods end at the same bits on host and device.  Off every product pass: nothing calls this unless asked.
//   mask kernel   one workgroup of 256 per box.  The thresholding is the only pass that touches the images: a wave takes 64
//                 consecutive pixels of a box row (3 bytes each from frame and background, consecutive lanes, consecutive
//                 addresses) and its ballot is two words of plane A.  Everything after that works on the two bit planes - in LDS
//                 when fg::in_lds(max_box) says so (dynamic LDS of exactly that size), else in the caller's scratch - and the
//                 last pass writes one byte per box pixel.  The workgroup is workgroup.h's wg::DevRed, the host twin wg::Host.
//   erase         two launches: dst = frame (dwords where the pointers allow it), then 16 workgroups per box put the
//                 background's three bytes wherever the box's mask byte is non-zero.  Overlapping boxes store equal bytes.
// No atomics.  A refused box (foreground.h: accept) is flagged by thread 0 and nothing of it is read or written.
#include <vector>
#include "common.h"
#include "foreground.h"

namespace fusg {

struct FgK {
    const unsigned char* frames[FUSG_MAX_FRAMES];
    const unsigned char* bgs[FUSG_MAX_FRAMES];
    int rows[FUSG_MAX_FRAMES + 1];                                // boxes [rows[f], rows[f + 1]) read frame f; past n_frames: n
    const int32_t* boxes;
    const int32_t* cores;
    const int64_t* offs;
    unsigned char* mask;
    long mask_len;
    int32_t* stats;
    uint32_t* scratch;
    int n_frames, H, W, n, max_h, max_w;
    fg::Params P;
};

// box b of the call -> what run_box takes; false: refused
FUSG_HD bool fg_box(const FgK& k, int b, fg::Box& bx) {
    const int32_t* r = k.boxes + 4L * b;
    const long off = (long)k.offs[b];
    if (!fg::accept(r, k.H, k.W, k.max_h, k.max_w, off, k.mask_len)) return false;
    int f = 0;
    while (f + 1 < k.n_frames && k.rows[f + 1] <= b) ++f;
    bx.frame = k.frames[f];
    bx.bgd = k.bgs[f];
    bx.mask = k.mask + off;
    bx.stats = k.stats + 4L * b;
    bx.W = k.W;
    bx.x0 = r[0];
    bx.y0 = r[1];
    bx.w = r[2] - r[0];
    bx.h = r[3] - r[1];
    fg::set_core(bx, k.cores + 4L * b);
    return true;
}

template <bool LDS>
__global__ __launch_bounds__(fg::THREADS) void foreground_masks_kernel(const FgK k) {
    extern __shared__ uint32_t s_planes[];
    __shared__ int s_red[4];
    const int b = (int)blockIdx.x;
    fg::Box bx;
    if (!fg_box(k, b, bx)) {                                      // uniform: every thread reads the same row
        if (threadIdx.x == 0) {
            int32_t* st = k.stats + 4L * b;
            st[0] = 0; st[1] = 0; st[2] = 0; st[3] = fg::FLAG_REFUSED;
        }
        return;
    }
    const long cap = fg::plane_words(k.max_h, k.max_w);
    uint32_t* A = LDS ? s_planes : k.scratch + (long)b * fg::PLANES * cap;
    wg::DevRed<fg::THREADS> ex{{}, s_red};
    fg::run_box(ex, bx, k.P, A, A + cap);
}

static int foreground_launch(FgK k, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (fg::in_lds(k.max_h, k.max_w))
        hipLaunchKernelGGL((foreground_masks_kernel<true>), dim3((unsigned)k.n), dim3(fg::THREADS), (size_t)fg::planes_bytes(k.max_h, k.max_w),
                           st, k);
    else
        hipLaunchKernelGGL((foreground_masks_kernel<false>), dim3((unsigned)k.n), dim3(fg::THREADS), 0, st, k);
    FUSG_LAUNCH_CHECK("foreground_masks_u8");
    return FUSG_OK;
}

static void foreground_host(const FgK& k) {
    wg::Host ex;
    for (int b = 0; b < k.n; ++b) {
        fg::Box bx;
        if (!fg_box(k, b, bx)) {
            int32_t* st = k.stats + 4L * b;
            st[0] = 0; st[1] = 0; st[2] = 0; st[3] = fg::FLAG_REFUSED;
            continue;
        }
        const long cap = (long)bx.h * fg::words(bx.w);            // exactly this box's planes
        std::vector<uint32_t> planes((size_t)(fg::PLANES * cap));
        fg::run_box(ex, bx, k.P, planes.data(), planes.data() + cap);
    }
}

// ---- erase: dst = frame, then background under every box's mask ----
struct EraseK {
    const unsigned char* frame;
    const unsigned char* bgd;
    const unsigned char* mask;
    const int64_t* offs;
    const int32_t* boxes;
    unsigned char* dst;
    long mask_len;
    int H, W, n;
};

// the pixels p, p + step, .. of box b; a box that fg::accept refuses (any extent allowed) is skipped
FUSG_HD void erase_box(const EraseK& k, int b, long p0, long step) {
    const int32_t* r = k.boxes + 4L * b;
    const long off = (long)k.offs[b];
    if (!fg::accept(r, k.H, k.W, fg::MAX_DIM, fg::MAX_DIM, off, k.mask_len)) return;
    const int w = r[2] - r[0], h = r[3] - r[1];
    const long np = (long)h * w;
    for (long p = p0; p < np; p += step) {
        if (k.mask[off + p] == 0) continue;
        const int i = (int)(p / w), j = (int)(p - (long)i * w);
        const long q = 3 * ((long)(r[1] + i) * k.W + r[0] + j);
        k.dst[q] = k.bgd[q];
        k.dst[q + 1] = k.bgd[q + 1];
        k.dst[q + 2] = k.bgd[q + 2];
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void erase_copy_kernel(const unsigned char* src, unsigned char* dst, long n_bytes) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (VEC) {
        if (4 * i + 4 <= n_bytes) {
            *(uint32_t*)(dst + 4 * i) = *(const uint32_t*)(src + 4 * i);
        } else {
            for (long q = 4 * i; q < n_bytes; ++q) dst[q] = src[q];
        }
    } else if (i < n_bytes) {
        dst[i] = src[i];
    }
}

// ERASE_SPLIT workgroups share a box's pixels (every pixel is on its own: nothing to agree on)
constexpr int ERASE_SPLIT = 16;
__global__ __launch_bounds__(256) void erase_boxes_kernel(const EraseK k) {
    erase_box(k, (int)blockIdx.x, (long)blockIdx.y * 256 + threadIdx.x, 256L * ERASE_SPLIT);
}

static int erase_launch(EraseK k, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const long nb = 3L * k.H * k.W;
    if (((((uintptr_t)k.frame) | ((uintptr_t)k.dst)) & 3) == 0) {
        const long dw = (nb + 3) / 4;
        hipLaunchKernelGGL((erase_copy_kernel<true>), dim3((unsigned)((dw + 255) / 256)), dim3(256), 0, st, k.frame, k.dst, nb);
    } else {
        hipLaunchKernelGGL((erase_copy_kernel<false>), dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, st, k.frame, k.dst, nb);
    }
    if (k.n > 0) hipLaunchKernelGGL(erase_boxes_kernel, dim3((unsigned)k.n, ERASE_SPLIT), dim3(256), 0, st, k);
    FUSG_LAUNCH_CHECK("erase_boxes_u8");
    return FUSG_OK;
}

}  // namespace fusg

using namespace fusg;

// every table and range, on the host, before anything is launched; n == 0 passes with empty tables
static int foreground_check(const void* const* frames, const void* const* backgrounds, const int32_t* frame_rows, int32_t n_frames,
                            int32_t H, int32_t W, const int32_t* boxes, const int32_t* cores, const int64_t* offsets, int32_t n,
                            int32_t thr, int32_t open_r, int32_t close_r, int32_t grow, int32_t fallback, int32_t max_box_h,
                            int32_t max_box_w, uint8_t* mask, int64_t mask_len, int32_t* stats, const char* what, FgK& k) {
    FUSG_CHECK(n >= 0, "%s: n = %d boxes", what, n);
    if (const int rc = fg::check_ranges(H, W, thr, open_r, close_r, what)) return rc;
    FUSG_CHECK(grow >= 0 && grow <= fg::MAX_GROW, "%s: grow = %d (0..%d)", what, grow, fg::MAX_GROW);
    FUSG_CHECK(max_box_h >= 0 && max_box_w >= 0 && max_box_h <= fg::MAX_DIM && max_box_w <= fg::MAX_DIM,
               "%s: max_box = %d x %d (0..%d)", what, max_box_h, max_box_w, fg::MAX_DIM);
    FUSG_CHECK(mask_len >= 0, "%s: a mask buffer of %lld bytes", what, (long long)mask_len);
    memset(&k, 0, sizeof(k));
    k.n = n;
    if (n == 0) return FUSG_OK;
    FUSG_CHECK(n_frames >= 1 && n_frames <= FUSG_MAX_FRAMES, "%s: n_frames = %d (1..%d)", what, n_frames, FUSG_MAX_FRAMES);
    FUSG_CHECK(frames && backgrounds && frame_rows, "%s: frames, backgrounds or frame_rows is null", what);
    FUSG_CHECK(boxes && cores && offsets && stats, "%s: boxes, cores, offsets or stats is null", what);
    FUSG_CHECK(mask != nullptr || mask_len == 0, "%s: a null mask buffer of %lld bytes", what, (long long)mask_len);
    FUSG_CHECK(frame_rows[0] == 0, "%s: frame_rows starts at %d, not at 0", what, frame_rows[0]);
    for (int f = 0; f < n_frames; ++f) {
        FUSG_CHECK(frame_rows[f + 1] >= frame_rows[f], "%s: frame_rows decreases at frame %d", what, f);
        k.rows[f + 1] = frame_rows[f + 1];
    }
    if (const int rc = wg::check_frame_pairs(frames, backgrounds, n_frames, k.frames, k.bgs, what)) return rc;
    FUSG_CHECK(frame_rows[n_frames] == n, "%s: frame_rows ends at %d, not at the %d boxes", what, frame_rows[n_frames], n);
    for (int f = n_frames; f < FUSG_MAX_FRAMES; ++f) k.rows[f + 1] = n;
    k.boxes = boxes; k.cores = cores; k.offs = offsets; k.mask = mask; k.mask_len = (long)mask_len; k.stats = stats;
    k.n_frames = n_frames; k.H = H; k.W = W; k.max_h = max_box_h; k.max_w = max_box_w;
    k.P = fg::Params{thr, open_r, close_r, grow, fallback != 0 ? 1 : 0};
    return FUSG_OK;
}

extern "C" int64_t fusg_foreground_masks_scratch_bytes(int32_t n_boxes, int32_t max_box_h, int32_t max_box_w) {
    if (n_boxes < 0 || max_box_h < 0 || max_box_w < 0 || max_box_h > fg::MAX_DIM || max_box_w > fg::MAX_DIM) return -1;
    return fg::in_lds(max_box_h, max_box_w) ? 0 : (int64_t)n_boxes * fg::planes_bytes(max_box_h, max_box_w);
}

extern "C" int fusg_foreground_masks_u8(const void* const* frames, const void* const* backgrounds, const int32_t* frame_rows,
                                        int32_t n_frames, int32_t H, int32_t W, const int32_t* boxes, const int32_t* cores,
                                        const int64_t* offsets, int32_t n, int32_t thr, int32_t open_r, int32_t close_r, int32_t grow,
                                        int32_t fallback, int32_t max_box_h, int32_t max_box_w, uint8_t* mask, int64_t mask_len,
                                        int32_t* stats, void* scratch, void* stream) {
    FgK k;
    const int rc = foreground_check(frames, backgrounds, frame_rows, n_frames, H, W, boxes, cores, offsets, n, thr, open_r, close_r, grow,
                                    fallback, max_box_h, max_box_w, mask, mask_len, stats, "foreground_masks_u8", k);
    if (rc != FUSG_OK || n == 0) return rc;
    FUSG_CHECK(scratch != nullptr || fg::in_lds(max_box_h, max_box_w),
               "foreground_masks_u8: boxes of up to %d x %d need %lld bytes of scratch (fusg_foreground_masks_scratch_bytes), got null",
               max_box_h, max_box_w, (long long)fusg_foreground_masks_scratch_bytes(n, max_box_h, max_box_w));
    FUSG_CHECK((((uintptr_t)scratch) & 3) == 0, "foreground_masks_u8: the scratch is not 4-byte aligned");
    k.scratch = (uint32_t*)scratch;
    return fusg::plan_dispatch(foreground_launch, stream, k);
}

extern "C" int fusg_foreground_masks_host(const void* const* frames, const void* const* backgrounds, const int32_t* frame_rows,
                                          int32_t n_frames, int32_t H, int32_t W, const int32_t* boxes, const int32_t* cores,
                                          const int64_t* offsets, int32_t n, int32_t thr, int32_t open_r, int32_t close_r, int32_t grow,
                                          int32_t fallback, int32_t max_box_h, int32_t max_box_w, uint8_t* mask, int64_t mask_len,
                                          int32_t* stats) {
    FgK k;
    const int rc = foreground_check(frames, backgrounds, frame_rows, n_frames, H, W, boxes, cores, offsets, n, thr, open_r, close_r, grow,
                                    fallback, max_box_h, max_box_w, mask, mask_len, stats, "foreground_masks_host", k);
    if (rc != FUSG_OK || n == 0) return rc;
    foreground_host(k);
    return FUSG_OK;
}

static int erase_check(const uint8_t* frame, const uint8_t* background, int32_t H, int32_t W, const uint8_t* mask, int64_t mask_len,
                       const int64_t* offsets, const int32_t* boxes, int32_t n, uint8_t* dst, const char* what, EraseK& k) {
    FUSG_CHECK(n >= 0, "%s: n = %d boxes", what, n);
    if (const int rc = wg::check_frame_size(H, W, what)) return rc;
    FUSG_CHECK(frame && background && dst, "%s: frame, background or dst is null", what);
    FUSG_CHECK(mask_len >= 0 && (mask != nullptr || mask_len == 0), "%s: a mask buffer of %lld bytes at %p", what, (long long)mask_len,
               (const void*)mask);
    FUSG_CHECK(n == 0 || (offsets && boxes), "%s: %d boxes and a null offsets or boxes table", what, n);
    const long nb = 3L * H * W;
    FUSG_CHECK((dst + nb <= frame || frame + nb <= dst) && (dst + nb <= background || background + nb <= dst),
               "%s: dst overlaps the frame or the background", what);
    k = EraseK{frame, background, mask, offsets, boxes, dst, (long)mask_len, H, W, n};
    return FUSG_OK;
}

extern "C" int fusg_erase_boxes_u8(const uint8_t* frame, const uint8_t* background, int32_t H, int32_t W, const uint8_t* mask,
                                   int64_t mask_len, const int64_t* offsets, const int32_t* boxes, int32_t n, uint8_t* dst, void* stream) {
    EraseK k;
    const int rc = erase_check(frame, background, H, W, mask, mask_len, offsets, boxes, n, dst, "erase_boxes_u8", k);
    if (rc != FUSG_OK) return rc;
    return fusg::plan_dispatch(erase_launch, stream, k);
}

extern "C" int fusg_erase_boxes_host(const uint8_t* frame, const uint8_t* background, int32_t H, int32_t W, const uint8_t* mask,
                                     int64_t mask_len, const int64_t* offsets, const int32_t* boxes, int32_t n, uint8_t* dst) {
    EraseK k;
    const int rc = erase_check(frame, background, H, W, mask, mask_len, offsets, boxes, n, dst, "erase_boxes_host", k);
    if (rc != FUSG_OK) return rc;
    memcpy(dst, frame, (size_t)(3L * H * W));
    for (int b = 0; b < n; ++b) erase_box(k, b, 0L, 1L);
    return FUSG_OK;
}
