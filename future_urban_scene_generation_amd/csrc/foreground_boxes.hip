// Vehicle boxes from the estimated background (include/fusg.h: fusg_foreground_boxes_u8), with a host twin by the same code.
// foreground_boxes.h states the definition, the record and plane layout and why host and device end at the same bits.  Off every
// product pass: nothing calls this unless asked.  Two launches:
//   cell pass    the only pass that touches the images.  A wave takes 64 consecutive pixels (3 bytes each from frame and
//                background, consecutive lanes, consecutive addresses) of each of a cell row's `cell` image rows - all the loads
//                issued before the first ballot - and ballots P.  Lane l < 64 / cell owns cell 64 c / cell + l: its bit field of
//                every ballot goes through fgb::CellAcc in registers, and it stores the cell's one record.  No LDS, no atomics.
//   label pass   one workgroup of 256 per frame, the two bit planes in dynamic LDS (fgb::planes_bytes, checked against the
//                budget on the host).  G0 by ballots over the records, the four fg::square passes, then the component loop of
//                fgb::label_frame.  The workgroup is workgroup.h's wg::DevRed with the Acc total added, the host twin wg::Host.
#include <vector>
#include "common.h"
#include "foreground_boxes.h"

namespace fusg {

struct BoxesK {
    const unsigned char* frames[FUSG_MAX_FRAMES];
    const unsigned char* bgs[FUSG_MAX_FRAMES];
    uint32_t* rec;                                                // [T][gh][gw]
    int32_t* boxes;                                               // [T][K][4]
    int32_t* box_stats;                                           // [T][K][2]
    int32_t* stats;                                               // [T][4]
    int T, H, W, gh, gw;
    fgb::Params P;
};

constexpr int BX_WAVES = fgb::THREADS / 64;

template <int CELL>
__global__ __launch_bounds__(fgb::THREADS) void foreground_cells_kernel(const BoxesK k) {
    constexpr int OWNERS = 64 / CELL;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int c = (int)blockIdx.x * BX_WAVES + wave, i = (int)blockIdx.y, f = (int)blockIdx.z;
    if (64 * c >= k.W) return;                                    // the whole wave; there is no barrier in this kernel
    const unsigned char* fr = k.frames[f];
    const unsigned char* bg = k.bgs[f];
    const int x = 64 * c + lane;
    bool p[CELL];
#pragma unroll
    for (int r = 0; r < CELL; ++r) {
        const int y = i * CELL + r;
        p[r] = x < k.W && y < k.H && fgb::pix(fr, bg, k.W, x, y, k.P);
    }
    fgb::CellAcc acc;
    const int sh = (lane * CELL) & 63;
#pragma unroll
    for (int r = 0; r < CELL; ++r) {
        const unsigned long long bal = __ballot(p[r]);
        acc.row((uint32_t)(bal >> sh) & ((1u << CELL) - 1u), r);
    }
    const int j = c * OWNERS + lane;
    if (lane < OWNERS && j < k.gw) k.rec[((long)f * k.gh + i) * k.gw + j] = acc.pack();
}

struct BoxesDev : wg::DevRed<fgb::THREADS> {                     // red: LDS int [BX_WAVES * 6]
    __device__ void total(fgb::Acc& a) const {
        for (int o = 32; o > 0; o >>= 1) {
            a.n_cells += __shfl_xor(a.n_cells, o);
            a.area += __shfl_xor(a.area, o);
            a.x0 = ::min(a.x0, __shfl_xor(a.x0, o));
            a.y0 = ::min(a.y0, __shfl_xor(a.y0, o));
            a.x1 = ::max(a.x1, __shfl_xor(a.x1, o));
            a.y1 = ::max(a.y1, __shfl_xor(a.y1, o));
        }
        if ((threadIdx.x & 63) == 0) {
            int* r = red + 6 * (threadIdx.x >> 6);
            r[0] = a.n_cells; r[1] = a.area; r[2] = a.x0; r[3] = a.y0; r[4] = a.x1; r[5] = a.y1;
        }
        __syncthreads();
        a = fgb::Acc();
        for (int w = 0; w < BX_WAVES; ++w) {
            const int* r = red + 6 * w;
            a.n_cells += r[0];
            a.area += r[1];
            a.x0 = ::min(a.x0, r[2]);
            a.y0 = ::min(a.y0, r[3]);
            a.x1 = ::max(a.x1, r[4]);
            a.y1 = ::max(a.y1, r[5]);
        }
        __syncthreads();
    }
};

struct BoxesHost : wg::Host {
    void total(fgb::Acc&) const {}
};

// static LDS: the reductions' words and the 256 bytes __syncthreads_or takes (the resource-usage remark says 352 in all)
static_assert(sizeof(int) * BX_WAVES * 6 + 256 <= fgb::LDS_STATIC, "the static LDS exceeds what the budget sets aside");

__global__ __launch_bounds__(fgb::THREADS) void foreground_label_kernel(const BoxesK k) {
    extern __shared__ uint32_t s_grid[];
    __shared__ int s_red[BX_WAVES * 6];
    const int f = (int)blockIdx.x;
    const long cap = fgb::plane_words(k.gh, k.gw);
    BoxesDev ex{{{}, s_red}};
    fgb::label_frame(ex, k.rec + (long)f * k.gh * k.gw, k.gh, k.gw, k.P, s_grid, s_grid + cap, k.boxes + 4L * k.P.K * f,
                     k.box_stats + 2L * k.P.K * f, k.stats + 4L * f);
}

static int boxes_launch(BoxesK k, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(((k.W + 63) / 64 + BX_WAVES - 1) / BX_WAVES), (unsigned)k.gh, (unsigned)k.T);
    if (k.P.cell == 4) hipLaunchKernelGGL((foreground_cells_kernel<4>), grid, dim3(fgb::THREADS), 0, st, k);
    else if (k.P.cell == 8) hipLaunchKernelGGL((foreground_cells_kernel<8>), grid, dim3(fgb::THREADS), 0, st, k);
    else hipLaunchKernelGGL((foreground_cells_kernel<16>), grid, dim3(fgb::THREADS), 0, st, k);
    hipLaunchKernelGGL(foreground_label_kernel, dim3((unsigned)k.T), dim3(fgb::THREADS), (size_t)fgb::planes_bytes(k.gh, k.gw), st, k);
    FUSG_LAUNCH_CHECK("foreground_boxes_u8");
    return FUSG_OK;
}

// the cell pass on one thread: the same fields, one cell at a time
static void boxes_host(const BoxesK& k) {
    BoxesHost ex;
    const int cell = k.P.cell;
    const long cap = fgb::plane_words(k.gh, k.gw);
    std::vector<uint32_t> rec((size_t)k.gh * k.gw), planes((size_t)(fgb::PLANES * cap));
    for (int f = 0; f < k.T; ++f) {
        for (int i = 0; i < k.gh; ++i)
            for (int j = 0; j < k.gw; ++j) {
                fgb::CellAcc acc;
                for (int r = 0; r < cell && i * cell + r < k.H; ++r) {
                    uint32_t field = 0u;
                    for (int q = 0; q < cell && j * cell + q < k.W; ++q)
                        field |= (uint32_t)fgb::pix(k.frames[f], k.bgs[f], k.W, j * cell + q, i * cell + r, k.P) << q;
                    acc.row(field, r);
                }
                rec[(size_t)i * k.gw + j] = acc.pack();
            }
        fgb::label_frame(ex, rec.data(), k.gh, k.gw, k.P, planes.data(), planes.data() + cap, k.boxes + 4L * k.P.K * f,
                         k.box_stats + 2L * k.P.K * f, k.stats + 4L * f);
    }
}

}  // namespace fusg

using namespace fusg;

// every range, on the host, before anything is launched or touched
static int boxes_check(const void* const* frames, const void* const* backgrounds, int32_t T, int32_t H, int32_t W, int32_t thr,
                       int32_t cell, int32_t min_count, int32_t open_r, int32_t close_r, int32_t min_area, int32_t min_w, int32_t min_h,
                       const int32_t* roi, int32_t K, int32_t* boxes, int32_t* box_stats, int32_t* stats, const char* what, BoxesK& k) {
    FUSG_CHECK(T >= 1 && T <= FUSG_MAX_FRAMES, "%s: T = %d frames (1..%d)", what, T, FUSG_MAX_FRAMES);
    FUSG_CHECK(frames && backgrounds, "%s: frames or backgrounds is null", what);
    if (const int rc = fg::check_ranges(H, W, thr, open_r, close_r, what)) return rc;
    FUSG_CHECK(cell == 4 || cell == 8 || cell == 16, "%s: cell = %d (4, 8 or 16)", what, cell);
    FUSG_CHECK(min_count >= 1 && min_count <= cell * cell, "%s: min_count = %d (1..%d for cell %d)", what, min_count, cell * cell, cell);
    FUSG_CHECK(min_area >= 1 && min_w >= 1 && min_h >= 1, "%s: min_area, min_w, min_h = %d, %d, %d (each >= 1)", what, min_area, min_w, min_h);
    FUSG_CHECK(K >= 1 && K <= fgb::MAX_K, "%s: K = %d boxes per frame (1..%d)", what, K, fgb::MAX_K);
    FUSG_CHECK(roi != nullptr, "%s: roi is null", what);
    FUSG_CHECK(roi[0] >= 0 && roi[1] >= 0 && roi[2] >= roi[0] && roi[3] >= roi[1] && roi[2] <= W && roi[3] <= H,
               "%s: roi = (%d, %d, %d, %d) leaves the %d x %d frame or is inverted (x0, y0, x1, y1, half-open)", what, roi[0], roi[1],
               roi[2], roi[3], W, H);
    FUSG_CHECK(boxes && box_stats && stats, "%s: boxes, box_stats or stats is null", what);
    const int gh = fgb::cells(H, cell), gw = fgb::cells(W, cell);
    FUSG_CHECK(fgb::fits(gh, gw), "%s: a grid of %d x %d cells needs %ld bytes of LDS, the budget is %ld: raise cell (now %d)", what, gh, gw,
               fgb::planes_bytes(gh, gw) + fgb::LDS_STATIC, fgb::LDS_BUDGET, cell);
    memset(&k, 0, sizeof(k));
    if (const int rc = wg::check_frame_pairs(frames, backgrounds, T, k.frames, k.bgs, what)) return rc;
    k.boxes = boxes; k.box_stats = box_stats; k.stats = stats;
    k.T = T; k.H = H; k.W = W; k.gh = gh; k.gw = gw;
    k.P = fgb::Params{thr, cell, min_count, open_r, close_r, min_area, min_w, min_h, K, roi[0], roi[1], roi[2], roi[3]};
    return FUSG_OK;
}

extern "C" int64_t fusg_foreground_boxes_scratch_bytes(int32_t T, int32_t H, int32_t W, int32_t cell) {
    if (T < 1 || T > FUSG_MAX_FRAMES || H < 1 || W < 1 || H > fg::MAX_DIM || W > fg::MAX_DIM || (cell != 4 && cell != 8 && cell != 16)) return -1;
    return 4 * (int64_t)fgb::scratch_words(T, fgb::cells(H, cell), fgb::cells(W, cell));
}

extern "C" int fusg_foreground_boxes_u8(const void* const* frames, const void* const* backgrounds, int32_t T, int32_t H, int32_t W,
                                        int32_t thr, int32_t cell, int32_t min_count, int32_t open_r, int32_t close_r, int32_t min_area,
                                        int32_t min_w, int32_t min_h, const int32_t* roi, int32_t K, int32_t* boxes, int32_t* box_stats,
                                        int32_t* stats, void* scratch, void* stream) {
    BoxesK k;
    const int rc = boxes_check(frames, backgrounds, T, H, W, thr, cell, min_count, open_r, close_r, min_area, min_w, min_h, roi, K, boxes,
                               box_stats, stats, "foreground_boxes_u8", k);
    if (rc != FUSG_OK) return rc;
    FUSG_CHECK(scratch != nullptr, "foreground_boxes_u8: the scratch is null (fusg_foreground_boxes_scratch_bytes: %lld bytes)",
               (long long)fusg_foreground_boxes_scratch_bytes(T, H, W, cell));
    FUSG_CHECK((((uintptr_t)scratch) & 3) == 0, "foreground_boxes_u8: the scratch is not 4-byte aligned");
    k.rec = (uint32_t*)scratch;
    return fusg::plan_dispatch(boxes_launch, stream, k);
}

extern "C" int fusg_foreground_boxes_host(const void* const* frames, const void* const* backgrounds, int32_t T, int32_t H, int32_t W,
                                          int32_t thr, int32_t cell, int32_t min_count, int32_t open_r, int32_t close_r, int32_t min_area,
                                          int32_t min_w, int32_t min_h, const int32_t* roi, int32_t K, int32_t* boxes, int32_t* box_stats,
                                          int32_t* stats) {
    BoxesK k;
    const int rc = boxes_check(frames, backgrounds, T, H, W, thr, cell, min_count, open_r, close_r, min_area, min_w, min_h, roi, K, boxes,
                               box_stats, stats, "foreground_boxes_host", k);
    if (rc != FUSG_OK) return rc;
    boxes_host(k);
    return FUSG_OK;
}
