// The workgroup mechanics the video front end's stages share (background.hip, foreground.hip, foreground_boxes.hip,
// track_boxes.hip).  Each stage states its arithmetic once, in a header, as `template <class Ex>` code; Ex is who runs it:
//   tid() of nth() members take part; sync() is a barrier between them; any(p) a vote, sum(v) a total and min(v) a minimum over
//   all of them (barriers too, the same value in every member); plane(..) fills a bit plane and ends with a barrier.
// wg::Dev<THREADS> is a workgroup of THREADS (tid, nth, sync, any, plane), wg::DevRed<THREADS> adds sum and min on four LDS words of
// the caller's, and wg::Host is one of one: the host twin of a kernel is the same code run by it.
// A bit plane holds one bit per element, 32 per word, row stride nw words, bit j of word k = element 32 k + j, the bits past
// `width` in a row's last word 0.  plane(A, rows, width, nw, dflt, load, bit, fold): element (i, j) has the value load(i, j) and
// the bit bit(value); fold(value) is called once per member for the values it loaded, and on the device also for dflt, the value
// of the elements past the edge of a wave's 64 - so fold(dflt) must do nothing and bit(dflt) be 0.
// Also here: the limit on an image's height and width, and the entry checks that more than one stage makes in the same words.
#pragma once
#include "common.h"
#include "resize.h"                                               // FUSG_HD

namespace fusg {
namespace wg {

constexpr int MAX_DIM = 32767;                                    // H and W of a frame; bg:: and fg:: take it from here

struct Host {
    int tid() const { return 0; }
    int nth() const { return 1; }
    void sync() const {}
    bool any(bool p) const { return p; }
    int sum(int v) const { return v; }
    int min(int v) const { return v; }
    template <class V, class Load, class Bit, class Fold>
    void plane(uint32_t* A, int rows, int width, int nw, V, Load load, Bit bit, Fold fold) const {
        for (int i = 0; i < rows; ++i)
            for (int k = 0; k < nw; ++k) {
                uint32_t w = 0u;
                for (int j = 32 * k; j < width && j < 32 * k + 32; ++j) {
                    const V v = load(i, j);
                    fold(v);
                    w |= (uint32_t)bit(v) << (j & 31);
                }
                A[i * nw + k] = w;
            }
    }
};

template <int THREADS>
struct Dev {
    __device__ int tid() const { return (int)threadIdx.x; }
    __device__ int nth() const { return THREADS; }
    __device__ void sync() const { __syncthreads(); }
    __device__ bool any(bool p) const { return __syncthreads_or(p ? 1 : 0) != 0; }
    // a wave takes 64 consecutive elements of a row, consecutive lanes, and its ballot is two words of the plane, stored by lane 0
    template <class V, class Load, class Bit, class Fold>
    __device__ void plane(uint32_t* A, int rows, int width, int nw, V dflt, Load load, Bit bit, Fold fold) const {
        const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
        const int chunks = (width + 63) >> 6, items = rows * chunks;
        constexpr int WAVES = THREADS / 64, U = 8;                // U items a turn: their loads are all issued before the first ballot
        for (int it0 = wave; it0 < items; it0 += WAVES * U) {     // the same trips for every lane of a wave
            V v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int it = it0 + WAVES * u, i = it / chunks, j = (it - i * chunks) * 64 + lane;
                v[u] = it < items && j < width ? load(i, j) : dflt;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int it = it0 + WAVES * u, i = it / chunks, c = it - i * chunks;
                fold(v[u]);
                const unsigned long long bal = __ballot(bit(v[u]));
                if (lane == 0 && it < items) {
                    A[i * nw + 2 * c] = (uint32_t)bal;
                    if (2 * c + 1 < nw) A[i * nw + 2 * c + 1] = (uint32_t)(bal >> 32);
                }
            }
        }
        __syncthreads();
    }
};

template <int THREADS>
struct DevRed : Dev<THREADS> {
    static_assert(THREADS == 256, "the reductions combine four waves' words");
    int* red;                                                     // LDS int [4]
    // a shuffle inside the wave, one word a wave, two barriers
    template <class Op>
    __device__ int reduce(int v, Op op) const {
        for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o));
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
        __syncthreads();
        const int s = op(op(red[0], red[1]), op(red[2], red[3]));
        __syncthreads();
        return s;
    }
    __device__ int sum(int v) const { return reduce(v, [](int a, int b) { return a + b; }); }
    __device__ int min(int v) const { return reduce(v, [](int a, int b) { return ::min(a, b); }); }
};

// ---- entry checks, on the host, before anything is launched ----
inline int check_frame_size(int H, int W, const char* what) {
    FUSG_CHECK(H >= 1 && W >= 1 && H <= MAX_DIM && W <= MAX_DIM, "%s: frames of %d x %d (H and W in 1..%d)", what, H, W, MAX_DIM);
    return FUSG_OK;
}

// T frame / background pointer pairs, each non-null, into a kernel struct's arrays (FUSG_MAX_FRAMES each; the caller checked T)
inline int check_frame_pairs(const void* const* frames, const void* const* backgrounds, int T, const unsigned char** kf,
                             const unsigned char** kb, const char* what) {
    for (int f = 0; f < T; ++f) {
        FUSG_CHECK(frames[f] != nullptr && backgrounds[f] != nullptr, "%s: frame or background %d is null", what, f);
        kf[f] = (const unsigned char*)frames[f];
        kb[f] = (const unsigned char*)backgrounds[f];
    }
    return FUSG_OK;
}

}  // namespace wg
}  // namespace fusg
