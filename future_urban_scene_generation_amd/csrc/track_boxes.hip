// Linking per-frame vehicle boxes into trajectories (include/fusg.h: fusg_link_boxes), with a host twin by the same code.
// track_boxes.h states the definition, the state's layout and why rounds of mutual best choices end at the sequential greedy
// matching.  Off every product pass: nothing calls this unless asked.  One launch:
//   one workgroup of 256 per video, its frames in order.  The live table (twice, for the compaction), the frame's detections and
//   expected boxes and the rounds' choices sit in static LDS (trk::Work).  In a round the 128 x 64 pairs are shared over the
//   workgroup twice: threads 0..127 take a live track each over the detections, threads 128..255 a detection over one half of
//   the live table, 64 pairs a thread either way; the workgroup is workgroup.h's wg::Dev, the host twin wg::Host.
//   No atomics, no scratch memory, no floating point; every global store is a plain C++ store by a vector lane.
#include "common.h"
#include "track_boxes.h"
#include "workgroup.h"

namespace fusg {

struct LinkK {
    const int32_t* boxes;                                         // [frames][K][4]
    const int32_t* stats;                                         // [frames][4]
    int32_t* state;                                               // [S][STATE_WORDS]
    int32_t* ids;                                                 // [frames][K]
    int32_t* tracks;                                              // [S][N][4]
    int32_t* out;                                                 // [S][4]
    int32_t first[trk::MAX_VIDEOS + 1], t0[trk::MAX_VIDEOS];
    int S, K;
    trk::Params P;
};

template <class Ex>
FUSG_HD void link_one(Ex& ex, trk::Work& w, const LinkK& k, int s) {
    const long f0 = k.first[s];
    trk::link_video(ex, w, k.boxes + 4L * k.K * f0, k.stats + 4L * f0, k.first[s + 1] - k.first[s], k.t0[s], k.K, k.P,
                    k.state + (long)trk::STATE_WORDS * s, k.ids + (long)k.K * f0, k.tracks + 4L * k.P.max_tracks * s, k.out + 4L * s);
}

__global__ __launch_bounds__(trk::THREADS) void link_boxes_kernel(const LinkK k) {
    __shared__ trk::Work w;
    wg::Dev<trk::THREADS> ex;
    link_one(ex, w, k, (int)blockIdx.x);
}

static int link_launch(LinkK k, void* stream) {
    hipLaunchKernelGGL(link_boxes_kernel, dim3((unsigned)k.S), dim3(trk::THREADS), 0, (hipStream_t)stream, k);
    FUSG_LAUNCH_CHECK("link_boxes");
    return FUSG_OK;
}

}  // namespace fusg

using namespace fusg;

// every range, on the host, before anything is launched or touched
static int link_check(const int32_t* boxes, const int32_t* stats, const int32_t* first, const int32_t* t0, int32_t S, int32_t K,
                      int32_t iou_num, int32_t iou_den, int32_t max_gap, int32_t predict, int32_t max_tracks, int32_t* state,
                      int32_t* ids, int32_t* tracks, int32_t* out_stats, const char* what, LinkK& k) {
    FUSG_CHECK(S >= 1 && S <= trk::MAX_VIDEOS, "%s: S = %d videos (1..%d)", what, S, trk::MAX_VIDEOS);
    FUSG_CHECK(K >= 1 && K <= trk::MAX_K, "%s: K = %d boxes per frame (1..%d)", what, K, trk::MAX_K);
    FUSG_CHECK(iou_den >= 1 && iou_den <= trk::MAX_DEN && iou_num >= 1 && iou_num <= iou_den,
               "%s: iou = %d / %d (0 < num <= den <= %d)", what, iou_num, iou_den, trk::MAX_DEN);
    FUSG_CHECK(max_gap >= 0 && max_gap <= trk::MAX_GAP, "%s: max_gap = %d (0..%d)", what, max_gap, trk::MAX_GAP);
    FUSG_CHECK(predict == 0 || predict == 1, "%s: predict = %d (0 or 1)", what, predict);
    FUSG_CHECK(max_tracks >= 1 && max_tracks <= trk::MAX_TRACKS, "%s: max_tracks = %d (1..%d)", what, max_tracks, trk::MAX_TRACKS);
    FUSG_CHECK(first && t0, "%s: first or t0 is null", what);
    FUSG_CHECK(first[0] == 0, "%s: first[0] = %d (the offsets start at 0)", what, first[0]);
    memset(&k, 0, sizeof(k));
    for (int s = 0; s < S; ++s) {
        FUSG_CHECK(first[s + 1] >= first[s] && first[s + 1] <= trk::MAX_T, "%s: first[%d] = %d after first[%d] = %d (offsets must not fall)",
                   what, s + 1, first[s + 1], s, first[s]);
        FUSG_CHECK(t0[s] >= 0 && (int64_t)t0[s] + (first[s + 1] - first[s]) <= trk::MAX_T, "%s: t0[%d] = %d with %d frames (frame indices in 0..%d)",
                   what, s, t0[s], first[s + 1] - first[s], trk::MAX_T);
        k.first[s] = first[s];
        k.t0[s] = t0[s];
    }
    k.first[S] = first[S];
    FUSG_CHECK(state && tracks && out_stats, "%s: state, tracks or out_stats is null", what);
    FUSG_CHECK(first[S] == 0 || (boxes && stats && ids), "%s: boxes, stats or ids is null", what);
    k.boxes = boxes; k.stats = stats; k.state = state; k.ids = ids; k.tracks = tracks; k.out = out_stats;
    k.S = S; k.K = K;
    k.P = trk::Params{iou_num, iou_den, max_gap, predict, max_tracks};
    return FUSG_OK;
}

extern "C" int32_t fusg_link_boxes_state_words(void) { return trk::STATE_WORDS; }

extern "C" int fusg_link_boxes(const int32_t* boxes, const int32_t* stats, const int32_t* first, const int32_t* t0, int32_t S, int32_t K,
                               int32_t iou_num, int32_t iou_den, int32_t max_gap, int32_t predict, int32_t max_tracks, int32_t* state,
                               int32_t* ids, int32_t* tracks, int32_t* out_stats, void* stream) {
    LinkK k;
    const int rc = link_check(boxes, stats, first, t0, S, K, iou_num, iou_den, max_gap, predict, max_tracks, state, ids, tracks, out_stats,
                              "link_boxes", k);
    if (rc != FUSG_OK) return rc;
    return fusg::plan_dispatch(link_launch, stream, k);
}

extern "C" int fusg_link_boxes_host(const int32_t* boxes, const int32_t* stats, const int32_t* first, const int32_t* t0, int32_t S, int32_t K,
                                    int32_t iou_num, int32_t iou_den, int32_t max_gap, int32_t predict, int32_t max_tracks, int32_t* state,
                                    int32_t* ids, int32_t* tracks, int32_t* out_stats) {
    LinkK k;
    const int rc = link_check(boxes, stats, first, t0, S, K, iou_num, iou_den, max_gap, predict, max_tracks, state, ids, tracks, out_stats,
                              "link_boxes_host", k);
    if (rc != FUSG_OK) return rc;
    wg::Host ex;
    trk::Work w;
    for (int s = 0; s < S; ++s) link_one(ex, w, k, s);
    return FUSG_OK;
}
