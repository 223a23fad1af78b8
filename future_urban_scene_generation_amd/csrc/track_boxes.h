// Linking per-frame vehicle boxes into trajectories, for host and device: the arithmetic fusg_link_boxes (track_boxes.hip) and its
// host twin share.  Integer from end to end.  The definition, per video s of S, each on its own.  The video's frames in this call
// have the absolute indices t = t0, t0 + 1, ...; frame t has n_t = clamp(stats[t][0], 0, K) detections boxes[t][0 .. n_t), half-open
// (x0, y0, x1, y1), exactly the tables fusg_foreground_boxes_u8 writes.  The call's parameters: the rational threshold iou_num /
// iou_den (0 < num <= den <= 1024), max_gap (0..255), predict (0 or 1) and max_tracks N.
//   track     id, first_t, last_t, hits, its last observed box, and the observation before it (prev_t and box)
//   live      a track is live at t while t - last_t <= max_gap + 1.  The live tracks are kept in ascending id, at most LIVE_MAX
//   expected  the expected box of a live track at t is its last box; with predict = 1 and hits >= 2 it is shifted in x by
//             tdiv(((x0 + x1)_last - (x0 + x1)_prev) (t - last_t), 2 (last_t - prev_t)) and likewise in y.  tdiv is C++'s division,
//             which TRUNCATES towards zero (numpy's // floors).  The size is kept and nothing is clipped
//   pair      (track a, detection d): inter = the area both boxes share, uni = area_a + area_d - inter.  ELIGIBLE when inter > 0
//             and inter iou_den >= iou_num uni.  Pair p is BETTER than q when inter_p uni_q > inter_q uni_p; on a tie the smaller
//             track id wins, then the smaller detection index: a strict total order of the pairs of a frame
//   BAD_BOX   a detection that is empty (x1 <= x0 or y1 <= y0) or has a coordinate outside [0, MAX_COORD = 16384] takes no part: it
//             gets id -1 and sets the flag.  The bound is what keeps the arithmetic exact: a side is <= 2^14, so inter <= 2^28 and
//             uni <= 2^29 (an expected box keeps the size of an observed one, wherever the shift puts it), inter iou_den and
//             iou_num uni are <= 2^39, and the products of `better` are <= 2^57 - every product stays below 2^58 in int64.  The
//             shift's numerator is at most 2^15 (max_gap + 1) < 2^24
//   matching  within a frame, repeatedly take the best eligible pair among the unmatched tracks and detections until none is
//             left.  This SEQUENTIAL GREEDY is the definition
//   after     a matched detection takes its track's id; the track's prev becomes its last, its last the detection, hits + 1.  The
//             unmatched detections (BAD_BOX ones aside) found new tracks in detection order with the ids next_id, next_id + 1, ...;
//             a birth at next_id == N is refused (id -1, flag TRACKS_FULL), else a birth with LIVE_MAX tracks live is refused
//             (id -1, flag LIVE_FULL).  A new track cannot be matched in the frame that founds it
//   outputs   ids int32 [frames][K], -1 from n_t on, written whole.  tracks int32 [N][4] = (first_t, last_t, hits, 0): the row of
//             every track that was live at some frame of this call or is live at its end is written, the rows from next_id on are
//             zeros, and the rows of tracks that had died before the call keep what the earlier call left - from a zeroed state the
//             table is written whole, and a caller that carries the state carries this table with it.  out int32 [4] = (n_tracks
//             = next_id, n_live = the live table's rows after the last frame, n_linked = the matched detections since the state was
//             zeroed, flags since then)
//   state     int32 [STATE_WORDS], in and out: (next_id, n_live, flags, next_t = the last frame index seen + 1, n_linked, 0, 0, 0)
//             and LIVE_MAX records of REC words (id, first_t, last_t, hits, prev_t, last box, prev box), zeros past n_live: a
//             zeroed state is a fresh video.  Tracks expire at the START of a frame, so the state after frame t is the same whether
//             the call ends there or goes on: a video cut into successive calls gives the bits of one long call.  A call whose t0
//             is below next_t is refused: flag ORDER in out only, ids -1, state and tracks untouched.  A state whose header cannot
//             be one (counts outside their ranges) is refused likewise with BAD_STATE; a record's id is checked again where it
//             indexes tracks.
//
// How the kernel reaches the greedy matching: in ROUNDS.  In a round every unmatched track finds its best eligible unmatched
// detection and every unmatched detection its best eligible unmatched track, all at once; a pair that chose each other is
// matched; the rounds end when one matches nothing.  Why that is the sequential greedy: `better` with its ties is a strict total
// order.  (1) A pair (a, d) that chose each other is taken by the greedy: the greedy walks the eligible pairs best first and skips
// a pair only when a better pair sharing a or d was taken before; among the still unmatched there is none (d is a's best, a is
// d's), and the ones matched in earlier rounds are, by induction, greedy pairs that hold neither a nor d.  (2) While an eligible
// pair is left among the unmatched, the best of them chose each other, so a round that matches nothing leaves none: the greedy
// has nothing more to take either.  The host twin runs the same rounds on one thread.
#pragma once
#include <stdint.h>
#include "resize.h"

namespace fusg {
namespace trk {

constexpr int LIVE_MAX = 128, MAX_K = 64, MAX_VIDEOS = 64, THREADS = 256;
constexpr int MAX_COORD = 16384, MAX_DEN = 1024, MAX_GAP = 255, MAX_TRACKS = 1 << 20, MAX_T = 1 << 30;
constexpr int HDR = 8, REC = 13, STATE_WORDS = HDR + LIVE_MAX * REC;
enum { FLAG_BAD_BOX = 1, FLAG_TRACKS_FULL = 2, FLAG_LIVE_FULL = 4, FLAG_ORDER = 8, FLAG_BAD_STATE = 16 };
enum { R_ID = 0, R_FIRST = 1, R_LAST = 2, R_HITS = 3, R_PREV = 4, R_BOX = 5, R_PBOX = 9 };        // a record's words
enum { UNMATCHED = -1, NO_PART = -2 };

struct Params { int iou_num, iou_den, max_gap, predict, max_tracks; };

// what a video's workgroup keeps in LDS (the host twin: on its stack)
struct Work {
    int32_t hdr[HDR];
    int32_t rec[2][LIVE_MAX * REC];                               // the live table, twice: expiry compacts from one into the other
    int32_t ebox[LIVE_MAX * 4], dbox[MAX_K * 4];                  // the frame's expected boxes and detections
    int32_t keep[LIVE_MAX], trk_det[LIVE_MAX], best_d[LIVE_MAX];  // per live track
    int32_t det_trk[MAX_K], rank[MAX_K];                          // per detection
    int32_t best_a[MAX_K * 2], best_i[MAX_K * 2], best_u[MAX_K * 2];   // a detection's best track in each half of the live table
    int32_t tmp[4];
};

FUSG_HD int64_t tdiv(int64_t a, int64_t b) { return a / b; }      // truncates towards zero

FUSG_HD bool box_ok(const int32_t* b) {
    return b[0] >= 0 && b[1] >= 0 && b[2] <= MAX_COORD && b[3] <= MAX_COORD && b[2] > b[0] && b[3] > b[1];
}

FUSG_HD void expected(const int32_t* r, int t, int predict, int32_t* e) {
    int64_t dx = 0, dy = 0;
    const int64_t den = 2 * ((int64_t)r[R_LAST] - r[R_PREV]);     // > 0 in every record a call wrote with hits >= 2
    if (predict != 0 && r[R_HITS] >= 2 && den > 0) {
        const int64_t dt = (int64_t)t - r[R_LAST];
        dx = tdiv(((int64_t)(r[R_BOX] + r[R_BOX + 2]) - (r[R_PBOX] + r[R_PBOX + 2])) * dt, den);
        dy = tdiv(((int64_t)(r[R_BOX + 1] + r[R_BOX + 3]) - (r[R_PBOX + 1] + r[R_PBOX + 3])) * dt, den);
    }
    e[0] = (int32_t)(r[R_BOX] + dx);
    e[1] = (int32_t)(r[R_BOX + 1] + dy);
    e[2] = (int32_t)(r[R_BOX + 2] + dx);
    e[3] = (int32_t)(r[R_BOX + 3] + dy);
}

// inter and uni of an expected box and a detection -> eligible
FUSG_HD bool pair(const int32_t* e, const int32_t* d, const Params& P, int64_t& inter, int64_t& uni) {
    const int64_t w = (int64_t)(e[2] < d[2] ? e[2] : d[2]) - (e[0] > d[0] ? e[0] : d[0]);
    const int64_t h = (int64_t)(e[3] < d[3] ? e[3] : d[3]) - (e[1] > d[1] ? e[1] : d[1]);
    inter = w > 0 && h > 0 ? w * h : 0;
    uni = (int64_t)(e[2] - e[0]) * (e[3] - e[1]) + (int64_t)(d[2] - d[0]) * (d[3] - d[1]) - inter;
    return inter > 0 && inter * P.iou_den >= (int64_t)P.iou_num * uni;
}

FUSG_HD bool better(int64_t ip, int64_t up, int64_t iq, int64_t uq) { return ip * uq > iq * up; }

FUSG_HD void track_row(int32_t* tracks, const int32_t* r, int next_id) {
    const int id = r[R_ID];
    if (id < 0 || id >= next_id) return;                          // only a state that no call wrote holds such a record
    int32_t* o = tracks + 4L * id;
    o[0] = r[R_FIRST]; o[1] = r[R_LAST]; o[2] = r[R_HITS]; o[3] = 0;
}

// Ex: who runs it - tid(), nth() (1, or at least 2 LIVE_MAX), sync() a barrier, any(p) a vote that is a barrier too.  Every branch
// around a barrier below is on a value every member holds alike: read from `w` after a barrier, from stats, or out of any().
template <class Ex>
FUSG_HD void link_video(Ex& ex, Work& w, const int32_t* boxes, const int32_t* stats, int T, int t0, int K, const Params& P,
                        int32_t* state, int32_t* ids, int32_t* tracks, int32_t* out) {
    const int t = ex.tid(), NT = ex.nth(), N = P.max_tracks;
    for (int e = t; e < HDR; e += NT) w.hdr[e] = state[e];
    ex.sync();
    int next_id = w.hdr[0], L = w.hdr[1], flags = w.hdr[2], next_t = w.hdr[3], linked = w.hdr[4];
    const bool bad = next_id < 0 || next_id > N || L < 0 || L > LIVE_MAX || L > next_id || next_t < 0 || next_t > MAX_T || linked < 0 ||
                     (flags & ~31) != 0;
    if (bad || (T > 0 && t0 < next_t)) {
        for (long e = t; e < (long)T * K; e += NT) ids[e] = -1;
        if (t == 0) {
            out[0] = next_id; out[1] = L; out[2] = linked;
            out[3] = bad ? FLAG_BAD_STATE : flags | FLAG_ORDER;
        }
        return;
    }
    int cur = 0;
    for (int e = t; e < L * REC; e += NT) w.rec[0][e] = state[HDR + e];
    ex.sync();
    for (int j = 0; j < T; ++j) {
        const int ft = t0 + j;
        const int32_t* fb = boxes + 4L * K * j;
        const int sn = stats[4L * j], n = sn < 0 ? 0 : sn > K ? K : sn;
        // tracks that are no longer live leave the table, the rest close ranks in their order
        bool drop = false;
        for (int a = t; a < L; a += NT) {
            const int k = ft - w.rec[cur][a * REC + R_LAST] <= P.max_gap + 1 ? 1 : 0;
            w.keep[a] = k;
            drop |= k == 0;
        }
        for (int d = t; d < n; d += NT) {
            for (int c = 0; c < 4; ++c) w.dbox[4 * d + c] = fb[4 * d + c];
            w.det_trk[d] = box_ok(fb + 4 * d) ? UNMATCHED : NO_PART;
        }
        if (ex.any(drop)) {
            for (int a = t; a < L; a += NT) {
                int pos = 0;
                for (int b = 0; b < a; ++b) pos += w.keep[b];
                const int32_t* r = w.rec[cur] + a * REC;
                if (w.keep[a] != 0)
                    for (int c = 0; c < REC; ++c) w.rec[cur ^ 1][pos * REC + c] = r[c];
                else
                    track_row(tracks, r, next_id);
                if (a == L - 1) w.tmp[3] = pos + w.keep[a];
            }
            ex.sync();
            L = w.tmp[3];
            cur ^= 1;
        }
        int32_t* rec = w.rec[cur];
        for (int a = t; a < L; a += NT) {
            expected(rec + a * REC, ft, P.predict, w.ebox + 4 * a);
            w.trk_det[a] = UNMATCHED;
        }
        ex.sync();
        for (;;) {
            // items 0 .. LIVE_MAX - 1: a track over the detections; the rest: a detection over one half of the live table
            for (int it = t; it < LIVE_MAX + 2 * MAX_K; it += NT) {
                int64_t bi = 0, bu = 1, pi, pu;
                int best = -1;
                if (it < LIVE_MAX) {
                    const int a = it;
                    if (a >= L) continue;
                    if (w.trk_det[a] == UNMATCHED)
                        for (int d = 0; d < n; ++d)
                            if (w.det_trk[d] == UNMATCHED && pair(w.ebox + 4 * a, w.dbox + 4 * d, P, pi, pu) && (best < 0 || better(pi, pu, bi, bu))) {
                                best = d; bi = pi; bu = pu;
                            }
                    w.best_d[a] = best;
                } else {
                    const int d = (it - LIVE_MAX) >> 1, half = (it - LIVE_MAX) & 1;
                    if (d >= n) continue;
                    const int a1 = L < (half + 1) * (LIVE_MAX / 2) ? L : (half + 1) * (LIVE_MAX / 2);
                    if (w.det_trk[d] == UNMATCHED)
                        for (int a = half * (LIVE_MAX / 2); a < a1; ++a)
                            if (w.trk_det[a] == UNMATCHED && pair(w.ebox + 4 * a, w.dbox + 4 * d, P, pi, pu) && (best < 0 || better(pi, pu, bi, bu))) {
                                best = a; bi = pi; bu = pu;
                            }
                    w.best_a[2 * d + half] = best;
                    w.best_i[2 * d + half] = (int32_t)bi;
                    w.best_u[2 * d + half] = (int32_t)bu;
                }
            }
            ex.sync();
            bool matched = false;
            for (int d = t; d < n; d += NT) {
                if (w.det_trk[d] != UNMATCHED) continue;
                const int a0 = w.best_a[2 * d], a1 = w.best_a[2 * d + 1];
                int a = a0 < 0 ? a1 : a0;                         // the lower half holds the smaller ids: it wins a tie
                if (a0 >= 0 && a1 >= 0 && better(w.best_i[2 * d + 1], w.best_u[2 * d + 1], w.best_i[2 * d], w.best_u[2 * d])) a = a1;
                if (a >= 0 && w.best_d[a] == d) {
                    w.det_trk[d] = a;
                    w.trk_det[a] = d;
                    matched = true;
                }
            }
            if (!ex.any(matched)) break;
        }
        // births in detection order: rank = the unmatched detections before this one
        for (int d = t; d < n; d += NT) {
            int um = 0, mt = 0, np = 0;
            for (int b = 0; b < d; ++b) {
                const int s = w.det_trk[b];
                um += s == UNMATCHED; mt += s >= 0; np += s == NO_PART;
            }
            w.rank[d] = um;
            if (d == n - 1) {
                const int s = w.det_trk[d];
                w.tmp[0] = um + (s == UNMATCHED); w.tmp[1] = mt + (s >= 0); w.tmp[2] = np + (s == NO_PART);
            }
        }
        if (n == 0 && t == 0) w.tmp[0] = w.tmp[1] = w.tmp[2] = 0;
        ex.sync();
        const int cand = w.tmp[0];
        int nb = cand;
        if (nb > N - next_id) nb = N - next_id;
        if (nb > LIVE_MAX - L) nb = LIVE_MAX - L;
        linked += w.tmp[1];
        if (w.tmp[2] > 0) flags |= FLAG_BAD_BOX;
        if (cand > nb) flags |= next_id + nb == N ? FLAG_TRACKS_FULL : FLAG_LIVE_FULL;
        for (int a = t; a < L; a += NT) {
            const int d = w.trk_det[a];
            if (d < 0) continue;
            int32_t* r = rec + a * REC;
            for (int c = 0; c < 4; ++c) { r[R_PBOX + c] = r[R_BOX + c]; r[R_BOX + c] = w.dbox[4 * d + c]; }
            r[R_PREV] = r[R_LAST];
            r[R_LAST] = ft;
            r[R_HITS] += 1;
        }
        for (int d = t; d < K; d += NT) {
            int id = -1;
            if (d < n) {
                const int s = w.det_trk[d];
                if (s >= 0) id = rec[s * REC + R_ID];
                else if (s == UNMATCHED && w.rank[d] < nb) {
                    id = next_id + w.rank[d];
                    int32_t* r = rec + (L + w.rank[d]) * REC;
                    r[R_ID] = id; r[R_FIRST] = ft; r[R_LAST] = ft; r[R_HITS] = 1; r[R_PREV] = ft;
                    for (int c = 0; c < 4; ++c) r[R_BOX + c] = r[R_PBOX + c] = w.dbox[4 * d + c];
                }
            }
            ids[(long)K * j + d] = id;
        }
        L += nb;
        next_id += nb;
        next_t = ft + 1;
        ex.sync();
    }
    const int32_t* rec = w.rec[cur];
    for (int a = t; a < L; a += NT) track_row(tracks, rec + a * REC, next_id);
    for (long e = 4L * next_id + t; e < 4L * N; e += NT) tracks[e] = 0;
    for (int e = t; e < LIVE_MAX * REC; e += NT) state[HDR + e] = e < L * REC ? rec[e] : 0;
    if (t == 0) {
        state[0] = next_id; state[1] = L; state[2] = flags; state[3] = next_t; state[4] = linked; state[5] = state[6] = state[7] = 0;
        out[0] = next_id; out[1] = L; out[2] = linked; out[3] = flags;
    }
}

}  // namespace trk
}  // namespace fusg
